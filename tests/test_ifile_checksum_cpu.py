"""Hadoop's IFile checksum trailer (mapred.uda.ifile.checksum) without a GPU: the host CRC32 and
crc32_combine against zlib, the trailer split of uncompressed and compressed partitions, and the CPU
backend stripping and verifying trailers as the bytes are pulled.
"""
import os
import random
import shutil
import struct
import subprocess
import zlib

import pytest

from uda_amd.bridge import UdaConsumer, UdaFallback, UdaProvider, run_reduce
from uda_amd.utils import datagen
from uda_amd.utils.mof import CODECS, encode_partitions

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPU = {"mapred.uda.merge.backend": "cpu"}
ALL_CODECS = [None, "snappy", "lzo", "lz4"]


def expected(maps, partition, key_class):
    recs = [kv for m in maps for kv in m[partition]]
    return sorted(recs, key=datagen.sort_key(key_class))


def same_records(recs, want, key_class):
    kf = datagen.sort_key(key_class)
    assert [kf(kv) for kv in recs] == [kf(kv) for kv in want]
    assert sorted(recs) == sorted(want)


def publish(provider, job, maps, codec=None, checksum=True, block_size=4096, corrupt=None, trailers=None):
    """Registers the maps' outputs in memory; corrupt(i, data, index) may change map i's bytes; trailers
    (a set of map numbers) limits the checksum to those maps."""
    ids = []
    for i, parts in enumerate(datagen.streams(maps)):
        mid = f"attempt_{job}_m_{i:06d}_0"
        data, index = encode_partitions(parts, codec, block_size, checksum and (trailers is None or i in trailers))
        if corrupt:
            data = corrupt(i, data, index)
        provider.add_mof_memory(job, mid, data, index)
        ids.append(mid)
    return ids


# ------------------------------------------------------------------------------------------ host CRC
def test_host_crc32_equals_zlib(native):
    assert native.crc32(b"") == 0
    assert native.crc32(b"123456789") == 0xCBF43926
    buf = random.Random(5).randbytes(9000)
    for n in range(71):
        assert native.crc32(buf[:n]) == zlib.crc32(buf[:n]), n
        assert native.crc32(buf[3:3 + n]) == zlib.crc32(buf[3:3 + n]), n
    for n in (4095, 4096, 4097, 8191):
        assert native.crc32(buf[:n], 0xDEADBEEF) == zlib.crc32(buf[:n], 0xDEADBEEF), n
        assert native.crc32(buf[100:n], native.crc32(buf[:100])) == zlib.crc32(buf[:n]), n


def test_crc32_combine_reproduces_the_crc_of_the_concatenation(native):
    buf = random.Random(6).randbytes(5000)
    for total in (0, 1, 9, 5000):
        for cut in (0, 1, total):
            if cut > total:
                continue
            a, b = buf[:cut], buf[cut:total]
            assert native.crc32_combine(zlib.crc32(a), zlib.crc32(b), len(b)) == zlib.crc32(buf[:total]), (total, cut)
    z = bytes(70000)
    assert native.crc32_combine(zlib.crc32(z[:1]), zlib.crc32(z[1:]), 69999) == zlib.crc32(z)


def test_native_selftest_under_sanitizers(tmp_path):
    """tests/native/ifile_checksum_selftest.cc with csrc/engine/ifile_checksum.cc under ASan + UBSan, as a
    program of its own; never loaded into Python."""
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "ifile_checksum_selftest")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I" + os.path.join(ROOT, "csrc", "include"),
                    os.path.join(ROOT, "tests", "native", "ifile_checksum_selftest.cc"),
                    os.path.join(ROOT, "csrc", "engine", "ifile_checksum.cc"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert " 0 failures" in r.stdout


# ------------------------------------------------------------------------------------------ the split
def test_writer_appends_the_trailer_and_counts_it_in_part_len(native):
    parts = datagen.streams(datagen.wordcount(num_maps=1, reducers=3, words_per_map=400, seed=3))[0]
    plain, index0 = encode_partitions(parts)
    data, index = encode_partitions(parts, checksum=True)
    assert len(data) == len(plain) + 4 * len(parts)
    for (start, raw, plen), (_, raw0, plen0), p in zip(index, index0, parts):
        assert raw == raw0 == len(p) and plen == raw + 4 and plen0 == raw0
        assert native.ifile_trailer_bytes(raw, plen) == 4 and native.ifile_trailer_bytes(raw0, plen0) == 0
        body = data[start:start + plen - 4]
        assert body == p
        assert struct.unpack(">I", data[start + plen - 4:start + plen])[0] == zlib.crc32(body)
    assert native.ifile_trailer_bytes(0, 4) == 0 and native.ifile_trailer_bytes(-1, 3) == 0
    assert native.ifile_trailer_bytes(100, 60) == 0 and native.ifile_trailer_bytes(100, 105) == 0


@pytest.mark.parametrize("codec", ["snappy", "lzo", "lz4"])
def test_framing_walk_finds_the_trailer_of_compressed_streams(native, codec):
    raw = datagen.streams(datagen.terasort(1, 1, 300, seed=9))[0][0]
    for block in (1000, 1 << 16):
        st = native.block_compress(CODECS[codec], raw, block)
        blocks = (len(raw) + block - 1) // block
        assert native.plan_block_streams(CODECS[codec], st) == (blocks, 0)
        assert native.plan_block_streams(CODECS[codec], st + struct.pack(">I", zlib.crc32(st))) == (blocks, 4)
        for extra in (1, 2, 3):  # malformed, as before
            with pytest.raises(ValueError):
                native.plan_block_streams(CODECS[codec], st + b"\x01" * extra)
        # what the writer makes is such a stream, and part_len counts the trailer while raw_len does not
        data, index = encode_partitions([raw], codec, block, checksum=True)
        assert index == [(0, len(raw), len(st) + 4)] and data[:-4] == st
        assert native.plan_block_streams(CODECS[codec], data) == (blocks, 4)


def test_a_final_zero_length_block_reads_as_the_checksum_of_nothing(native):
    """The one ambiguity of the rule "exactly four bytes left at a block boundary are the checksum": a
    trailer-less stream ending in a zero-length block (00 00 00 00). It is taken as a checksum of 0, which
    is crc32(b"") -- right for Hadoop's empty stream, and the stream's records are the same either way.
    Anywhere else a zero-length block stays a block."""
    zero = struct.pack(">I", 0)
    assert zlib.crc32(b"") == 0
    st = native.block_compress(CODECS["lz4"], b"hello world " * 300, 1 << 16)
    assert native.plan_block_streams(CODECS["lz4"], zero) == (0, 4)
    assert native.plan_block_streams(CODECS["lz4"], st + zero) == (1, 4)
    assert native.plan_block_streams(CODECS["lz4"], zero + st) == (1, 0)
    assert native.plan_block_streams(CODECS["lz4"], zero + st + zero + zero) == (1, 4)
    assert native.plan_block_streams(CODECS["lz4"], b"") == (0, 0)


# ------------------------------------------------------------------------------------------ CPU backend
@pytest.fixture
def provider():
    p = UdaProvider()
    yield p
    p.close()


@pytest.mark.parametrize("codec", ALL_CODECS, ids=[c or "none" for c in ALL_CODECS])
def test_cpu_backend_delivers_the_oracle_and_verifies(provider, codec):
    wc = datagen.wordcount(num_maps=6, reducers=2, words_per_map=3000, seed=21)
    ts = datagen.terasort(num_maps=7, reducers=2, rows_per_map=700, seed=22)
    for name, maps in (("wc", wc), ("ts", ts)):
        job = f"job_ck_{name}_{codec or 'none'}"
        ids = publish(provider, job, maps, codec)
        for r in range(2):
            # small fetch buffers: many chunks per partition, the trailer in a chunk of its own now and then
            recs, st, c = run_reduce("h", job, ids, r, datagen.TEXT, codec=codec, conf=CPU, max_buf_kb=16,
                                     kv_buf_size=8192)
            same_records(recs, expected(maps, r, datagen.TEXT), datagen.TEXT)
            assert st["ifile_checksum"] == "verified" and st["checksum_partitions"] == len(ids), st
            assert st["checksum_bytes"] > 0 and st["gpu_checksum_ms"] == 0, st
            assert c.failure_calls == 0


def test_trailer_in_a_fetch_chunk_of_its_own(provider):
    """A body that ends exactly where a fetch chunk does: the consumer stops reading at the EOF marker, so
    the fetcher has to go and get the trailer itself before it hands out the last records."""
    from uda_amd.utils.ifile import encode_stream, text
    page = os.sysconf("SC_PAGESIZE")
    part = encode_stream([(text(b"k" * 10), b"v" * (2 * page))])
    part = encode_stream([(text(b"k" * 10), b"v" * (2 * page - (len(part) - 2 * page)))])
    assert len(part) == 2 * page  # the fetch buffer below: the trailer is the partition's third chunk
    data, index = encode_partitions([part], checksum=True)
    provider.add_mof_memory("job_ck_edge", "attempt_job_ck_edge_m_000000_0", data, index)
    for good in (True, False):
        mid = "attempt_job_ck_edge_m_000000_0"
        if not good:
            mid = "attempt_job_ck_edge_m_000001_0"
            bad = bytearray(data)
            bad[-1] ^= 1
            provider.add_mof_memory("job_ck_edge", mid, bytes(bad), index)
        c = UdaConsumer(1, "job_ck_edge", f"attempt_job_ck_edge_r_000000_{int(good)}", datagen.TEXT, conf=CPU,
                        max_buf_kb=2 * page // 1024, min_buf_kb=4)
        c.fetch("h", "job_ck_edge", mid, 0)
        if good:
            assert len(c.wait(60)) == 1
            assert c.close()["ifile_checksum"] == "verified"
        else:
            with pytest.raises(UdaFallback, match="checksum"):
                c.wait(60)
            c.close()


def _flip_value_byte(victim, partition):
    def corrupt(i, data, index):
        if i != victim:
            return data
        start = index[partition][0]
        out = bytearray(data)
        out[start + 60] ^= 0x10  # inside the first record's 90-byte value: the framing stays valid
        return bytes(out)
    return corrupt


def test_a_flipped_value_byte_fails_the_task_once(provider):
    maps = datagen.terasort(num_maps=7, reducers=2, rows_per_map=700, seed=23)
    ids = publish(provider, "job_ck_bad", maps, corrupt=_flip_value_byte(3, 1))
    c = UdaConsumer(len(ids), "job_ck_bad", "attempt_job_ck_bad_r_000001_0", datagen.TEXT, conf=CPU)
    for m in ids:
        c.fetch("h", "job_ck_bad", m, 1)
    with pytest.raises(UdaFallback, match=r"IFile checksum mismatch in map output attempt_job_ck_bad_m_000003_0: "
                                          r"stored 0x[0-9a-f]{8}, computed 0x[0-9a-f]{8} over \d+ bytes"):
        c.wait(60)
    c.close()
    assert c.failure_calls == 1
    # the other partition of the same maps is intact
    recs, st, _ = run_reduce("h", "job_ck_bad", ids, 0, datagen.TEXT, conf=CPU)
    same_records(recs, expected(maps, 0, datagen.TEXT), datagen.TEXT)
    # off: stripped, not verified -- the flipped byte is delivered
    recs, st, c = run_reduce("h", "job_ck_bad", ids, 1, datagen.TEXT, conf=dict(CPU, **{"mapred.uda.ifile.checksum": "off"}))
    assert st["ifile_checksum"] == "off" and st["checksum_partitions"] == 0 and c.failure_calls == 0, st
    want = expected(maps, 1, datagen.TEXT)
    assert len(recs) == len(want) and sorted(recs) != sorted(want)


@pytest.mark.parametrize("codec", [None, "lz4"], ids=["none", "lz4"])
def test_a_flipped_trailer_byte_fails_the_task(provider, codec):
    maps = datagen.wordcount(num_maps=6, reducers=2, words_per_map=2000, seed=24)

    def corrupt(i, data, index):
        if i != 2:
            return data
        out = bytearray(data)
        out[index[0][0] + index[0][2] - 2] ^= 0x80
        return bytes(out)

    job = f"job_ck_tr_{codec or 'none'}"
    ids = publish(provider, job, maps, codec, corrupt=corrupt)
    c = UdaConsumer(len(ids), job, f"attempt_{job}_r_000000_0", datagen.TEXT, codec=codec, conf=CPU)
    for m in ids:
        c.fetch("h", job, m, 0)
    with pytest.raises(UdaFallback, match="checksum mismatch in map output attempt_%s_m_000002_0" % job):
        c.wait(60)
    c.close()
    assert c.failure_calls == 1


def test_hybrid_merge_verifies_too(provider, tmp_path):
    maps = datagen.terasort(num_maps=11, reducers=1, rows_per_map=300, seed=25)
    ids = publish(provider, "job_ck_hyb", maps)
    recs, st, _ = run_reduce("h", "job_ck_hyb", ids, 0, datagen.TEXT, approach=2, lpq_size=4, conf=CPU,
                             local_dirs=(str(tmp_path),))
    same_records(recs, expected(maps, 0, datagen.TEXT), datagen.TEXT)
    assert st["lpqs"] > 1 and st["ifile_checksum"] == "verified" and st["checksum_partitions"] == 11, st


def test_mixed_and_trailerless_jobs(provider):
    maps = datagen.wordcount(num_maps=6, reducers=1, words_per_map=1500, seed=26)
    for codec in (None, "snappy"):
        ids = publish(provider, f"job_ck_mix_{codec}", maps, codec, trailers={0, 2, 4})
        recs, st, _ = run_reduce("h", f"job_ck_mix_{codec}", ids, 0, datagen.TEXT, codec=codec, conf=CPU)
        same_records(recs, expected(maps, 0, datagen.TEXT), datagen.TEXT)
        assert st["ifile_checksum"] == "verified" and st["checksum_partitions"] == 3, st
        ids = publish(provider, f"job_ck_plain_{codec}", maps, codec, checksum=False)
        recs, st, _ = run_reduce("h", f"job_ck_plain_{codec}", ids, 0, datagen.TEXT, codec=codec, conf=CPU)
        same_records(recs, expected(maps, 0, datagen.TEXT), datagen.TEXT)
        assert st["ifile_checksum"] == "none" and st["checksum_partitions"] == 0 and st["checksum_bytes"] == 0, st


def test_an_unknown_value_fails_init():
    for bad in ("maybe", "AUTO", "on"):
        with pytest.raises(RuntimeError, match="mapred.uda.ifile.checksum"):
            UdaConsumer(1, "job_ck_conf", "attempt_job_ck_conf_r_000000_0", datagen.TEXT,
                        conf=dict(CPU, **{"mapred.uda.ifile.checksum": bad}))
    for ok in ("auto", "off"):
        UdaConsumer(1, "job_ck_conf", "attempt_job_ck_conf_r_000000_0", datagen.TEXT,
                    conf=dict(CPU, **{"mapred.uda.ifile.checksum": ok})).close()
