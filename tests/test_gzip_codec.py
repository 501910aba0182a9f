"""gzip map outputs (Hadoop's GzipCodec) on the host: gzip_decompress and the gzip-mode Inflater behind
BlockDecoder / host_decode_partition on the members of tests/gzip_cases.py (which Python's zlib has judged:
tests/test_gzip_cases_cpu.py) and on what gzip.compress writes, trailer detection behind one and behind
several members, the two codec resolvers, the MOF writer, reduce tasks on the CPU backend, and the inflater's
stand-alone sanitizer program in gzip mode."""
import collections
import gzip
import os
import struct
import zlib

import pytest

from tests.gzip_cases import (GZ_TEXT, gzip_valid_cases, header, header_matrix, invalid_members, member,
                              multi_member_cases)
from tests.test_zlib_codec import LEVELS, PAYLOADS
from uda_amd.utils import datagen

GZIP = 5
GZIP_CLASS = "org.apache.hadoop.io.compress.GzipCodec"
INVALID = invalid_members()


@pytest.fixture(scope="module")
def geometry(native):
    g = native.gpu_inflate_geometry()
    assert (g["window"], g["literal_stage"]) == (256, 64)  # what tests/test_gzip_cases_cpu.py judged the cases at
    return g


@pytest.fixture(scope="module")
def valid(geometry):
    return gzip_valid_cases(geometry["window"], geometry["literal_stage"])


@pytest.fixture(scope="module")
def matrix(geometry):
    return header_matrix(geometry["window"], geometry["literal_stage"])


def level_streams():
    """[(name, member, raw)] of gzip.compress at four levels; shared with tests/test_gpu_gzip_inflate.py."""
    return [("%s-l%d" % (name, level), gzip.compress(raw, level, mtime=0), raw)
            for name, raw in PAYLOADS.items() for level in LEVELS]


def ifile_crc(stream):
    return struct.pack(">I", zlib.crc32(stream))


def check_three_variants(native, name, stream, want):
    """The stream alone, with a correct IFile checksum behind it, and with four zero bytes behind it."""
    out, used = native.gzip_decompress(stream, len(want))
    assert out == want and used == len(stream), name
    assert native.host_decode_partition(GZIP, stream) == (want, 0), name
    for tail in (ifile_crc(stream), b"\x00\x00\x00\x00"):
        out, used = native.gzip_decompress(stream + tail, len(want))
        assert out == want and used == len(stream), name
        assert native.host_decode_partition(GZIP, stream + tail) == (want, 4), name


def test_valid_cases_bare_header(native, valid):
    for name, stream, want in valid:
        check_three_variants(native, name, stream, want)


def test_header_matrix(native, matrix):
    for name, stream, want, _ in matrix:
        check_three_variants(native, name, stream, want)


def test_gzip_compress_levels(native):
    for name, stream, want in level_streams():
        check_three_variants(native, name, stream, want)


def test_more_output_than_cap(native, valid):
    for name, stream, want in valid[:80]:
        if want:
            with pytest.raises(ValueError):
                native.gzip_decompress(stream, len(want) - 1)


def test_junk_behind_a_member_is_refused(native, valid):
    """No byte or the four of an IFile checksum are accepted behind the last member; 1, 2, 3, 5 or 8 are malformed.
    The member's own last four bytes (its ISIZE) are not taken for a trailer."""
    picked = valid[:6] + [("text", gzip.compress(GZ_TEXT, mtime=0), GZ_TEXT), ("empty", gzip.compress(b"", mtime=0), b"")]
    for name, stream, want in picked:
        for k in (1, 2, 3, 5, 8):
            with pytest.raises((ValueError, RuntimeError)):
                native.host_decode_partition(GZIP, stream + b"\x01" * k)
        for cut in (1, 4, 5, 8):
            with pytest.raises((ValueError, RuntimeError)):
                native.host_decode_partition(GZIP, stream[:-cut])


@pytest.mark.parametrize("feed", [1, 7, 4096])
def test_incremental_feeds(native, valid, matrix, feed):
    for name, stream, want in valid:
        assert native.block_decompress(GZIP, stream, feed) == want, name
    for name, stream, want, _ in matrix:
        if feed == 1 and len(stream) > 20000:
            continue
        assert native.block_decompress(GZIP, stream, feed) == want, name


def test_pieces_cut_inside_header_fextra_and_trailer(native):
    """The header is committed only once it is whole, and so is the trailer, wherever the feeds cut them: a feed
    size of k puts a cut behind byte k, 2k, ...; the sizes below cut the fixed header, XLEN, the FEXTRA bytes,
    FNAME, FHCRC and the trailer (whose offsets differ by header) in every place."""
    c = zlib.compressobj(6, zlib.DEFLATED, -15)
    body = c.compress(GZ_TEXT) + c.flush()
    for hdr in (header(), header(extra=b"0123456789abcdef" * 3), header(2, extra=b"xy", name=b"n", comment=b"c"),
                header(2), header(name=b"a-file-name")):
        stream = member(body, GZ_TEXT, hdr)
        assert zlib.decompress(stream, 31) == GZ_TEXT
        for feed in list(range(1, len(hdr) + 12)) + [len(stream) - k for k in range(1, 10)]:
            assert native.block_decompress(GZIP, stream, feed) == GZ_TEXT, (hdr[3], feed)


def test_multi_member_cases(native, geometry):
    for name, stream, want, _ in multi_member_cases(geometry["window"], geometry["literal_stage"]):
        check_three_variants(native, name, stream, want)
        for feed in (1, 7, 4096):
            assert native.block_decompress(GZIP, stream, feed) == want, (name, feed)


@pytest.mark.parametrize("name", [c[0] for c in INVALID])
def test_invalid_member_refused(native, name):
    stream = dict(INVALID)[name]
    with pytest.raises(ValueError):
        native.gzip_decompress(stream, 1 << 20)
    with pytest.raises((ValueError, RuntimeError)):
        native.host_decode_partition(GZIP, stream)
    for feed in (1, 7, 4096):
        with pytest.raises((ValueError, RuntimeError)):
            native.block_decompress(GZIP, stream, feed)


def test_invalid_second_member_refused(native, valid):
    good = valid[0][1]
    for name, stream in INVALID:
        if len(stream) >= 18 and stream[:3] == b"\x1f\x8b\x08":  # (what is taken for another member's start)
            with pytest.raises((ValueError, RuntimeError)):
                native.host_decode_partition(GZIP, good + stream)


def test_the_two_codec_resolvers(native):
    pkg = "org.apache.hadoop.io.compress."
    assert native.map_output_codec(GZIP_CLASS) == 5
    assert native.map_output_codec(pkg + "DefaultCodec") == 4
    assert native.map_output_codec(pkg + "DeflateCodec") == 4
    assert native.map_output_codec(pkg + "SnappyCodec") == 1
    assert native.map_output_codec("com.hadoop.compression.lzo.LzoCodec") == 2
    assert native.map_output_codec(pkg + "Lz4Codec") == 3
    assert native.map_output_codec("") == 0
    assert native.map_output_codec(pkg + "BZip2Codec") == -1
    assert native.map_output_codec(pkg + "ZStandardCodec") == -1
    assert native.codec_from_class(GZIP_CLASS) == -1  # the block and zlib entry points' table keeps its answers


def test_gzip_is_no_block_codec(native):
    with pytest.raises((ValueError, RuntimeError)):
        native.block_compress(GZIP, b"abc", 4096)
    with pytest.raises((ValueError, RuntimeError)):
        native.plan_block_streams(GZIP, gzip.compress(b"abc" * 100))


def test_gzip_mof_tables():
    from uda_amd.utils.mof import CODEC_CLASSES, CODECS, encode_partitions
    assert CODECS["gzip"] == 5
    assert CODEC_CLASSES["gzip"] == GZIP_CLASS
    parts = [b"first partition " * 50, b"", b"third"]
    for checksum in (False, True):
        data, index = encode_partitions(parts, "gzip", checksum=checksum)
        assert [r for _, r, _ in index] == [len(p) for p in parts]
        for (start, raw, plen), p in zip(index, parts):
            body = data[start:start + plen]
            assert body[:10] == b"\x1f\x8b\x08\x00\x00\x00\x00\x00" + body[8:10]  # bare header, mtime 0
            if checksum:
                assert body[-4:] == struct.pack(">I", zlib.crc32(body[:-4]))
                body = body[:-4]
            assert gzip.decompress(body) == p
        assert sum(plen for _, _, plen in index) == len(data)


def two_member_partitions(parts, checksum):
    """(file bytes, index) with every partition written as two gzip members."""
    data, index = bytearray(), []
    for p in parts:
        cut = len(p) // 3
        body = gzip.compress(p[:cut], mtime=0) + gzip.compress(p[cut:], mtime=0)
        if checksum:
            body += struct.pack(">I", zlib.crc32(body))
        index.append((len(data), len(p), len(body)))
        data += body
    return bytes(data), index


def sorted_records(maps, partition):
    return sorted((kv for m in maps for kv in m[partition]), key=datagen.sort_key(datagen.TEXT))


def same_records(recs, want):
    kf = datagen.sort_key(datagen.TEXT)
    assert [kf(kv) for kv in recs] == [kf(kv) for kv in want]
    assert collections.Counter(recs) == collections.Counter(want)


@pytest.mark.parametrize("checksum", [False, True], ids=["no-trailers", "trailers"])
@pytest.mark.parametrize("where", ["memory", "file"])
def test_gzip_loopback_reduce_cpu_backend(tmp_path, where, checksum):
    from uda_amd.bridge import UdaProvider, run_reduce
    from uda_amd.utils.mof import encode_partitions, write_mof
    p = UdaProvider()
    try:
        job = "job_1_05%d%d" % (where == "file", checksum)
        maps = datagen.wordcount(num_maps=6, reducers=2, words_per_map=4000, seed=9)
        ids = []
        for i, parts in enumerate(datagen.streams(maps)):
            mid = f"attempt_{job}_m_{i:06d}_0"
            if where == "file":
                path, _ = write_mof(str(tmp_path), mid, parts, codec="gzip", checksum=checksum)
                p.add_mof_file(job, mid, path)
            else:
                p.add_mof_memory(job, mid, *encode_partitions(parts, "gzip", checksum=checksum))
            ids.append(mid)
        for max_buf_kb in (16, 1024):
            recs, st, c = run_reduce("h", job, ids, 0, datagen.TEXT, codec="gzip", max_buf_kb=max_buf_kb, kv_buf_size=8192)
            same_records(recs, sorted_records(maps, 0))
            assert c.failure is None and st["finished"]
            assert st["ifile_checksum"] == ("verified" if checksum else "none"), st
    finally:
        p.close()


@pytest.mark.parametrize("checksum", [False, True], ids=["no-trailers", "trailers"])
def test_gzip_two_member_partitions_cpu_backend(checksum):
    from uda_amd.bridge import UdaProvider, run_reduce
    p = UdaProvider()
    try:
        job = "job_1_056%d" % checksum
        maps = datagen.wordcount(num_maps=5, reducers=1, words_per_map=3000, seed=21)
        ids = []
        for i, parts in enumerate(datagen.streams(maps)):
            mid = f"attempt_{job}_m_{i:06d}_0"
            p.add_mof_memory(job, mid, *two_member_partitions(parts, checksum))
            ids.append(mid)
        recs, st, c = run_reduce("h", job, ids, 0, datagen.TEXT, codec="gzip", max_buf_kb=16, kv_buf_size=8192)
        same_records(recs, sorted_records(maps, 0))
        assert c.failure is None and st["finished"]
        assert st["ifile_checksum"] == ("verified" if checksum else "none"), st
    finally:
        p.close()


def test_gzip_corrupt_partition_fails_the_cpu_task_once(tmp_path):
    from uda_amd.bridge import UdaConsumer, UdaFallback, UdaProvider
    from uda_amd.utils.mof import write_mof
    p = UdaProvider()
    try:
        job = "job_1_0570"
        maps = datagen.wordcount(num_maps=3, reducers=1, words_per_map=3000, seed=4)
        ids = []
        for i, parts in enumerate(datagen.streams(maps)):
            mid = f"attempt_{job}_m_{i:06d}_0"
            path, index = write_mof(str(tmp_path), mid, parts, codec="gzip")
            if i == 1:
                with open(path, "r+b") as f:
                    f.seek(index[0][2] // 2)
                    b = f.read(1)
                    f.seek(index[0][2] // 2)
                    f.write(bytes([b[0] ^ 0x10]))
            p.add_mof_file(job, mid, path)
            ids.append(mid)
        c = UdaConsumer(len(ids), job, f"attempt_{job}_r_000000_0", datagen.TEXT, codec="gzip", max_buf_kb=16,
                        conf={"mapred.uda.ifile.checksum": "off"})
        for m in ids:
            c.fetch("h", job, m, 0)
        with pytest.raises(UdaFallback, match="gzip|decodes to") as e:
            c.wait(60)
        c.close()
        assert c.failure_calls == 1
        assert ids[1] in str(e.value), str(e.value)
    finally:
        p.close()


def test_init_still_refuses_bzip2():
    from uda_amd.bridge import UdaConsumer
    with pytest.raises(Exception, match="unsupported compression codec"):
        c = UdaConsumer(1, "job_1_0580", "attempt_job_1_0580_r_000000_0", datagen.TEXT,
                        codec="org.apache.hadoop.io.compress.BZip2Codec")
        c.close()


def test_gzip_native_selftest_under_sanitizers(tmp_path, geometry, valid, matrix):
    """tests/native/gzip_selftest.cc, a program of its own, built with csrc/codec/inflate.cc under ASan + UBSan,
    over the valid, matrix, multi-member, invalid and truncated cases dumped here. Exit status 0 = no report,
    no disagreement. Nothing is loaded into Python under a sanitizer."""
    import shutil
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    cases = tmp_path / "cases"
    cases.mkdir()
    lines = []

    def dump(kind, name, stream, want=None):
        name = name.replace("@", "_at_")
        (cases / (name + ".in")).write_bytes(stream)
        if want is not None:
            (cases / (name + ".out")).write_bytes(want)
        lines.append(kind + " " + name)

    for name, stream, want in valid:
        dump("V", name, stream, want)
    first_bodies = {c[0].split("@")[0] for c in matrix[:4 * (len(matrix) // 12)]}
    for name, stream, want, _ in matrix:  # (a third of the matrix's bodies, under every header: the program is slow)
        if name.split("@")[0] in first_bodies:
            dump("V", "m_" + name, stream, want)
    for name, stream, want, _ in multi_member_cases(geometry["window"], geometry["literal_stage"]):
        dump("M", name, stream, want)
    for name, stream in INVALID:
        dump("I", name, stream)
    (cases / "manifest").write_text("\n".join(lines) + "\n")
    exe = str(tmp_path / "gzip_selftest")
    subprocess.run([cxx, "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I" + os.path.join(root, "csrc", "include"), os.path.join(root, "tests", "native", "gzip_selftest.cc"),
                    os.path.join(root, "csrc", "codec", "inflate.cc"), "-o", exe], check=True)
    r = subprocess.run([exe, str(cases)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    assert " 0 failures" in r.stdout
