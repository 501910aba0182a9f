"""zlib map outputs (Hadoop's DefaultCodec / DeflateCodec) on the host: the in-tree inflater against streams
that Python's zlib module wrote at every level and strategy, trailer detection behind a stream, codec
selection, the MOF writer and a reduce task on the CPU backend; and the inflater's stand-alone sanitizer
program over the hand-assembled cases of tests/inflate_cases.py.
"""
import collections
import os
import random
import struct
import zlib

import pytest

from tests.inflate_cases import invalid_cases, valid_cases
from uda_amd.utils import datagen

ZLIB = 4
LEVELS = (0, 1, 6, 9)
STRATEGIES = {"default": zlib.Z_DEFAULT_STRATEGY, "fixed": zlib.Z_FIXED, "huffman_only": zlib.Z_HUFFMAN_ONLY,
              "rle": zlib.Z_RLE}


def _payloads():
    """The payload set of tests/test_lz4_codec.py, and a TeraSort partition; seeded, so that a failure on the
    host or on the device can be replayed on the same bytes."""
    rng = random.Random(11)
    yield "random", rng.randbytes(300_000)
    yield "period1", b"\x00" * 100_000
    yield "period3", b"abc" * 50_000 + b"x"
    yield "mixed", b"".join(
        (rng.randbytes(rng.randint(1, 300)) if rng.random() < 0.5 else bytes([rng.randrange(256)]) * rng.randint(1, 900))
        for _ in range(600))
    base = rng.randbytes(5000)  # slices of one text: long non-overlapping back-references at odd alignments
    yield "slices", b"".join(base[o:o + n] for o, n in ((rng.randrange(4700), rng.randint(4, 300)) for _ in range(2000)))
    yield "ifile", datagen.streams(datagen.secondary_sort(3, 1, 3000, seed=2))[0][0]
    yield "terasort", datagen.streams(datagen.terasort(2, 1, 2800, seed=5))[0][0]
    yield "tiny", b"q"
    yield "empty", b""


PAYLOADS = {k: v[:300_000] for k, v in _payloads()}  # (the device tests take streams of at most 300 KB raw)


def deflate(data, level, strategy):
    c = zlib.compressobj(level, zlib.DEFLATED, 15, 9, strategy)
    return c.compress(data) + c.flush()


def roundtrip_streams():
    """[(name, stream, raw)] for every payload x level x strategy; shared with tests/test_gpu_inflate.py."""
    out = []
    for pname, raw in PAYLOADS.items():
        for level in LEVELS:
            for sname, strategy in STRATEGIES.items():
                out.append(("%s-l%d-%s" % (pname, level, sname), deflate(raw, level, strategy), raw))
    return out


@pytest.mark.parametrize("name", list(PAYLOADS))
def test_zlib_roundtrip_levels_and_strategies(native, name):
    raw = PAYLOADS[name]
    for level in LEVELS:
        for sname, strategy in STRATEGIES.items():
            st = deflate(raw, level, strategy)
            out, used = native.zlib_decompress(st, len(raw))
            assert out == raw and used == len(st), (level, sname)
    st = zlib.compress(raw)  # what encode_partitions writes
    for feed in (1, 4096) if len(raw) < 120_000 else (4096,):
        assert native.block_decompress(ZLIB, st, feed) == raw


def test_zlib_trailer_detection(native):
    """Behind a stream, no byte or the four of an IFile checksum are accepted; one to three are malformed.
    The stream's own last four bytes (its Adler-32) are not taken for a trailer."""
    for name in ("ifile", "tiny", "empty", "period3"):
        raw = PAYLOADS[name]
        st = zlib.compress(raw)
        assert native.host_decode_partition(ZLIB, st) == (raw, 0), name
        crc = struct.pack(">I", zlib.crc32(st))
        assert native.host_decode_partition(ZLIB, st + crc) == (raw, 4), name
        assert native.host_decode_partition(ZLIB, st + b"\x00\x00\x00\x00") == (raw, 4), name
        for k in (1, 2, 3, 5, 8):
            with pytest.raises((ValueError, RuntimeError)):
                native.host_decode_partition(ZLIB, st + b"\x01" * k)
        for cut in (1, 4, 5):
            with pytest.raises((ValueError, RuntimeError)):
                native.host_decode_partition(ZLIB, st[:-cut])


def test_zlib_codec_class(native):
    assert native.codec_from_class("org.apache.hadoop.io.compress.DefaultCodec") == 4
    assert native.codec_from_class("org.apache.hadoop.io.compress.DeflateCodec") == 4
    for other in ("GzipCodec", "BZip2Codec", "ZStandardCodec"):
        assert native.codec_from_class("org.apache.hadoop.io.compress." + other) == -1
    assert native.codec_from_class("org.apache.hadoop.io.compress.SnappyCodec") == 1
    assert native.codec_from_class("com.hadoop.compression.lzo.LzoCodec") == 2
    assert native.codec_from_class("org.apache.hadoop.io.compress.Lz4Codec") == 3
    assert native.codec_from_class("") == 0


def test_zlib_is_no_block_codec(native):
    """The block entry points keep refusing it: it has no framing to compress into or to walk."""
    with pytest.raises((ValueError, RuntimeError)):
        native.block_compress(ZLIB, b"abc", 4096)
    with pytest.raises((ValueError, RuntimeError)):
        native.plan_block_streams(ZLIB, zlib.compress(b"abc" * 100))


def test_zlib_mof_tables():
    from uda_amd.utils.mof import CODEC_CLASSES, CODECS, encode_partitions
    assert CODECS["zlib"] == 4
    assert CODEC_CLASSES["zlib"] == "org.apache.hadoop.io.compress.DefaultCodec"
    parts = [b"first partition " * 50, b"", b"third"]
    for checksum in (False, True):
        data, index = encode_partitions(parts, "zlib", checksum=checksum)
        assert [r for _, r, _ in index] == [len(p) for p in parts]
        for (start, raw, plen), p in zip(index, parts):
            body = data[start:start + plen]
            d = zlib.decompressobj()  # one stream, no framing
            assert d.decompress(body) == p and d.eof
            if checksum:
                assert d.unused_data == struct.pack(">I", zlib.crc32(body[:-4]))
            else:
                assert d.unused_data == b""
        assert sum(plen for _, _, plen in index) == len(data)


@pytest.mark.parametrize("checksum", [False, True])
def test_zlib_loopback_reduce_cpu_backend(tmp_path, checksum):
    """A reduce task on the CPU backend over zlib MOF files: the Inflater behind BlockDecoder in the fetch
    path, fed in 16 KiB fetches, with and without IFile checksum trailers."""
    from uda_amd.bridge import UdaProvider, run_reduce
    from uda_amd.utils.mof import write_mof
    p = UdaProvider()
    try:
        job = "job_1_04%02d" % (30 + checksum)
        maps = datagen.wordcount(num_maps=6, reducers=2, words_per_map=4000, seed=9)
        ids = []
        for i, parts in enumerate(datagen.streams(maps)):
            mid = f"attempt_{job}_m_{i:06d}_0"
            path, _ = write_mof(str(tmp_path), mid, parts, codec="zlib", checksum=checksum)
            p.add_mof_file(job, mid, path)
            ids.append(mid)
        recs, st, c = run_reduce("h", job, ids, 0, datagen.TEXT, codec="zlib", max_buf_kb=16)
        want = sorted((kv for m in maps for kv in m[0]), key=datagen.sort_key(datagen.TEXT))
        kf = datagen.sort_key(datagen.TEXT)
        assert [kf(kv) for kv in recs] == [kf(kv) for kv in want]
        assert collections.Counter(recs) == collections.Counter(want)
        assert c.failure is None and st["finished"]
        assert st["ifile_checksum"] == ("verified" if checksum else "none"), st
    finally:
        p.close()


def test_zlib_corrupt_partition_fails_the_cpu_task_once(tmp_path):
    from uda_amd.bridge import UdaConsumer, UdaFallback, UdaProvider
    from uda_amd.utils.mof import write_mof
    p = UdaProvider()
    try:
        job = "job_1_0439"
        maps = datagen.wordcount(num_maps=3, reducers=1, words_per_map=3000, seed=4)
        ids = []
        for i, parts in enumerate(datagen.streams(maps)):
            mid = f"attempt_{job}_m_{i:06d}_0"
            path, index = write_mof(str(tmp_path), mid, parts, codec="zlib")
            if i == 1:
                with open(path, "r+b") as f:
                    f.seek(index[0][2] // 2)
                    b = f.read(1)
                    f.seek(index[0][2] // 2)
                    f.write(bytes([b[0] ^ 0x10]))
            p.add_mof_file(job, mid, path)
            ids.append(mid)
        c = UdaConsumer(len(ids), job, f"attempt_{job}_r_000000_0", datagen.TEXT, codec="zlib", max_buf_kb=16,
                        conf={"mapred.uda.ifile.checksum": "off"})
        for m in ids:
            c.fetch("h", job, m, 0)
        with pytest.raises(UdaFallback, match="zlib|decodes to"):
            c.wait(60)
        c.close()
        assert c.failure_calls == 1
    finally:
        p.close()


def test_inflate_native_selftest_under_sanitizers(tmp_path, native):
    """tests/native/inflate_selftest.cc, a program of its own, built with csrc/codec/inflate.cc (and with it
    csrc/codec/inflate_tables.h, the table code the device kernel runs) under ASan + UBSan, over every case
    of tests/inflate_cases.py dumped here. Exit status 0 = no report, no disagreement."""
    import shutil
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    g = native.gpu_inflate_geometry()
    cases = tmp_path / "cases"
    cases.mkdir()
    lines = []
    for name, stream, want in valid_cases(g["window"], g["literal_stage"]):
        (cases / (name + ".in")).write_bytes(stream)
        (cases / (name + ".out")).write_bytes(want)
        lines.append("V " + name)
    for name, stream in invalid_cases():
        (cases / (name + ".in")).write_bytes(stream)
        lines.append("I " + name)
    (cases / "manifest").write_text("\n".join(lines) + "\n")
    exe = str(tmp_path / "inflate_selftest")
    subprocess.run([cxx, "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I" + os.path.join(root, "csrc", "include"), os.path.join(root, "tests", "native", "inflate_selftest.cc"),
                    os.path.join(root, "csrc", "codec", "inflate.cc"), "-o", exe], check=True)
    r = subprocess.run([exe, str(cases)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert " 0 failures" in r.stdout
