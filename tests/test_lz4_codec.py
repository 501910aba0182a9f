"""In-tree LZ4 block-format codec (Hadoop's Lz4Codec) on the host: the raw codec, the Hadoop block
framing, codec selection and a reduce task on the CPU backend.

No LZ4 library is importable here, so the decoder is checked against hand-assembled streams
(tests/lz4_vectors.py) and the encoder's output is decoded by the pure-Python decoder of that file,
which also yields the sequences the end-of-block rules are checked on.
"""
import collections
import os
import random
import struct

import pytest

from tests.lz4_vectors import VECTORS, hadoop_block, lz4_block_decode, lz4_walk
from uda_amd.utils import datagen

LZ4 = 3


def _payloads():
    rng = random.Random(11)
    yield "random", os.urandom(300_000)
    yield "period1", b"\x00" * 100_000
    yield "period3", b"abc" * 50_000 + b"x"
    yield "mixed", b"".join(
        (os.urandom(rng.randint(1, 300)) if rng.random() < 0.5 else bytes([rng.randrange(256)]) * rng.randint(1, 900))
        for _ in range(600))
    base = os.urandom(5000)  # slices of one text: long non-overlapping back-references at odd alignments
    yield "slices", b"".join(base[o:o + n] for o, n in ((rng.randrange(4700), rng.randint(4, 300)) for _ in range(2000)))
    yield "ifile", datagen.streams(datagen.secondary_sort(3, 1, 3000, seed=2))[0][0]
    yield "tiny", b"q"
    yield "empty", b""


PAYLOADS = dict(_payloads())


@pytest.mark.parametrize("name", [v[0] for v in VECTORS])
def test_lz4_spec_vectors(native, name):
    """Hand-assembled streams decode to the output the format defines: raw decoder (exact-size output),
    Hadoop block framing, and the pure-Python decoder that checks the encoder below."""
    stream, want = {v[0]: (v[1], v[2]) for v in VECTORS}[name]
    assert native.lz4_decompress(stream, len(want)) == want
    if want:  # a zero-length block has no chunk in the framing
        assert native.block_decompress(LZ4, hadoop_block(want, stream), 7) == want
    assert lz4_block_decode(stream) == want


@pytest.mark.parametrize("name", list(PAYLOADS))
def test_lz4_roundtrip_and_independent_decode(native, name):
    d = PAYLOADS[name]
    c = native.lz4_compress(d)
    assert native.lz4_decompress(c, len(d)) == d
    assert lz4_block_decode(c) == d


def _check_end_rules(d, c):
    out, seqs = lz4_walk(c)
    assert out == d
    n = len(d)
    for lit, start, off, mlen in seqs[:-1]:
        assert mlen >= 4 and 1 <= off <= 65535
        assert start + 12 <= n, "a match starts in the last 12 bytes"
        assert start + mlen <= n - 5, "a match covers one of the last 5 bytes"
    assert seqs[-1][2:] == (0, 0)
    if seqs[:-1]:
        assert seqs[-1][0] >= 5


@pytest.mark.parametrize("name", list(PAYLOADS))
def test_lz4_encoder_end_of_block_rules(native, name):
    d = PAYLOADS[name]
    _check_end_rules(d, native.lz4_compress(d))


def test_lz4_encoder_short_inputs_and_tails(native):
    assert native.lz4_compress(b"") == b"\x00"
    assert native.lz4_compress(b"q") == b"\x10q"
    d12 = b"a" * 12
    assert native.lz4_compress(d12) == b"\xc0" + d12  # shorter than 13 bytes: all literals
    # 13 bytes is the shortest input that may hold a match, and every length around the end-of-block
    # limits on data that matches everywhere
    for n in list(range(0, 80)) + [13]:
        for d in (b"a" * n, (b"abcdefg" * 12)[:n]):
            c = native.lz4_compress(d)
            _check_end_rules(d, c)
            assert native.lz4_decompress(c, n) == d
    assert len(native.lz4_compress(b"a" * 64)) < 16  # and matches are found at all


def test_lz4_truncated_streams_rejected(native):
    """Every proper prefix of a valid stream is rejected outright, or decodes to fewer bytes than the
    block announces, which the framing layer refuses."""
    rng = random.Random(3)
    d = b"".join(bytes([rng.randrange(4)]) * rng.randint(1, 30) + os.urandom(rng.randint(0, 6)) for _ in range(60))
    c = native.lz4_compress(d)
    assert len(c) < len(d)
    for k in range(len(c)):
        try:
            got = native.lz4_decompress(c[:k], len(d))
        except ValueError:
            got = None
        assert got is None or len(got) < len(d), k
        with pytest.raises((ValueError, RuntimeError)):
            native.block_decompress(LZ4, hadoop_block(d, c[:k]), 1 << 16)
    for name, stream, want in VECTORS:
        for k in range(min(len(stream), 300)):
            try:
                got = native.lz4_decompress(stream[:k], len(want))
            except ValueError:
                got = None
            assert got is None or len(got) < len(want), (name, k)


@pytest.mark.parametrize("name,stream,cap,bad_format", [
    ("offset_0", b"\x10a" + b"\x00\x00" + b"\x00", 64, True),
    ("offset_past_the_start", b"\x30abc" + b"\x04\x00" + b"\x00", 64, True),
    ("offset_past_the_start_65535", b"\x30abc" + b"\xff\xff" + b"\x00", 64, True),
    ("literal_extension_to_the_end", b"\xf0" + b"\xff" * 40, 1 << 20, True),
    ("match_extension_to_the_end", b"\x1fa" + b"\x01\x00" + b"\xff" * 40, 1 << 20, True),
    ("literal_run_past_cap", b"\x80abcdefgh", 7, False),
    ("match_past_cap", b"\x16a" + b"\x01\x00" + b"\x00", 10, False),
    ("ends_after_a_match", b"\x16a" + b"\x01\x00", 64, True),
    ("ends_inside_the_offset", b"\x16a" + b"\x01", 64, True),
    ("ends_inside_the_literals", b"\x50abc", 64, True),
    ("no_input", b"", 64, True),
])
def test_lz4_corrupt_streams_rejected(native, name, stream, cap, bad_format):
    with pytest.raises(ValueError):
        native.lz4_decompress(stream, cap)
    if bad_format:  # the oracle agrees that the format forbids it
        with pytest.raises(ValueError):
            lz4_block_decode(stream)
    else:  # valid for the format, one byte too long for cap
        assert len(lz4_block_decode(stream)) == cap + 1
    with pytest.raises((ValueError, RuntimeError)):
        native.block_decompress(LZ4, hadoop_block(b"x" * cap, stream), 1 << 16)


@pytest.mark.parametrize("block", [4096, 262144])
@pytest.mark.parametrize("feed", [1, 65536])
def test_lz4_block_framing_roundtrip(native, block, feed):
    d = PAYLOADS["ifile"][:150_000] + PAYLOADS["mixed"][:60_000] if feed == 1 else \
        b"".join(PAYLOADS[k] for k in ("ifile", "mixed", "slices", "random"))
    framed = native.block_compress(LZ4, d, block)
    assert struct.unpack(">I", framed[:4])[0] == min(block, len(d))
    assert native.block_decompress(LZ4, framed, feed) == d


def test_lz4_three_chunk_block_decodes_on_the_host(native):
    """A block whose compressed output was split into three chunks: a chunk carries no length, the decoder
    reports what each produced; offsets reach back to the chunk's own start at most."""
    parts = [os.urandom(5000), b"z" * 7000, b"hello world " * 300]
    chunks = [native.lz4_compress(p) for p in parts]
    raw = b"".join(parts)
    block = struct.pack(">I", len(raw)) + b"".join(struct.pack(">I", len(c)) + c for c in chunks)
    stream = struct.pack(">I", 0) + block + struct.pack(">I", 0) + block
    for feed in (5, 1 << 20):
        assert native.block_decompress(LZ4, stream, feed) == raw + raw
    # a second chunk that reaches into the first chunk's output is corrupt
    bad = struct.pack(">I", 16) + struct.pack(">I", 9) + b"\x80abcdefgh" + struct.pack(">I", 4) + b"\x04\x08\x00\x00"
    with pytest.raises((ValueError, RuntimeError)):
        native.block_decompress(LZ4, bad, 1 << 16)


def test_lz4_codec_class(native):
    assert native.codec_from_class("org.apache.hadoop.io.compress.Lz4Codec") == 3
    assert native.codec_from_class("org.apache.hadoop.io.compress.GzipCodec") == -1
    assert native.codec_from_class("org.apache.hadoop.io.compress.SnappyCodec") == 1
    assert native.codec_from_class("com.hadoop.compression.lzo.LzoCodec") == 2


def test_lz4_mof_tables():
    from uda_amd.utils.mof import CODEC_CLASSES, CODECS
    assert CODECS["lz4"] == 3
    assert CODEC_CLASSES["lz4"] == "org.apache.hadoop.io.compress.Lz4Codec"


def test_lz4_loopback_reduce_cpu_backend(tmp_path):
    """A reduce task on the CPU backend over LZ4-compressed MOF files (BlockDecoder in the fetch path)."""
    from uda_amd.bridge import UdaProvider, run_reduce
    from uda_amd.utils.mof import write_mof
    p = UdaProvider()
    try:
        maps = datagen.wordcount(num_maps=6, reducers=2, words_per_map=4000, seed=9)
        ids = []
        for i, parts in enumerate(datagen.streams(maps)):
            mid = f"attempt_job_1_0404_m_{i:06d}_0"
            path, _ = write_mof(str(tmp_path), mid, parts, codec="lz4", block_size=8192)
            p.add_mof_file("job_1_0404", mid, path)
            ids.append(mid)
        recs, st, c = run_reduce("h", "job_1_0404", ids, 0, datagen.TEXT, codec="lz4", max_buf_kb=16)
        want = sorted((kv for m in maps for kv in m[0]), key=datagen.sort_key(datagen.TEXT))
        kf = datagen.sort_key(datagen.TEXT)
        assert [kf(kv) for kv in recs] == [kf(kv) for kv in want]
        assert collections.Counter(recs) == collections.Counter(want)
        assert c.failure is None and st["finished"]
    finally:
        p.close()


def test_lz4_native_selftest_under_sanitizers(tmp_path):
    """tests/native/lz4_selftest.cc, a program of its own, built with csrc/codec/lz4.cc under ASan + UBSan:
    vectors, round trips and thousands of mutated and truncated streams on exact-size heap buffers,
    compared with a slow reference decoder. Exit status 0 = no report, no disagreement."""
    import shutil
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "lz4_selftest")
    subprocess.run([cxx, "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I" + os.path.join(root, "csrc", "include"), os.path.join(root, "tests", "native", "lz4_selftest.cc"),
                    os.path.join(root, "csrc", "codec", "lz4.cc"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert " 0 failures" in r.stdout
