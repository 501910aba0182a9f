"""F6 device block decode of LZ4 (Hadoop's Lz4Codec) against the original bytes, the host decoder and
hand-assembled streams, and LZ4 jobs through the GPU consumer paths: per-round streaming decode (prefix
decode with a clip), whole-partition device decode, and the staged (host-fetched) path.
"""
import os
import random
import struct

import pytest

from tests.lz4_vectors import VECTORS, hadoop_block
from uda_amd.utils import datagen

pytestmark = pytest.mark.gpu

LZ4 = 3
GPU = {"mapred.uda.merge.backend": "gpu"}


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


@pytest.fixture(scope="module")
def payloads():
    out = dict(_payloads())
    out["terasort"] = datagen.streams(datagen.terasort(2, 1, 6000, seed=5))[0][0]
    return out


def expected(maps, partition, key_class):
    recs = [kv for m in maps for kv in m[partition]]
    return sorted(recs, key=datagen.sort_key(key_class))


def test_lz4_spec_vectors_on_device(require_gpu, native):
    """The device decoder on hand-assembled streams (not produced by our encoder), one block each. The
    empty vector is framed the way Hadoop frames no data: a zero-length block, which has no chunk."""
    streams = [hadoop_block(want, st) if want else struct.pack(">I", 0) for _, st, want in VECTORS]
    outs, blocks, _ = native.gpu_block_decode("lz4", streams)
    assert blocks == sum(1 for _, _, want in VECTORS if want)
    for (name, _, want), out in zip(VECTORS, outs):
        assert out == want, name
    # all vectors as the blocks of one stream: neighbours in one workgroup, outputs back to back
    outs, blocks, _ = native.gpu_block_decode("org.apache.hadoop.io.compress.Lz4Codec", [b"".join(streams)])
    assert outs == [b"".join(want for _, _, want in VECTORS)]


@pytest.mark.parametrize("block", [4096, 65536, 262144])
def test_lz4_device_decode_roundtrip(require_gpu, native, payloads, block):
    names, raws = list(payloads), list(payloads.values())
    streams = [native.block_compress(LZ4, raw, block) for raw in raws]
    outs, blocks, _ms = native.gpu_block_decode("lz4", streams)
    assert blocks == sum((len(r) + block - 1) // block for r in raws)
    for name, raw, out, st in zip(names, raws, outs, streams):
        assert out == raw, name
        assert out == native.block_decompress(LZ4, st, 1 << 20), name


def test_lz4_empty_streams_and_zero_length_blocks(require_gpu, native):
    raw = b"hello world " * 300
    block = native.block_compress(LZ4, raw, 1 << 16)
    zero = struct.pack(">I", 0)
    outs, blocks, _ = native.gpu_block_decode("lz4", [b"", zero, zero + block + zero + block, b""])
    assert outs == [b"", b"", raw + raw, b""]
    assert blocks == 2


def _corrupt_streams(native):
    raw = b"abcdefgh" * 4000 + os.urandom(1000)
    st = bytearray(native.block_compress(LZ4, raw, 65536))
    for i in range(12, min(len(st), 60)):  # a broken back-reference, as in the Snappy / LZO corrupt tests
        st[i] = 0xFF
    yield "body_overwritten", bytes(st)
    # 8 literals, a match, and the chunk ends after the first offset byte
    yield "cut_inside_an_offset", hadoop_block(b"x" * 20, b"\x80abcdefgh" + b"\x08")
    # an offset of 9 after 8 bytes of output: one byte before the block's start
    yield "offset_before_the_block", hadoop_block(b"x" * 16, b"\x84abcdefgh" + b"\x09\x00" + b"\x00")
    yield "offset_zero", hadoop_block(b"x" * 16, b"\x84abcdefgh" + b"\x00\x00" + b"\x00")
    # length extensions of 0xFF up to the chunk's end (literal and match side)
    yield "literal_extension_to_the_end", hadoop_block(b"x" * 70000, b"\xf0" + b"\xff" * 300)
    yield "match_extension_to_the_end", hadoop_block(b"x" * 70000, b"\x1fa" + b"\x01\x00" + b"\xff" * 300)
    yield "ends_after_a_match", hadoop_block(b"x" * 11, b"\x16a" + b"\x01\x00")
    yield "block_shorter_than_announced", hadoop_block(b"x" * 12, b"\x16a" + b"\x01\x00" + b"\x00")
    yield "block_longer_than_announced", hadoop_block(b"x" * 10, b"\x16a" + b"\x01\x00" + b"\x00")


@pytest.mark.parametrize("name", ["body_overwritten", "cut_inside_an_offset", "offset_before_the_block", "offset_zero",
                                  "literal_extension_to_the_end", "match_extension_to_the_end", "ends_after_a_match",
                                  "block_shorter_than_announced", "block_longer_than_announced"])
def test_lz4_corrupt_block_raises(require_gpu, native, name):
    """One launch per case that returns with the status word set: every check of the device parse is a
    bounds test ahead of the access, as in the host decoder (which refuses the same streams)."""
    st = dict(_corrupt_streams(native))[name]
    with pytest.raises((ValueError, RuntimeError)):
        native.block_decompress(LZ4, st, 1 << 20)
    with pytest.raises(Exception, match="corrupt|framing"):
        native.gpu_block_decode("lz4", [st])


def test_lz4_terasort_streaming_decode_rounds(require_gpu):
    """LZ4-compressed TeraSort partitions decoded per key-range round: the prefix decode clips every
    block's first bytes into adjacent 128-byte slots (one byte too many would corrupt the neighbour's
    first key); the stream must equal the whole-partition decode path's, record for record."""
    from uda_amd.bridge import UdaProvider, run_reduce
    from uda_amd.utils.mof import encode_partitions
    provider = UdaProvider()
    try:
        job = "job_9_0354"
        maps = datagen.terasort(num_maps=7, reducers=2, rows_per_map=4000, seed=61)
        ids = []
        for i, parts in enumerate(datagen.streams(maps)):
            mid = f"attempt_{job}_m_{i:06d}_0"
            data, index = encode_partitions(parts, "lz4", block_size=5000)  # not a multiple of 104
            provider.add_mof_device(job, mid, data, index, device=0)
            ids.append(mid)
        base = dict(GPU, **{"mapred.uda.gpu.fetch": "device", "mapred.uda.gpu.round.bytes": 96 << 10})
        for r in range(2):
            recs, st, _ = run_reduce("h", job, ids, r, datagen.TEXT, codec="lz4", conf=base, kv_buf_size=32 << 10)
            assert recs == expected(maps, r, datagen.TEXT)
            assert st["merge_path"] == "device-fixed10-stream" and st["rpq_rounds"] > 4, st
            assert st["device_descriptors"] == 7 and st["device_decoded_blocks"] > 0, st
            whole, st2, _ = run_reduce("h", job, ids, r, datagen.TEXT, codec="lz4", kv_buf_size=32 << 10,
                                       conf=dict(base, **{"mapred.uda.gpu.decode.stream": 0}))
            assert st2["merge_path"] == "device-fixed10" and whole == recs, st2
    finally:
        provider.close()


def test_lz4_wordcount_from_mof_files_decodes_on_device(require_gpu, tmp_path):
    from uda_amd.bridge import UdaProvider, run_reduce
    from uda_amd.utils.mof import write_mof
    p = UdaProvider()
    try:
        maps = datagen.wordcount(num_maps=6, reducers=2, words_per_map=5000, seed=13)
        ids = []
        for i, parts in enumerate(datagen.streams(maps)):
            mid = f"attempt_dlz4_m_{i:06d}_0"
            path, _ = write_mof(str(tmp_path), mid, parts, codec="lz4")
            p.add_mof_file("job_dlz4", mid, path)
            ids.append(mid)
        recs, st, _ = run_reduce("h", "job_dlz4", ids, 0, datagen.TEXT, codec="lz4", conf=GPU, kv_buf_size=8192)
        assert st["device_decoded_blocks"] > 0
        want = expected(maps, 0, datagen.TEXT)
        kf = datagen.sort_key(datagen.TEXT)
        assert [kf(kv) for kv in recs] == [kf(kv) for kv in want]
        assert sorted(recs) == sorted(want)
    finally:
        p.close()


def test_lz4_secondary_sort_staged_gpu_path(require_gpu, tmp_path):
    """Host-resident LZ4 MOFs through the staged GPU path: fetched compressed by the host, staged and
    decoded on the device, merged there; same records as the CPU backend."""
    from uda_amd.bridge import UdaProvider, run_reduce
    from uda_amd.utils.mof import write_mof
    p = UdaProvider()
    try:
        maps = datagen.secondary_sort(num_maps=12, reducers=2, rows_per_map=500, seed=5)
        ids = []
        for i, parts in enumerate(datagen.streams(maps)):
            mid = f"attempt_glz4_m_{i:06d}_0"
            path, _ = write_mof(str(tmp_path), mid, parts, codec="lz4", block_size=16 << 10)
            p.add_mof_file("job_glz4", mid, path)
            ids.append(mid)
        recs_gpu, st, _ = run_reduce("h", "job_glz4", ids, 1, datagen.TEXT, codec="lz4", conf=GPU, kv_buf_size=8192)
        recs_cpu, _, _ = run_reduce("h", "job_glz4", ids, 1, datagen.TEXT, codec="lz4", kv_buf_size=8192)
        assert st["backend"] == "gpu" and st["merge_path"].startswith("staged"), st
        assert st["device_descriptors"] == 0 and st["device_decoded_blocks"] > 0, st
        assert [k for k, _ in recs_gpu] == [k for k, _ in recs_cpu]
        assert sorted(recs_gpu) == sorted(recs_cpu)
        want = expected(maps, 1, datagen.TEXT)
        assert sorted(recs_gpu) == sorted(want)
    finally:
        p.close()
