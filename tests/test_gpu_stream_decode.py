"""GPU: device_reduce_fixed_blocks as a whole (device framing walk, prefix decode, block first keys, the
round plan, per-round block decode and cut, merge, delivery) on the block geometries of stream_cases.

The delivered bytes must equal the Python stable sort of the runs (key, then run, then position) to the
byte: the streamed path promises the order of equal keys that device_reduce_fixed keeps. The number of
decoded blocks is checked against block_round_plan fed with first keys read from the raw partitions in
Python, so the device's prefix decode and first-key kernel are compared with an independent source."""
import struct

import pytest

from tests import decode_cases as dc
from tests import fixed10_cases as fc
from tests import stream_cases as sc

pytestmark = pytest.mark.gpu
L = sc.L
EOF = sc.EOF
KV = 8192
PIECE = 32 << 10
IDS = [c.name for c in sc.CASES]
V1_CASE = "heavy_key-snappy-5000"


def reduce_blocks(native, codec, streams, round_bytes, pack, trailers=False):
    return native.gpu_device_reduce_fixed_blocks(sc.CODEC_ID[codec], list(streams), KV, round_bytes, PIECE, pack, 0,
                                                 trailers)


@pytest.mark.parametrize("name", IDS)
def test_streamed_reduce(require_gpu, native, name):
    b = sc.build(native, sc.BY_NAME[name])
    c = b.case
    assert 4 <= b.Q <= 8
    nrec = [len(r) // L for r in b.runs]
    want = sc.expected(c.shape, c.K, c.n)
    blocks = sc.planned_blocks(sc.plan_of(native, b), nrec)
    over = native.hbm_stats(0)["over"]
    guard = native.device_guard_violations()
    for pack in ("auto", "off") + (("v1",) if name == V1_CASE else ()):
        bufs, st = reduce_blocks(native, c.codec, b.streams, b.round_bytes, pack, c.trailer)
        assert st["streamed"] is True, pack
        joined = b"".join(bufs)
        assert len(joined) == len(want), (pack, len(joined), len(want))
        if joined != want:
            i = next(i for i in range(0, len(want), L) if joined[i:i + L] != want[i:i + L])
            raise AssertionError(f"{name} {pack}: first difference in record {i // L}: "
                                 f"{joined[i:i + 20].hex()} for {want[i:i + 20].hex()}")
        assert all(0 < len(x) <= KV for x in bufs)
        assert all(len(x) % L == 0 for x in bufs[:-1]) and len(bufs[-1]) % L == 2 and bufs[-1].endswith(EOF)
        assert st["rounds"] == b.Q and st["records"] == b.N and st["bytes"] == b.N * L, (pack, st)
        assert st["buffers"] == len(bufs) and st["pieces"] == st["packed_pieces"] + st["raw_pieces"], (pack, st)
        assert st["decoded_blocks"] == blocks, (pack, st, blocks)
        if pack == "off":
            assert st["d2h_bytes"] == b.N * L and st["packed_pieces"] == 0, st
    assert native.hbm_stats(0)["over"] == over
    assert native.device_guard_violations() == guard


def _plain(native, codec, parts, block=5000):
    return [sc.compress_stream(native, codec, p, (block,))[0] for p in parts]


@pytest.mark.parametrize("codec", sc.ROTATION)
def test_not_terasort_shaped_falls_back(require_gpu, native, codec):
    """The record that starts block 2 of one stream has another head; the stream decodes all the same."""
    b = sc.build(native, sc.BY_NAME[f"uniform-{codec}-mid"])
    parts = list(b.parts)
    at = -(-10000 // L) * L  # the first record start in the third block of 5000 bytes
    p = bytearray(parts[2])
    assert p[at:at + 3] == b"\x0b\x5b\x0a"
    p[at + 2] = 0x0B
    parts[2] = bytes(p)
    streams = _plain(native, codec, parts)
    assert dc.stream_decode(codec, streams[2])[0] == parts[2]
    bufs, st = reduce_blocks(native, codec, streams, b.round_bytes, "auto")
    assert st["streamed"] is False and bufs == [] and st["buffers"] == 0 and st["records"] == 0


@pytest.mark.parametrize("codec", sc.ROTATION)
def test_descending_block_keys_fall_back(require_gpu, native, codec):
    b = sc.build(native, sc.BY_NAME[f"uniform-{codec}-mid"])
    parts = list(b.parts)
    parts[1] = b"".join(reversed(fc.records(b.runs[1]))) + EOF
    bufs, st = reduce_blocks(native, codec, _plain(native, codec, parts), b.round_bytes, "auto")
    assert st["streamed"] is False and bufs == [] and st["buffers"] == 0 and st["records"] == 0


@pytest.mark.parametrize("codec", sc.ROTATION)
def test_all_runs_empty(require_gpu, native, codec):
    streams = _plain(native, codec, [EOF] * 3) + [sc.compress_stream(native, codec, EOF, (1,))[0]]
    bufs, st = reduce_blocks(native, codec, streams, 4096, "auto")
    assert st["streamed"] is True and bufs == [EOF] and st["buffers"] == 1 and st["records"] == 0


@pytest.mark.parametrize("codec", sc.ROTATION)
def test_damaged_chunk_in_a_later_round_is_an_error(require_gpu, native, codec):
    """A chunk that lost its last byte, in a block no earlier round decodes and behind the 128 bytes the prefix
    pass reads: the round that decodes it must raise, and the call must return."""
    b = sc.build(native, sc.BY_NAME[f"uniform-{codec}-mid"])
    streams = _plain(native, codec, b.parts)
    sizes = [[len(x) for x in sc.cut(p, (5000,))] for p in b.parts]
    plan = native.block_round_plan([len(r) // L for r in b.runs], sizes, sc.first_keys(b.parts, sizes), b.round_bytes)
    k = len(streams) - 1
    blk0 = sum(len(s) for s in sizes[:k])
    target = blk0 + len(sizes[k]) - 2  # a whole block of 5000 bytes near the end of the last stream
    rounds = [q for q, row in enumerate(plan["spans"]) if row[k]["b0"] <= target <= row[k]["b1"]]
    assert rounds and min(rounds) >= 1
    descs = sc.walk(codec, streams, False)[0]
    stream_k = [d for d in descs if d[0] == k]
    _, src, src_end, _, raw = stream_k[target - blk0]
    assert raw == 5000
    s = streams[k]
    # the block's one chunk: [clen][chunk] at src .. src_end; drop the chunk's last byte
    clen = struct.unpack(">I", s[src:src + 4])[0]
    assert src + 4 + clen == src_end
    streams[k] = s[:src] + struct.pack(">I", clen - 1) + s[src + 4:src_end - 1] + s[src_end:]
    assert sc.walk(codec, streams, False) is not None
    with pytest.raises(ValueError):
        dc.stream_decode(codec, streams[k])
    with pytest.raises(Exception, match="corrupt compressed block"):
        reduce_blocks(native, codec, streams, b.round_bytes, "auto")
    # the device and the pooled workspaces are as usable as before
    bufs, st = reduce_blocks(native, codec, _plain(native, codec, b.parts), b.round_bytes, "auto")
    assert st["streamed"] is True and b"".join(bufs) == sc.expected("uniform", 6, 800)
