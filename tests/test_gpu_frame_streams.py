"""GPU: the device framing walk (frame_streams_kernel, plan_block_streams_device) against the host walk
plan_block_streams, field by field, on the streams of stream_cases and on truncated and malformed ones.

The streams of a call lie back to back in one device buffer without alignment, so a lane that read past
its stream's end would read its neighbour's bytes and change its answer; the binding checks the guard
bytes behind the last stream after every call."""
import struct
import zlib

import pytest

from tests import stream_cases as sc

pytestmark = pytest.mark.gpu
CODECS = sc.ROTATION
IDS = [c.name for c in sc.CASES]


def both(native, codec, streams, tails):
    """The device plan, asserted equal to the host plan; None when both say not resolvable."""
    host = native.plan_block_streams_descs(sc.CODEC_ID[codec], streams, tails)
    dev = native.gpu_plan_block_streams_device(sc.CODEC_ID[codec], streams, tails, 0)
    assert (host is None) == (dev is None), (codec, tails, [len(s) for s in streams], host, dev)
    if host is None:
        return None
    assert len(host[0]) == len(dev[0])
    for i, (h, d) in enumerate(zip(host[0], dev[0])):
        assert tuple(h) == tuple(d), (i, h, d)
    assert list(host[1]) == list(dev[1]) and list(host[2]) == list(dev[2])
    return dev


def small_stream(native, codec, records=3, pattern=(50,), trailer=False, zeros=(), split=False, seed=0):
    part = bytes((seed + i * 7) % 251 for i in range(records * sc.L)) + sc.EOF
    return sc.compress_stream(native, codec, part, pattern, zeros, split, trailer)[0]


@pytest.mark.parametrize("name", IDS)
def test_case_streams(require_gpu, native, name):
    b = sc.build(native, sc.BY_NAME[name])
    c = b.case
    for tails in (False, True):
        dev = both(native, c.codec, list(b.streams), tails)
        if c.trailer and not tails:
            continue  # a trailer is no block framing: the walks only have to agree on what its bytes are
        assert dev is not None
        want = sc.walk(c.codec, b.streams, tails)
        assert [tuple(d) for d in dev[0]] == want[0] and list(dev[1]) == want[1] and list(dev[2]) == want[2]


@pytest.mark.parametrize("codec", CODECS)
def test_trailered_streams_without_the_trailer_aware_walk(require_gpu, native, codec):
    """Four more bytes than the blocks: a block header without its chunk, unless the CRC's bytes happen to
    frame something. Both walks must say the same."""
    streams = [small_stream(native, codec, trailer=True, seed=s) for s in range(5)]
    both(native, codec, streams, False)
    assert both(native, codec, streams, True)[2] == [4] * 5


@pytest.mark.parametrize("codec", CODECS)
@pytest.mark.parametrize("count", [1, 63, 64, 65, 130])
def test_stream_counts_around_a_workgroup(require_gpu, native, codec, count):
    streams = [small_stream(native, codec, records=1 + s % 3, pattern=(13 + s % 5, 104), trailer=s % 2 == 1,
                            zeros=(s % 4,) if s % 3 == 0 else (), split=codec == "snappy" and s % 2 == 0, seed=s)
               for s in range(count)]
    dev = both(native, codec, streams, True)
    assert dev is not None and list(dev[2]) == [4 * (s % 2) for s in range(count)]
    assert [tuple(d) for d in dev[0]] == sc.walk(codec, streams, True)[0]


@pytest.mark.parametrize("codec", CODECS)
def test_empty_and_trailer_only_streams(require_gpu, native, codec):
    a = small_stream(native, codec, seed=1)
    crc0 = struct.pack(">I", zlib.crc32(b""))
    crc = struct.pack(">I", 0x89ABCDEF)
    for streams in ([b""], [b"", b""], [a, b"", a], [b"", a, b""], [crc0], [crc], [a, crc, a], [a, crc0, b"", a]):
        dev = both(native, codec, streams, True)
        assert dev is not None and list(dev[2]) == [4 if len(s) == 4 else 0 for s in streams]
        assert [tuple(d) for d in dev[0]] == sc.walk(codec, streams, True)[0]
        both(native, codec, streams, False)  # four bytes alone: a block header without its chunks
    # a zero-length block is a stream's last four bytes: a trailer to the trailer-aware walk, a block otherwise
    z = a + bytes(4)
    assert list(both(native, codec, [a, z, a], True)[2]) == [0, 4, 0]
    assert both(native, codec, [a, z, a], False) is not None
    assert both(native, codec, [bytes(4)], False) is not None and both(native, codec, [bytes(8)], True)[2] == [4]


@pytest.mark.parametrize("codec", CODECS)
def test_truncated_streams_between_intact_neighbours(require_gpu, native, codec):
    """One stream cut at every length up to the end of its second block's first chunk: every cut inside the
    first two block headers, the first chunk headers and Snappy's length varint is among them."""
    a = small_stream(native, codec, seed=3)
    victim = small_stream(native, codec, records=2, pattern=(13,), split=codec == "snappy", seed=5)
    descs = sc.walk(codec, [victim], False)[0]
    upto = descs[1][2] + 1
    assert upto < 120
    verdicts = set()
    for tails in (False, True):
        for n in range(upto + 1):
            got = both(native, codec, [a, victim[:n], a], tails)
            verdicts.add(got is not None)
            if got is not None:  # the neighbours' plans do not depend on the cut
                assert [d[1:3] for d in got[0] if d[0] == 0] == [d[1:3] for d in got[0] if d[0] == 2]
    assert verdicts == {True, False}


def _snappy_block(raw, chunks):
    return struct.pack(">I", raw) + b"".join(struct.pack(">I", len(c)) + c for c in chunks)


def test_snappy_chunk_lengths(require_gpu, native):
    """Chunks the walk judges by their length varint alone (it decodes nothing): empty and one-byte chunks,
    a five-byte varint, a varint that never ends, a length above what the block still lacks."""
    a = small_stream(native, "snappy", seed=7)
    body = bytes(range(40, 60))
    variants = {
        "clen0": (_snappy_block(13, [b""]), False),
        "clen0-then-more": (_snappy_block(13, [b"", b"\x0d" + body]), False),
        "clen1-zero": (_snappy_block(13, [b"\x00"]), False),
        "clen1-all": (_snappy_block(13, [b"\x0d"]), True),
        "clen1-part": (_snappy_block(13, [b"\x05", b"\x08" + body]), True),
        "varint5": (_snappy_block(13, [b"\x8d\x80\x80\x80\x00" + body]), True),
        "varint5-only": (_snappy_block(13, [b"\x8d\x80\x80\x80\x00"]), True),
        "varint5-high": (_snappy_block(13, [b"\x8d\x80\x80\x80\x10" + body]), False),
        "varint-unending": (_snappy_block(13, [b"\x8d\x80\x80\x80\x80\x00" + body]), False),
        "varint-cut-by-clen": (_snappy_block(13, [b"\x8d\x80"]), False),
        "above-left": (_snappy_block(13, [b"\x0e" + body]), False),
        "above-left-2nd": (_snappy_block(13, [b"\x0a" + body, b"\x04" + body]), False),
        "exact-2nd": (_snappy_block(13, [b"\x0a" + body, b"\x03" + body]), True),
        "zero-2nd": (_snappy_block(13, [b"\x0a" + body, b"\x00"]), False),
    }
    for name, (stream, ok) in variants.items():
        for tails in (False, True):
            for s in (stream, stream + _snappy_block(0, []) + stream):
                got = both(native, "snappy", [a, s, a], tails)
                assert (got is not None) == ok, (name, tails)
                assert (sc.walk("snappy", [a, s, a], tails) is not None) == ok, name
