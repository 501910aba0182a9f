"""Shared by the streamed block-decode tests: block-compressed FIXED10 partitions on odd block geometry.

Records come from fixed10_cases (sorted runs, the EOF marker ff ff appended per stream); every stream is
cut into blocks whose raw sizes cycle through a pattern, each block compressed by the host codec and framed
by decode_cases.frame. Options: zero-length blocks at given block positions (never a stream's last block:
with a trailer-aware walk a trailer-less stream's final 00 00 00 00 reads as a checksum), Snappy blocks
split into several chunks with a first chunk below the 128-byte prefix slot, and a CRC32 trailer per stream.

A case's round size gives 4..8 key-range rounds. The pure-Python pieces here (walk, first_keys, run_keys)
are the oracles the CPU and GPU tests compare the native code with."""
import collections
import functools
import struct
import zlib

from tests import decode_cases as dc
from tests import fixed10_cases as fc

L = fc.L
EOF = fc.EOF
CODEC_ID = dc.CODEC_ID
PREFIX_SLOT = 128

PATTERNS = ((1,), (12,), (13,), (14,), (103,), (104,), (105,), (116,), (117,), (208,), (5000,),
            (3, 500, 11, 104), (104, 1, 104, 13))
MID = (105,)  # every first-record offset 0..103 occurs; at 93..103 the key straddles the block end
SHAPES = ("all_equal", "heavy_key", "hi_tie", "extremes", "ragged", "uniform")
ROTATION = ("lzo", "snappy", "lz4")

Case = collections.namedtuple("Case", "name codec shape K n pattern zeros split trailer")


def _cases():
    out = []
    for shape in SHAPES:
        for codec in ROTATION:
            out.append(Case(f"{shape}-{codec}-mid", codec, shape, 6, 800, MID, (), False, False))
    for i, pat in enumerate(PATTERNS):
        codec = ROTATION[i % 3]
        shape = ("heavy_key", "hi_tie")[i % 2]
        n = 60 if min(pat) < 52 else 800
        zeros = (0, 1, 2, 7) if i % 4 in (1, 2) else ()
        split = codec == "snappy" and max(pat) >= 116
        out.append(Case(f"{shape}-{codec}-{'_'.join(map(str, pat))}", codec, shape, 6, n, pat, zeros, split,
                        i % 2 == 0))
    return tuple(out)


CASES = _cases()
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)


def compressor(native, codec):
    return {"snappy": native.snappy_compress, "lzo": native.lzo1x_compress, "lz4": native.lz4_compress}[codec]


def cut(part, pattern):
    """The raw blocks of a partition: sizes cycle through `pattern`, the last block takes what is left."""
    out, i, j = [], 0, 0
    while i < len(part):
        n = pattern[j % len(pattern)]
        out.append(part[i:i + n])
        i += n
        j += 1
    return out


def _chunks(comp, raw, split):
    """(chunk, raw) pairs of one block. split: a first chunk of under 128 raw bytes, then up to three more."""
    if not split or len(raw) < 2:
        return [(comp(raw), raw)]
    a = min(50, len(raw) // 2)
    pieces, rest = [raw[:a]], raw[a:]
    step = -(-len(rest) // 3)
    pieces += [rest[i:i + step] for i in range(0, len(rest), step)]
    return [(comp(p), p) for p in pieces]


def compress_stream(native, codec, part, pattern, zeros=(), split=False, trailer=False):
    """(stream, raw sizes of its non-empty blocks)."""
    comp = compressor(native, codec)
    raws = cut(part, pattern)
    blocks = [_chunks(comp, r, split) for r in raws]
    for z in sorted(zeros):
        if z < len(blocks):  # never behind the last block
            blocks.insert(z, [])
    stream, braws = dc.frame(blocks)
    assert braws == raws
    if trailer:
        stream += struct.pack(">I", zlib.crc32(stream))
    return stream, [len(r) for r in raws]


Built = collections.namedtuple("Built", "case runs parts streams blocks round_bytes Q N")


def _round_bytes(total):
    rb = max(L, -(-total // 6))
    return rb, max(1, -(-total // rb))


_BUILT = {}


def build(native, case):
    """The case's runs (records only), partitions (with EOF), compressed streams, per-stream block sizes."""
    if case.name not in _BUILT:
        runs = fc.case(case.shape)[0] if case.shape == "ragged" else fc.case(case.shape, case.K, case.n)[0]
        parts = tuple(r + EOF for r in runs)
        streams, blocks = [], []
        for p in parts:
            s, b = compress_stream(native, case.codec, p, case.pattern, case.zeros, case.split, case.trailer)
            streams.append(s)
            blocks.append(b)
        total = sum(len(r) for r in runs)
        rb, Q = _round_bytes(total)
        _BUILT[case.name] = Built(case, runs, parts, tuple(streams), tuple(blocks), rb, Q, total // L)
    return _BUILT[case.name]


@functools.lru_cache(maxsize=None)
def expected(shape, K, n):
    runs = fc.case(shape)[0] if shape == "ragged" else fc.case(shape, K, n)[0]
    return fc.oracle(runs) + EOF


def run_keys(run):
    return [run[i + 3:i + 13] for i in range(0, len(run), L)]


def first_keys(parts, blocks):
    """Per block of all streams: the 10 bytes where the key of the first record starting in the block would
    lie (None where the partition ends before them). Which of them are keys is for the plan to know."""
    out = []
    for part, sizes in zip(parts, blocks):
        rel = 0
        for raw in sizes:
            at = rel + (-rel) % L + 3
            out.append(part[at:at + 10] if at + 10 <= len(part) else None)
            rel += raw
    return out


def first_offsets(parts, blocks):
    """The oracle of `first`: the offset in the block of the first whole record that starts in it, -1 when
    there is none or its 13 bytes of head and key do not fit in the block."""
    out = []
    for part, sizes in zip(parts, blocks):
        nrec, rel = (len(part) - 2) // L, 0
        for raw in sizes:
            r = -(-rel // L)  # the first record that starts at or behind the block's first byte
            start = r * L - rel
            out.append(start if r < nrec and start < raw and start + 13 <= raw else -1)
            rel += raw
    return out


def plan_of(native, built, round_bytes=None):
    return native.block_round_plan([len(r) // L for r in built.runs], [list(b) for b in built.blocks],
                                   first_keys(built.parts, built.blocks), round_bytes or built.round_bytes)


def planned_blocks(plan, nrec):
    """Blocks the rounds of a plan decode (boundary blocks count once per round that holds them)."""
    return sum(sp["b1"] - sp["b0"] + 1 for row in plan["spans"] for k, sp in enumerate(row)
               if nrec[k] > 0 and sp["b1"] >= sp["b0"])


def _varint(buf):
    v = 0
    for k in range(5):
        if k >= len(buf):
            return None
        v |= (buf[k] & 0x7F) << (7 * k)
        if not buf[k] & 0x80:
            return v if v < 1 << 32 else None
    return None


def walk(codec, streams, tails):
    """The documented framing (block_decoder.h) walked in Python over several streams: ([(stream, src,
    src_end, dst, raw)], raw_offset, tails) as the native plans report it, or None when not resolvable."""
    descs, raw_offset, tl, dst = [], [0], [], 0
    for k, s in enumerate(streams):
        i, n, tail = 0, len(s), 0
        while i < n:
            if tails and n - i == 4:
                tail = 4
                break
            if i + 4 > n:
                return None
            raw = int.from_bytes(s[i:i + 4], "big")
            i += 4
            if raw == 0:
                continue
            src, left = i, raw
            while left > 0:
                if i + 4 > n:
                    return None
                clen = int.from_bytes(s[i:i + 4], "big")
                if i + 4 + clen > n:
                    return None
                produced = left
                if codec == "snappy":
                    produced = _varint(s[i + 4:i + 4 + clen])
                    if produced is None or produced == 0 or produced > left:
                        return None
                i += 4 + clen
                left -= produced
            descs.append((k, src, i, dst, raw))
            dst += raw
        raw_offset.append(dst)
        tl.append(tail)
    return descs, raw_offset, (tl if tails else [])
