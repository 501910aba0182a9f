"""Hand-built zstd (RFC 8878) frames for the codec tests: pure Python, no project code.

A frame / block header assembler, a pure-Python XXH64, the FSE table construction for the three predefined
distributions (enough to lay one sequence per block to the bit: with Predefined mode and a single sequence the
bitstream is three initial states and the extra bits), an expander that says what such frames decode to, and
named cases:

VALID     (name, stream, raw): every Frame_Header_Descriptor layout, Raw / RLE blocks of 0, 1 and 128 KiB bytes,
          empty frames, compressed blocks with Raw or RLE literals and zero or one sequence, skippable frames
          before, between and after frames, two frames.
SHAPES    (name, stream, raw): one-sequence blocks at the shapes a wave-parallel decoder can get wrong (literal
          runs of 0, 1, 63, 64, 65; offset 1 with a long match; an offset equal to the bytes produced; a repeat
          offset taken with literal length 0; a match ending on the last byte; a match reaching into the
          previous block).
BEYOND_WINDOW / STRICTER: the places where libzstd's one-shot call and the format differ (see _window_cases).
INVALID   (name, stream, cap): streams a decoder must refuse; test_zstd_cases_cpu.py holds each against libzstd.

The judge of all of them is libzstd where it loads (tests/test_zstd_cases_cpu.py).
"""
from __future__ import annotations

import struct

MAGIC = b"\x28\xb5\x2f\xfd"
BLOCK_MAX = 128 * 1024
M64 = (1 << 64) - 1

# ---------------------------------------------------------------- XXH64
_P1, _P2, _P3, _P4, _P5 = (0x9E3779B185EBCA87, 0xC2B2AE3D27D4EB4F, 0x165667B19E3779F9, 0x85EBCA77C2B2AE63,
                           0x27D4EB2F165667C5)


def _rotl(v, r):
    return ((v << r) | (v >> (64 - r))) & M64


def _round(acc, inp):
    return (_rotl((acc + inp * _P2) & M64, 31) * _P1) & M64


def _merge(h, v):
    return (((h ^ _round(0, v)) * _P1) + _P4) & M64


def xxh64(data: bytes, seed: int = 0) -> int:
    n = len(data)
    at = 0
    if n >= 32:
        v = [(seed + _P1 + _P2) & M64, (seed + _P2) & M64, seed, (seed - _P1) & M64]
        while at + 32 <= n:
            for j, w in enumerate(struct.unpack_from("<4Q", data, at)):
                v[j] = _round(v[j], w)
            at += 32
        h = (_rotl(v[0], 1) + _rotl(v[1], 7) + _rotl(v[2], 12) + _rotl(v[3], 18)) & M64
        for x in v:
            h = _merge(h, x)
    else:
        h = (seed + _P5) & M64
    h = (h + n) & M64
    while at + 8 <= n:
        h = (_rotl(h ^ _round(0, struct.unpack_from("<Q", data, at)[0]), 27) * _P1 + _P4) & M64
        at += 8
    if at + 4 <= n:
        h = (_rotl(h ^ (struct.unpack_from("<I", data, at)[0] * _P1) & M64, 23) * _P2 + _P3) & M64
        at += 4
    while at < n:
        h = (_rotl(h ^ (data[at] * _P5) & M64, 11) * _P1) & M64
        at += 1
    h ^= h >> 33
    h = (h * _P2) & M64
    h ^= h >> 29
    h = (h * _P3) & M64
    h ^= h >> 32
    return h


# ---------------------------------------------------------------- headers
def frame_header(*, fcs=None, fcs_flag=0, single=False, window=(7, 0), checksum=False, dict_id=None, dict_flag=0,
                 reserved=False) -> bytes:
    """Magic and Frame_Header. fcs_flag 0..3 picks the FCS field size (0: one byte if single else none);
    window = (exponent, mantissa) of the Window_Descriptor (absent when single); dict_flag 0..3 -> 0/1/2/4 bytes."""
    d = (fcs_flag << 6) | (0x20 if single else 0) | (0x08 if reserved else 0) | (0x04 if checksum else 0) | dict_flag
    out = bytearray(MAGIC)
    out.append(d)
    if not single:
        out.append((window[0] << 3) | window[1])
    out += (dict_id or 0).to_bytes((0, 1, 2, 4)[dict_flag], "little")
    n = (1 if single else 0) if fcs_flag == 0 else 1 << fcs_flag
    if n:
        v = fcs - 256 if n == 2 else fcs
        out += v.to_bytes(n, "little")
    return bytes(out)


def block_header(btype: int, size: int, last: bool) -> bytes:
    return ((size << 3) | (btype << 1) | (1 if last else 0)).to_bytes(3, "little")


def raw_block(data: bytes, last=False) -> bytes:
    return block_header(0, len(data), last) + data


def rle_block(byte: int, n: int, last=False) -> bytes:
    return block_header(1, n, last) + bytes([byte])


def compressed_block(payload: bytes, last=False) -> bytes:
    return block_header(2, len(payload), last) + payload


def literals_raw(data: bytes, size_format=None) -> bytes:
    return _lit_header(0, len(data), size_format) + data


def literals_rle(byte: int, n: int, size_format=None) -> bytes:
    return _lit_header(1, n, size_format) + bytes([byte])


def _lit_header(kind, n, size_format):
    if size_format is None:
        size_format = 0 if n < 32 else 1 if n < 4096 else 3
    if size_format in (0, 2):
        assert n < 32
        return bytes([(n << 3) | (size_format << 2) | kind])
    if size_format == 1:
        assert n < 4096
        return ((n << 4) | (1 << 2) | kind).to_bytes(2, "little")
    return ((n << 4) | (3 << 2) | kind).to_bytes(3, "little")


def skippable(payload: bytes, nibble: int = 0) -> bytes:
    return struct.pack("<II", 0x184D2A50 | nibble, len(payload)) + payload


def frame(blocks, raw: bytes = b"", **hdr) -> bytes:
    """A frame of already-built blocks; with checksum=True the low 32 bits of XXH64(raw) follow."""
    out = frame_header(**hdr) + b"".join(blocks)
    if hdr.get("checksum"):
        out += struct.pack("<I", xxh64(raw) & 0xFFFFFFFF)
    return out


# ---------------------------------------------------------------- predefined FSE tables, one sequence per block
LL_NORM = [4, 3, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 1, 1, 1, 2, 2, 2, 2, 2, 2, 2, 2, 2, 3, 2, 1, 1, 1, 1, 1, -1, -1, -1, -1]
ML_NORM = [1, 4, 3, 2, 2, 2, 2, 2, 2] + [1] * 37 + [-1] * 7
OF_NORM = [1, 1, 1, 1, 1, 1, 2, 2, 2] + [1] * 15 + [-1] * 5
LL_BASE = list(range(16)) + [16, 18, 20, 22, 24, 28, 32, 40, 48, 64, 128, 256, 512, 1024, 2048, 4096, 8192, 16384,
                             32768, 65536]
LL_BITS = [0] * 16 + [1, 1, 1, 1, 2, 2, 3, 3, 4, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16]
ML_BASE = list(range(3, 35)) + [35, 37, 39, 41, 43, 47, 51, 59, 67, 83, 99, 131, 259, 515, 1027, 2051, 4099, 8195,
                                16387, 32771, 65539]
ML_BITS = [0] * 32 + [1, 1, 1, 1, 2, 2, 3, 3, 4, 4, 5, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16]


def fse_table(norm, alog):
    """[(symbol, nbits, baseline)] of the decoding table (RFC 8878, 4.1.1)."""
    size = 1 << alog
    sym = [0] * size
    high = size - 1
    nxt = []
    for s, p in enumerate(norm):
        if p == -1:
            sym[high] = s
            high -= 1
            nxt.append(1)
        else:
            nxt.append(p)
    pos = 0
    step = (size >> 1) + (size >> 3) + 3
    for s, p in enumerate(norm):
        for _ in range(max(p, 0)):
            sym[pos] = s
            pos = (pos + step) & (size - 1)
            while pos > high:
                pos = (pos + step) & (size - 1)
    assert pos == 0
    table = []
    for u in range(size):
        s = sym[u]
        n = nxt[s]
        nxt[s] += 1
        nbits = alog - (n.bit_length() - 1)
        table.append((s, nbits, (n << nbits) - size))
    return table


_LL_T, _OF_T, _ML_T = fse_table(LL_NORM, 6), fse_table(OF_NORM, 5), fse_table(ML_NORM, 6)


def _code(bases, v):
    c = 0
    while c + 1 < len(bases) and bases[c + 1] <= v:
        c += 1
    return c


def _state(table, code):
    return next(u for u, e in enumerate(table) if e[0] == code)


class _Bits:
    def __init__(self):
        self.acc = 0
        self.n = 0

    def put(self, v, nb):
        assert 0 <= v < (1 << nb) or nb == 0
        self.acc |= v << self.n
        self.n += nb

    def done(self) -> bytes:
        self.put(1, 1)
        return self.acc.to_bytes((self.n + 7) // 8, "little")


def one_sequence(ll: int, ml: int, ov: int) -> bytes:
    """Sequences section of one sequence in Predefined mode: literal length, match length, Offset_Value."""
    lc, mc, oc = _code(LL_BASE, ll), _code(ML_BASE, ml), ov.bit_length() - 1
    w = _Bits()  # written in the reverse of the order the decoder reads
    w.put(ll - LL_BASE[lc], LL_BITS[lc])
    w.put(ml - ML_BASE[mc], ML_BITS[mc])
    w.put(ov - (1 << oc), oc)
    w.put(_state(_ML_T, mc), 6)
    w.put(_state(_OF_T, oc), 5)
    w.put(_state(_LL_T, lc), 6)
    return b"\x01\x00" + w.done()


def seq_block(literals: bytes, ll: int, ml: int, ov: int, last=False, rle_literals=False) -> bytes:
    """A compressed block: Raw (or RLE: literals is then one byte repeated) literals and one sequence taking `ll`
    of them; the rest follow the match."""
    lit = literals_rle(literals[0], len(literals)) if rle_literals else literals_raw(literals)
    return compressed_block(lit + one_sequence(ll, ml, ov), last)


def expand(steps) -> bytes:
    """What a frame decodes to. steps: ('raw', bytes) | ('rle', byte, n) | ('seq', literals, ll, ml, ov)."""
    out = bytearray()
    rep = [1, 4, 8]
    for st in steps:
        if st[0] == "raw":
            out += st[1]
        elif st[0] == "rle":
            out += bytes([st[1]]) * st[2]
        else:
            _, lits, ll, ml, ov = st
            out += lits[:ll]
            if ov > 3:
                off = ov - 3
                rep = [off, rep[0], rep[1]]
            else:
                idx = ov + (1 if ll == 0 else 0)
                if idx == 1:
                    off = rep[0]
                elif idx == 2:
                    off = rep[1]
                    rep = [off, rep[0], rep[2]]
                elif idx == 3:
                    off = rep[2]
                    rep = [off, rep[0], rep[1]]
                else:
                    off = rep[0] - 1
                    rep = [off, rep[0], rep[1]]
            assert 0 < off <= len(out)
            for _ in range(ml):
                out.append(out[-off])
            out += lits[ll:]
    return bytes(out)


def seq_frame(steps, **hdr):
    """(stream, raw) of a frame laid from expand()'s steps, one block a step."""
    raw = expand(steps)
    blocks = []
    for i, st in enumerate(steps):
        last = i + 1 == len(steps)
        if st[0] == "raw":
            blocks.append(raw_block(st[1], last))
        elif st[0] == "rle":
            blocks.append(rle_block(st[1], st[2], last))
        else:
            blocks.append(seq_block(st[1], st[2], st[3], st[4], last))
    hdr.setdefault("window", (7, 0))
    return frame(blocks, raw, **hdr), raw


def structure(stream: bytes):
    """Offsets of the structural boundaries of a single frame: after the magic, after the header, after every
    block header and every block, and (with a checksum) where it starts. For truncation cases."""
    cuts = [4]
    d = stream[4]
    single = bool(d & 0x20)
    at = 5 + (0 if single else 1) + (0, 1, 2, 4)[d & 3]
    fcsf = d >> 6
    at += (1 if single else 0) if fcsf == 0 else 1 << fcsf
    cuts.append(at)
    while True:
        bh = int.from_bytes(stream[at:at + 3], "little")
        at += 3
        cuts.append(at)
        at += 1 if (bh >> 1) & 3 == 1 else bh >> 3
        cuts.append(at)
        if bh & 1:
            break
    if d & 4:
        cuts.append(at + 4)
    return cuts


# ---------------------------------------------------------------- cases
def _pattern(n: int, mul: int = 37) -> bytes:
    return bytes((i * mul + (i >> 8)) & 0xFF for i in range(n))


def _valid():
    cases = []
    small = _pattern(300)
    # every Frame_Header_Descriptor layout
    cases.append(("fcs0-window", frame([raw_block(small, True)], window=(0, 0)), small))
    cases.append(("fcs1-single", frame([raw_block(small[:200], True)], single=True, fcs=200), small[:200]))
    for flag, name in ((1, "fcs2"), (2, "fcs4"), (3, "fcs8")):
        cases.append((name + "-single", frame([raw_block(small, True)], single=True, fcs_flag=flag, fcs=300), small))
        cases.append((name + "-window", frame([raw_block(small, True)], fcs_flag=flag, fcs=300, window=(0, 3)), small))
    cases.append(("window-min", frame([raw_block(small, True)], window=(0, 0)), small))
    cases.append(("window-huge", frame([raw_block(small, True)], window=(21, 7)), small))  # windowLog 31
    cases.append(("dict-id-zero", frame([raw_block(small, True)], dict_flag=1, dict_id=0), small))
    cases.append(("checksum", frame([raw_block(small, True)], small, checksum=True), small))
    cases.append(("checksum-fcs", frame([raw_block(small, True)], small, checksum=True, single=True, fcs_flag=1, fcs=300), small))
    # blocks of 0, 1 and 128 KiB bytes
    big = _pattern(BLOCK_MAX, 101)
    for n, data in ((0, b""), (1, b"x"), (BLOCK_MAX, big)):
        cases.append((f"raw-{n}", frame([raw_block(data, True)]), data))
        cases.append((f"rle-{n}", frame([rle_block(0x5A, n, True)]), b"\x5a" * n))
    cases.append(("empty-single", frame([raw_block(b"", True)], single=True, fcs=0), b""))
    cases.append(("empty-blocks", frame([raw_block(b""), rle_block(1, 0), raw_block(b"", True)]), b""))
    cases.append(("raw-rle-raw", frame([raw_block(small), rle_block(7, 1000), raw_block(small[:5], True)]),
                  small + b"\x07" * 1000 + small[:5]))
    # compressed blocks with no sequences
    for n in (0, 1, 31, 32, 4095, 4096, 70000):
        data = _pattern(n, 11)
        if n:  # (libzstd refuses a compressed block of under three bytes, which Raw literals of none would be)
            cases.append((f"lit-raw-{n}", frame([compressed_block(literals_raw(data) + b"\x00", True)]), data))
        cases.append((f"lit-rle-{n}", frame([compressed_block(literals_rle(0x41, n) + b"\x00", True)]), b"A" * n))
    cases.append(("lit-raw-format2", frame([compressed_block(literals_raw(b"abc", 2) + b"\x00", True)]), b"abc"))
    # skippable frames and two frames
    f1, f2 = frame([raw_block(small, True)]), frame([rle_block(9, 77, True)], single=True, fcs=77)
    r2 = b"\x09" * 77
    cases.append(("skip-before", skippable(b"hello") + f1, small))
    cases.append(("skip-between", f1 + skippable(b"", 15) + f2, small + r2))
    cases.append(("skip-after", f1 + skippable(b"x" * 100, 3), small))
    cases.append(("two-frames", f1 + f2, small + r2))
    return cases


def _shapes():
    cases = []
    base = _pattern(400, 13)
    for ll in (0, 1, 63, 64, 65):
        # a first block gives the match something to reach; then ll literals and a match
        steps = [("raw", base[:100]), ("seq", base[100:100 + ll + 7], ll, 9, 50 + 3)]
        cases.append((f"literal-run-{ll}",) + seq_frame(steps))
    cases.append(("offset1-long",) + seq_frame([("seq", b"Q" + base[:3], 1, 200, 1 + 3)]))
    cases.append(("offset1-short",) + seq_frame([("seq", b"Q", 1, 64, 1 + 3)]))
    cases.append(("offset-overlap-3",) + seq_frame([("seq", b"abc", 3, 100, 3 + 3)]))
    cases.append(("offset-eq-produced",) + seq_frame([("seq", base[:70], 70, 70, 70 + 3)]))
    cases.append(("match-ends-output",) + seq_frame([("raw", base[:10]), ("seq", base[10:12], 2, 12, 12 + 3)]))
    cases.append(("rep-with-ll0",) + seq_frame([("seq", base[:8], 8, 4, 8 + 3), ("seq", base[8:12], 4, 5, 6 + 3),
                                                ("seq", b"", 0, 6, 1)]))  # ll 0, value 1: the second recent offset
    cases.append(("rep-ll0-value3",) + seq_frame([("seq", base[:20], 20, 4, 9 + 3), ("seq", b"", 0, 5, 3)]))  # rep[0] - 1
    cases.append(("rep-value1",) + seq_frame([("seq", base[:20], 20, 4, 9 + 3), ("seq", base[20:23], 3, 5, 1)]))
    cases.append(("rep-initial",) + seq_frame([("raw", base[:10]), ("seq", base[10:11], 1, 3, 2)]))  # initial rep[1] = 4
    cases.append(("match-crosses-block",) + seq_frame([("raw", base[:300]), ("seq", base[300:301], 1, 250, 280 + 3)]))
    cases.append(("long-literals-long-match",) + seq_frame([("seq", base[:333], 300, 1000, 299 + 3)]))
    cases.append(("rle-block-then-match",) + seq_frame([("rle", 0x33, 500), ("seq", b"xy", 2, 70, 400 + 3)]))
    lits = b"\x77" * 90
    raw = lits[:80] + b"\x77" * 30 + lits[80:]
    cases.append(("rle-literals-seq", frame([seq_block(lits, 80, 30, 5 + 3, True, rle_literals=True)]), raw))
    return cases


def _invalid():
    small = _pattern(100)
    good = frame([raw_block(small, True)])
    cases = []
    cases.append(("wrong-magic", b"\x28\xb5\x2f\xfc" + good[4:], 100))
    cases.append(("reserved-descriptor-bit", frame([raw_block(small, True)], reserved=True), 100))
    cases.append(("reserved-block-type", frame([block_header(3, 100, True) + small]), 100))
    cases.append(("dictionary-id", frame([raw_block(small, True)], dict_flag=1, dict_id=7), 100))
    cases.append(("dictionary-id-4", frame([raw_block(small, True)], dict_flag=3, dict_id=0x12345678), 100))
    cases.append(("oversize-compressed-block", frame([block_header(2, BLOCK_MAX + 1, True) + b"\x00" * (BLOCK_MAX + 1)]),
                  BLOCK_MAX + 1))
    cases.append(("fcs-mismatch", frame([raw_block(small, True)], single=True, fcs=99), 100))
    cases.append(("fcs-mismatch-more", frame([raw_block(small, True)], single=True, fcs_flag=1, fcs=300), 300))
    bad_sum = bytearray(frame([raw_block(small, True)], small, checksum=True))
    bad_sum[-1] ^= 0x80
    cases.append(("checksum-mismatch", bytes(bad_sum), 100))
    cases.append(("offset-before-start", frame([seq_block(b"ab", 2, 5, 3 + 3, True)]), 100))
    cases.append(("offset-before-start-block2", frame([raw_block(b"0123456789"), seq_block(b"ab", 2, 5, 13 + 3, True)]), 100))
    treeless = (((1 | (1 << 10)) << 4) | 3).to_bytes(3, "little")  # Treeless, one stream, 1 byte regenerated from 1
    cases.append(("treeless-first-block", frame([compressed_block(treeless + b"\x01\x00", True)]), 100))
    # Huffman literals, direct weights 3 and 1: 4 + 1 = 5 leaves 3 to the last symbol, no power of two
    huf = bytes([129, 0x31, 0x01])
    v = (4 | (len(huf) << 10)) << 4 | 2
    cases.append(("weights-incomplete", frame([compressed_block(v.to_bytes(3, "little") + huf + b"\x00", True)]), 100))
    # an offsets table description of accuracy log 5 that never stops naming zero-probability symbols
    w = _Bits()
    w.put(0, 4)
    w.put(1, 5)
    for _ in range(14):
        w.put(3, 2)
    desc = w.acc.to_bytes(5, "little") + b"\xff\xff"
    cases.append(("fse-description-overshoots",
                  frame([compressed_block(literals_raw(b"abcd") + b"\x01\x20" + desc + b"\x01", True)]), 100))
    cases.append(("sequence-needs-more-literals", frame([seq_block(b"ab", 3, 5, 1 + 3, True)]), 100))
    cases.append(("bytes-behind-no-sequences", frame([compressed_block(literals_raw(b"abc") + b"\x00\x00", True)]), 100))
    for cut in sorted(set(structure(good))):
        if cut < len(good):
            cases.append((f"truncated-at-{cut}", good[:cut], 100))
    cases.append(("truncated-mid-block", good[:50], 100))
    cases.append(("truncated-magic", good[:3], 100))
    return cases


def _window_cases():
    """Where the format and libzstd 1.4.8's one-shot ZSTD_decompress part ways, pinned by tests.
    BEYOND_WINDOW (name, stream, raw): an offset larger than Window_Size but inside the frame's output. libzstd
    takes it, and so does the one-shot decoder here.
    STRICTER (name, stream, cap): what the format forbids and the decoders here refuse, but libzstd's one-shot call
    takes: a Raw or RLE block larger than Window_Size (it checks that for compressed blocks only), a compressed
    block that regenerates more than Block_Maximum_Size, a sequence bitstream with bits left over, and one that
    runs out inside its last sequence."""
    base = _pattern(2048, 29)
    steps = [("raw", base[:1024]), ("raw", base[1024:]), ("seq", b"zz", 2, 40, 2000 + 3)]
    beyond = [("offset-beyond-window",) + seq_frame(steps, window=(0, 0))]
    stricter = [("rle-block-past-window", frame([rle_block(1, 1025, True)], window=(0, 0)), 2000),
                ("raw-block-past-window", frame([raw_block(base[:1025], True)], window=(0, 0)), 2000)]
    # a compressed block that regenerates more than Block_Maximum_Size (here the window's 1 KiB)
    stricter.append(("block-regenerates-past-its-limit", frame([seq_block(b"ab", 2, 2000, 1 + 3, True)], window=(0, 0)), 4000))
    # a sequence bitstream with eight bits nobody reads below its first field, and one whose last field runs out
    # eight bits early (libzstd reads zeros there)
    sec = one_sequence(2, 5, 2 + 3)
    stricter.append(("bitstream-left-over", frame([compressed_block(literals_raw(b"ab") + sec[:2] + b"\x00" + sec[2:], True)]), 100))
    sec = one_sequence(2, 2000, 1 + 3)
    stricter.append(("bitstream-runs-out", frame([compressed_block(literals_raw(b"ab") + sec[:2] + sec[3:], True)]), 4000))
    return beyond, stricter


VALID = _valid()
BEYOND_WINDOW, STRICTER = _window_cases()
SHAPES = _shapes()
INVALID = _invalid()
