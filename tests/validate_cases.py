"""Shared by the tests of the device validators and of the TeraGen kernel (test_validate_cases_cpu.py,
test_gpu_validate.py): a pure-Python oracle of what `validate_fixed_kernel`, `slice_checksum_kernel`,
`check_fixed_kernel`, `count_mismatch_kernel` (csrc/gpu/merge.hip) and `teragen_kernel` (csrc/gpu/datagen.hip)
compute, and small streams that are wrong in one known way, placed on the kernels' edges: a 64-lane wave, a
256-thread block, and record n - 1. Nothing native is imported here.

A record is 104 bytes: 0b 5b 0a, the 10 key bytes (3..12), 5a, 90 value bytes. Every expected number is an
exact integer; most are also known in closed form (the third member of an order case)."""
import functools

import numpy as np

from tests import fixed10_cases as fc

L = fc.L
KEY = fc.KEY
M64 = (1 << 64) - 1
MAX_RECORDS = 1200  # no stream of a case is longer

# ------------------------------------------------------------------ csrc/include/uda/hash.h


def mix64(x):
    x ^= x >> 33
    x = x * 0xFF51AFD7ED558CCD & M64
    x ^= x >> 33
    x = x * 0xC4CEB9FE1A85EC53 & M64
    x ^= x >> 33
    return x


def record_hash(rec):
    """Little-endian 8-byte words, the last one zero padded, seed 0x9E3779B97F4A7C15 ^ len."""
    h = 0x9E3779B97F4A7C15 ^ len(rec)
    for i in range(0, len(rec), 8):
        h = mix64(h ^ int.from_bytes(rec[i:i + 8], "little"))
    return h


def stream_checksum(stream):
    """Sum (mod 2^64) of the record hashes of whole 104-byte records."""
    assert len(stream) % L == 0
    return sum(record_hash(rec) for rec in fc.records(stream)) & M64


# ------------------------------------------------------------------ the validators


def validate(chunks):
    """(order_errors, checksum, last_key) of the concatenated chunks: adjacent pairs whose 10-byte key decreases,
    the sum of the record hashes, the last record's key (b"" when there is no record). Empty chunks are skipped."""
    errors, ck, prev = 0, 0, None
    for chunk in chunks:
        for rec in fc.records(bytes(chunk)):
            key = rec[KEY]
            if prev is not None and prev > key:
                errors += 1
            prev = key
            ck = (ck + record_hash(rec)) & M64
    return errors, ck, prev if prev is not None else b""


def layout_ok(rec):
    return rec[0] == 0x0B and rec[1] == 0x5B and rec[2] == 0x0A and rec[13] == 0x5A


def slices_ok(slices):
    return all(layout_ok(rec) for s in slices for rec in fc.records(bytes(s)))


def count_mismatch(a, b, start=0):
    assert len(a) == len(b)
    return start + sum(1 for x, y in zip(a, b) if x != y)


# ------------------------------------------------------------------ csrc/gpu/datagen.hip


def splitmix64(state):
    """(new state, draw)"""
    state = (state + 0x9E3779B97F4A7C15) & M64
    z = state
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9 & M64
    z = (z ^ (z >> 27)) * 0x94D049BB133111EB & M64
    return state, z ^ (z >> 31)


def printable8(r):
    """Eight letters 'A'..'Z' (one per byte of r) as a little-endian word."""
    w = 0
    for b in range(8):
        w |= (65 + ((r >> (8 * b)) & 0xFF) % 26) << (8 * b)
    return w


def teragen_record(i, n, key_lo, key_span, seed, unsorted=False):
    """Record i of a run of n: the draws are the key's first 8 bytes (jitter, or the whole of it), its last two
    bytes, then the 12 value words; the first value word gives only its low two bytes (word 1's top)."""
    st = seed ^ (0xD1B54A32D192ED03 * (i + 1) & M64)
    stride = key_span // n
    if unsorted:
        st, draw = splitmix64(st)
        hi = key_lo + (draw if key_span == M64 else draw % key_span)
    else:
        jitter = 0
        if stride:
            st, draw = splitmix64(st)
            jitter = draw % stride
        hi = key_lo + i * stride + jitter
    hi &= M64
    st, draw = splitmix64(st)
    lo16 = draw & 0xFFFF
    st, draw = splitmix64(st)
    v0 = printable8(draw)
    rec = bytes((0x0B, 0x5B, 0x0A)) + hi.to_bytes(8, "big") + lo16.to_bytes(2, "big") + b"\x5a"
    rec += (v0 & 0xFFFF).to_bytes(2, "little")
    for _ in range(2, 13):
        st, draw = splitmix64(st)
        rec += printable8(draw).to_bytes(8, "little")
    assert len(rec) == L
    return rec


@functools.lru_cache(maxsize=None)
def teragen_run(n, key_lo, key_span, seed, unsorted=False):
    """The run's bytes as the kernel writes them: n records and the IFile EOF marker ff ff."""
    return b"".join(teragen_record(i, n, key_lo, key_span, seed, unsorted) for i in range(n)) + fc.EOF


TOP = 1 << 64
THIRD = M64 // 3
# (nrec, key_lo, key_span, seed) per run of one launch: every run but the last is shorter than max_nrec
TERAGEN_SORTED = (
    (1, 0, M64, 0x5EED),                            # one rank's whole key space, one record
    (2, 0x1234_5678_9ABC_DEF0, 2, 1),               # span == n: stride 1, jitter always 0
    (255, TOP - (1 << 40), 1 << 40, 2),             # the top of the key space: key_lo + key_span == 2^64
    (256, THIRD, THIRD, 0xFFFF_FFFF_FFFF_FFFF),     # rank 1 of 3
    (257, TOP - 257, 257, 3),                       # span == n at the top: the last key is ff * 8
    (1000, 0, M64 // 2, 0x0123_4567_89AB_CDEF),
)
TERAGEN_UNSORTED = (
    (1, 0, M64, 7),
    (2, 5, 1, 8),                                   # span 1: every key is key_lo
    (255, 0, M64, 9),                               # span == 2^64 - 1: the draw itself
    (256, TOP - 7, 7, 10),                          # a small span at the top
    (257, THIRD, THIRD, 11),
    (1000, 1 << 63, 1000, 12),
)


# ------------------------------------------------------------------ record builders


def from_keys(keys, seed=0):
    """A stream of the given key rows in the given order (make_run sorts; this does not). All records differ."""
    keys = np.asarray(keys, np.uint8).reshape(-1, 10)
    n = len(keys)
    rng = np.random.RandomState(4000 + seed)
    a = np.frombuffer(fc.make_run(keys, seed % 600, rng), np.uint8).reshape(n, L).copy()
    a[:, KEY] = keys
    return a.tobytes()


@functools.lru_cache(maxsize=None)
def ascending(n, seed=0):
    """n records with distinct keys, strictly ascending."""
    rng = np.random.RandomState(3000 + seed)
    return fc.make_run(fc.distinct_keys(rng, n), seed % 600, rng)


def swap(stream, p):
    """Records p and p + 1 exchanged. In a strictly ascending stream this inverts pair p and no other."""
    r = fc.records(stream)
    r[p], r[p + 1] = r[p + 1], r[p]
    return b"".join(r)


def set_byte(stream, rec, pos, value):
    a = bytearray(stream)
    a[rec * L + pos] = value
    return bytes(a)


def flip_bit(stream, rec, pos, bit):
    a = bytearray(stream)
    a[rec * L + pos] ^= 1 << bit
    return bytes(a)


def cut(stream, cuts):
    """The stream's records cut at the given record numbers (repeated numbers give empty chunks)."""
    n = len(stream) // L
    edges = [0] + list(cuts) + [n]
    assert edges == sorted(edges)
    return [stream[a * L:b * L] for a, b in zip(edges[:-1], edges[1:])]


def _tied(tails, head=bytes.fromhex("5aa5c33c0ff06996")):
    """Key rows with the first 8 bytes tied and the given 16-bit tails (bytes 8..9)."""
    keys = np.tile(np.frombuffer(head + bytes(2), np.uint8), (len(tails), 1))
    t = np.asarray(tails)
    keys[:, 8] = t >> 8
    keys[:, 9] = t & 0xFF
    return keys


# ------------------------------------------------------------------ order cases

ORDER_N = (2, 64, 65, 256, 257, 1000)


def _pairs(n):
    return sorted({p for p in (0, 62, 63, 64, 254, 255, 256, n - 2) if 0 <= p <= n - 2})


@functools.lru_cache(maxsize=None)
def order_cases():
    """{name: (stream, order errors in closed form)}"""
    out = {}
    for n in ORDER_N:
        for p in _pairs(n):
            out[f"swap_n{n}_p{p}"] = (swap(ascending(n, n), p), 1)
    # first 8 bytes tied; the pair that crosses the first wave's end inverts. Tails 2i stay below 0x100 here, so
    # records 63 and 64 (007e, 0080) differ in byte 9 only; tails i << 8 | 0x55 differ in byte 8 only
    out["byte9_only"] = (swap(from_keys(_tied([2 * i for i in range(100)]), 1), 63), 1)
    out["byte8_only"] = (swap(from_keys(_tied([(i << 8) | 0x55 for i in range(100)]), 2), 63), 1)
    keys = np.tile(np.frombuffer(bytes.fromhex("00112233445566778899"), np.uint8), (200, 1))
    keys[:, 0] = np.arange(200)
    out["byte0_only"] = (swap(from_keys(keys, 3), 100), 1)
    out["all_equal"] = (from_keys(np.tile(np.frombuffer(fc.HEAVY_KEY, np.uint8), (300, 1)), 4), 0)
    out["descending"] = (b"".join(reversed(fc.records(ascending(1000, 5)))), 999)
    zero, ones = np.zeros(10, np.uint8), np.full(10, 255, np.uint8)
    out["zeros_then_ones"] = (from_keys([zero, zero, ones, ones], 6), 0)
    out["ones_then_zeros"] = (from_keys([zero, ones, zero, ones, ones, zero], 7), 2)
    out["n1"] = (ascending(1, 8), 0)
    out["ascending_1000"] = (ascending(1000, 9), 0)
    return out


# ------------------------------------------------------------------ chunking cases

CHUNK_N = 1000
CHUNK_INVERSIONS = (0, 63, 255, 300, 600, 998)  # pairs 0, 63, 255 and 998 sit on the cuts 1, 64, 256 and n - 1
CHUNK_CUTS = (1, 63, 64, 65, 255, 256, 257, CHUNK_N - 1)
# empty chunks first, between and last; one-record chunks without (record 0) and with a predecessor (256, 999)
MANY_CUTS = (0, 0, 1, 1, 64, 64, 64, 256, 257, 600, 999, 1000, 1000)


@functools.lru_cache(maxsize=None)
def chunk_stream():
    s = ascending(CHUNK_N, 20)
    for p in CHUNK_INVERSIONS:
        s = swap(s, p)
    return s


@functools.lru_cache(maxsize=None)
def tail_stream():
    """200 records tied on their first 8 key bytes; the pair (63, 64) inverts, so it differs in bytes 8..9 only."""
    return swap(from_keys(_tied([3 * i + 1 for i in range(200)]), 21), 63)


# ------------------------------------------------------------------ checksum cases

CK_N, CK_REC = 70, 37


@functools.lru_cache(maxsize=None)
def checksum_base():
    return ascending(CK_N, 30)


@functools.lru_cache(maxsize=None)
def bit_flips():
    """104 streams: one bit (pos % 8) of byte pos of record CK_REC flipped, for every byte position."""
    return tuple(flip_bit(checksum_base(), CK_REC, pos, pos % 8) for pos in range(L))


def permuted():
    r = fc.records(checksum_base())
    order = np.random.RandomState(31).permutation(len(r))
    return b"".join(r[i] for i in order)


def values_exchanged():
    """Records 3 and 50 exchange their value bytes: the same bytes in the stream, other records."""
    r = fc.records(checksum_base())
    a, b = r[3], r[50]
    r[3], r[50] = a[:14] + b[14:], b[:14] + a[14:]
    return b"".join(r)


# ------------------------------------------------------------------ layout cases

LAYOUT_N = 1000
HEADER = {0: 0x0B, 1: 0x5B, 2: 0x0A, 13: 0x5A}
LAYOUT_RECORDS = (0, LAYOUT_N - 1, 300)  # first, last, and one past the first grid stride (256 threads)


@functools.lru_cache(maxsize=None)
def layout_cases():
    """{name: (slices, good)}"""
    base = ascending(LAYOUT_N, 40)
    out = {"good": ((base,), True)}
    for rec in LAYOUT_RECORDS:
        for pos, good in HEADER.items():
            out[f"rec{rec}_byte{pos}_flip"] = ((set_byte(base, rec, pos, good ^ 0x01),), False)
            out[f"rec{rec}_byte{pos}_zero"] = ((set_byte(base, rec, pos, 0),), False)
        for pos in (3, 12, 14, 103):  # key and value bytes are no part of the layout
            out[f"rec{rec}_byte{pos}_other"] = ((set_byte(base, rec, pos, 0x00),), True)
    small = [ascending(5, 41 + i) for i in range(40)]
    out["many_good"] = (tuple(small), True)
    out["only_last_slice_bad"] = (tuple(small[:-1]) + (set_byte(small[-1], 4, 13, 0x5B),), False)
    out["with_empty_slices"] = ((b"", small[0], b"", small[1], b""), True)
    return out


# ------------------------------------------------------------------ slice cases

SLICE_SIZES = (0, 1, 63, 64, 65, 256, 257, 1000)


@functools.lru_cache(maxsize=None)
def slice_mix():
    return tuple(ascending(n, 50 + i) for i, n in enumerate(SLICE_SIZES))


@functools.lru_cache(maxsize=None)
def slice_singles():
    """300 one-record slices (grid.y = 300)."""
    return tuple(fc.records(ascending(300, 60)))


# ------------------------------------------------------------------ mismatch cases

MISMATCH_N = (1, 255, 256, 257, 1000)


@functools.lru_cache(maxsize=None)
def mismatch_cases():
    """{name: (a, b)} of equally long lists of 64-bit words"""
    out = {}
    for n in MISMATCH_N:
        rng = np.random.RandomState(70 + n)
        a = [int(x) * 4 + 1 for x in rng.randint(0, 1 << 62, size=n, dtype=np.int64)]  # all 64 bits in use
        out[f"n{n}_equal"] = (a, list(a))
        out[f"n{n}_all_differ"] = (a, [x ^ M64 for x in a])
        at = sorted({i for i in (0, 255, 256, n - 1) if i < n})
        out[f"n{n}_edges"] = (a, [x ^ 0x10 if i in at else x for i, x in enumerate(a)])
        for bit in (0, 63):  # the lowest and the highest bit alone
            for i in at:
                out[f"n{n}_bit{bit}_at{i}"] = (a, [x ^ (1 << bit) if j == i else x for j, x in enumerate(a)])
    return out


def all_streams():
    """Every record stream of every case (the CPU test bounds their length)."""
    for s, _ in order_cases().values():
        yield s
    yield chunk_stream()
    yield tail_stream()
    yield checksum_base()
    for slices, _ in layout_cases().values():
        yield from slices
    yield from slice_mix()
    yield from slice_singles()
