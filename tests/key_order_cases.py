"""Shared by the tests of mapred.uda.key.order=hadoop: a pure-Python oracle of the order and of the merge
under it, and the edge values of every numeric key class.

Nothing here touches the native module (the VInt writer and the record framing come from tests/generic_cases.py,
which does not either). The sortable word S of a key follows the issue's table, written with `struct` and `int`:

  Byte / Short / Int / LongWritable   big-endian two's complement v, S = v ^ 2^63 (v taken mod 2^64)
  VIntWritable / VLongWritable        v = readVLong(key), any encoding of it; S = v ^ 2^63
  FloatWritable                       Java's Float.compare: bits b, every NaN the canonical 0x7fc00000,
                                      s = b ^ (0xffffffff if b's sign bit else 0x80000000), S = s << 32
  DoubleWritable                      the same on 64 bits, canonical NaN 0x7ff8000000000000

The order of the merge is S unsigned, then run, then position in the run: one stable sort."""
import functools
import random
import struct

from tests.generic_cases import read_vlong, record, write_vlong

P = "org.apache.hadoop.io."
BYTE, SHORT, INT, LONG = P + "ByteWritable", P + "ShortWritable", P + "IntWritable", P + "LongWritable"
VINT, VLONG, FLOAT, DOUBLE = P + "VIntWritable", P + "VLongWritable", P + "FloatWritable", P + "DoubleWritable"
CLASSES = (BYTE, SHORT, INT, LONG, VINT, VLONG, FLOAT, DOUBLE)
WIDTH = {BYTE: 1, SHORT: 2, INT: 4, LONG: 8, FLOAT: 4, DOUBLE: 8}
KIND = {BYTE: 3, SHORT: 4, INT: 5, LONG: 6, VINT: 7, VLONG: 8, FLOAT: 9, DOUBLE: 10}  # uda::KeyKind
HADOOP = {"mapred.uda.key.order": "hadoop"}
SIGN = 1 << 63
M64 = (1 << 64) - 1
EOF = b"\xff\xff"


class BadKey(ValueError):
    pass


def sortable(cls, key):
    """S(key), an int in [0, 2^64); BadKey for a key of the wrong length."""
    if cls in (BYTE, SHORT, INT, LONG):
        if len(key) != WIDTH[cls]:
            raise BadKey(cls, len(key))
        return (int.from_bytes(key, "big", signed=True) & M64) ^ SIGN
    if cls in (VINT, VLONG):
        if not key:
            raise BadKey(cls, 0)
        v, used = read_vlong(key + bytes(9), 0)
        if used != len(key) or (cls == VINT and not -(1 << 31) <= v < (1 << 31)):
            raise BadKey(cls, len(key))
        return (v & M64) ^ SIGN
    if cls == FLOAT:
        if len(key) != 4:
            raise BadKey(cls, len(key))
        b, = struct.unpack(">I", key)
        if (b & 0x7fffffff) > 0x7f800000:
            b = 0x7fc00000
        return (b ^ (0xffffffff if b >> 31 else 0x80000000)) << 32
    if cls == DOUBLE:
        if len(key) != 8:
            raise BadKey(cls, len(key))
        b, = struct.unpack(">Q", key)
        if (b & ~SIGN & M64) > 0x7ff0000000000000:
            b = 0x7ff8000000000000
        return b ^ (M64 if b >> 63 else SIGN)
    raise KeyError(cls)


def merged_records(runs, cls):
    """All (key, value) of the runs (lists of records) in merged order: S, then run, then position."""
    tagged = [(sortable(cls, k), r, i, k, v) for r, run in enumerate(runs) for i, (k, v) in enumerate(run)]
    tagged.sort(key=lambda t: t[:3])
    return [(k, v) for _, _, _, k, v in tagged]


def oracle_merge(runs, cls):
    """The merged stream's record bytes, without the EOF marker."""
    return b"".join(record(k, v) for k, v in merged_records(runs, cls))


def sort_run(cls, recs):
    """A run as a map task writes it: stable in S."""
    return sorted(recs, key=lambda kv: sortable(cls, kv[0]))


def stream(recs, eof=True):
    return b"".join(record(k, v) for k, v in recs) + (EOF if eof else b"")


def fold_sum(records, cls, op):
    """The merged records combined under sum.int / sum.vint: the first record of each group of equal S, its value
    the wrapped 32-bit sum of the group's values (sum.vint: written canonically)."""
    out = []
    for k, v in records:
        x = int.from_bytes(v, "big", signed=True) if op == "sum.int" else read_vlong(v, 0)[0]
        if out and sortable(cls, out[-1][0]) == sortable(cls, k):
            out[-1][1] += x
        else:
            out.append([k, x])
    res = []
    for k, x in out:
        x &= 0xFFFFFFFF
        x -= (x >> 31) << 32
        res.append((k, x.to_bytes(4, "big", signed=True) if op == "sum.int" else write_vlong(x)))
    return res


# ------------------------------------------------------------------------------------------------ keys
def int_key(cls, v):
    return v.to_bytes(WIDTH[cls], "big", signed=True)


def noncanonical_vlong(v, n):
    """v (>= 0 here, or negative) in a VLong of n magnitude bytes, more than it needs."""
    first, m = (-120, ~v) if v < 0 else (-112, v)
    return bytes([(first - n) & 0xFF]) + m.to_bytes(n, "big")


def f32(bits):
    return struct.pack(">I", bits)


def f64(bits):
    return struct.pack(">Q", bits)


def _int_edges(bits):
    lo, hi = -(1 << (bits - 1)), (1 << (bits - 1)) - 1
    vals = {lo, lo + 1, hi, hi - 1, -1, 0, 1, -2, 2}
    for b in range(8, bits, 8):  # straddling each byte boundary, both signs
        for d in (-1, 0, 1):
            vals |= {(1 << b) + d, -(1 << b) + d, (1 << (b - 1)) + d, -(1 << (b - 1)) + d}
    return sorted(v for v in vals if lo <= v <= hi)


def _vlong_edges(bits):
    """Values at every encoded length the width allows (1..5 under VInt, 1..9 under VLong), both signs."""
    lo, hi = -(1 << (bits - 1)), (1 << (bits - 1)) - 1
    vals = {lo, hi, -1, 0, 1, -112, -113, 127, 128}
    for n in range(1, bits // 8 + 1):
        for v in ((1 << (8 * n)) - 1, 1 << (8 * n), -(1 << (8 * n)), -(1 << (8 * n)) - 1, (1 << (8 * n - 1))):
            vals.add(v)
    return sorted(v for v in vals if lo <= v <= hi)


FLOAT_BITS = (0x00000000, 0x80000000,  # +-0
              0x00000001, 0x80000001, 0x007fffff, 0x807fffff,  # +-denormals
              0x00800000, 0x80800000,  # least normals
              0x3f800000, 0x3f800001, 0x3f7fffff, 0xbf800000, 0xbf800001, 0xbf7fffff,  # adjacent around +-1
              0x7f7fffff, 0xff7fffff, 0x7f800000, 0xff800000,  # +-max, +-inf
              0x7fc00000, 0xffc00001, 0x7f800001, 0xffffffff)  # NaNs: payloads and signs differ
DOUBLE_BITS = (0x0000000000000000, 0x8000000000000000,
               0x0000000000000001, 0x8000000000000001, 0x000fffffffffffff, 0x800fffffffffffff,
               0x0010000000000000, 0x8010000000000000,
               0x3ff0000000000000, 0x3ff0000000000001, 0x3fefffffffffffff,
               0xbff0000000000000, 0xbff0000000000001, 0xbfefffffffffffff,
               0x7fefffffffffffff, 0xffefffffffffffff, 0x7ff0000000000000, 0xfff0000000000000,
               0x7ff8000000000000, 0xfff8000000000001, 0x7ff0000000000001, 0xffffffffffffffff)


@functools.lru_cache(maxsize=None)
def edge_keys(cls):
    """The class's edge keys as serialized bytes (VInt / VLong: one non-canonical encoding equal to a canonical
    one among them, of 300 and of -1)."""
    if cls in (BYTE, SHORT, INT, LONG):
        return tuple(int_key(cls, v) for v in _int_edges(8 * WIDTH[cls]))
    if cls in (VINT, VLONG):
        bits = 32 if cls == VINT else 64
        keys = [write_vlong(v) for v in _vlong_edges(bits)]
        assert {len(k) for k in keys} == set(range(1, (5 if cls == VINT else 9) + 1))  # every encoded length
        keys += [write_vlong(300), noncanonical_vlong(300, 4), noncanonical_vlong(-1, 2), noncanonical_vlong(5, 1)]
        return tuple(keys)
    if cls == FLOAT:
        return tuple(f32(b) for b in FLOAT_BITS)
    return tuple(f64(b) for b in DOUBLE_BITS)


def random_key(cls, rng):
    if cls in (BYTE, SHORT, INT, LONG):
        bits = 8 * WIDTH[cls]
        v = rng.randint(-40, 40) if rng.random() < 0.4 else rng.randint(-(1 << (bits - 1)), (1 << (bits - 1)) - 1)
        return int_key(cls, v)
    if cls in (VINT, VLONG):
        bits = rng.choice((7, 8, 9, 16, 24, 31) if cls == VINT else (7, 8, 16, 31, 33, 48, 56, 63))
        v = rng.randint(-(1 << bits), (1 << bits) - 1)
        return write_vlong(v)
    if rng.random() < 0.2:  # floats: an edge value now and then, else finite values of both signs
        return rng.choice(edge_keys(cls))
    x = rng.choice((-1, 1)) * rng.random() * 10 ** rng.randint(-3, 3)
    return struct.pack(">f" if cls == FLOAT else ">d", x)


@functools.lru_cache(maxsize=None)
def random_keys(cls, n=300):
    rng = random.Random("key-order/random/" + cls)
    return tuple(random_key(cls, rng) for _ in range(n))


def make_runs(cls, counts, seed, keys=None, vbytes=(0, 1, 4, 9), disjoint=False):
    """Sorted runs of len(counts) maps: counts[r] records whose keys are drawn from `keys` (default: the edge
    keys and random ones, negatives among them); the value names the record (run.position, then padding).
    disjoint: no two runs share a key (by S), so the merged stream does not depend on the order of the runs: a
    reduce task numbers its map outputs as their fetches complete."""
    rng = random.Random(f"key-order/runs/{cls}/{seed}")
    pool = list(keys) if keys is not None else list(edge_keys(cls)) + list(random_keys(cls))
    runs = []
    for r, n in enumerate(counts):
        mine = [k for k in pool if (sortable(cls, k) * 0x9E3779B97F4A7C15 >> 40) % len(counts) == r] if disjoint else pool
        recs = [(rng.choice(mine), b"%d.%d" % (r, i) + bytes(rng.choice(vbytes))) for i in range(n)] if mine else []
        runs.append(sort_run(cls, recs))
    return runs


TWO_VALUES = {INT: (int_key(INT, -1), int_key(INT, 0)), LONG: (int_key(LONG, -1), int_key(LONG, 0)),
              VLONG: (write_vlong(-1), write_vlong(0)), FLOAT: (f32(0x80000000), f32(0)),
              DOUBLE: (f64(0x8000000000000000), f64(0))}
