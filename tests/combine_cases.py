"""Shared by the combiner tests (mapred.uda.merge.combine): a pure-Python oracle and the run sets of
the ops-level cases. The oracle merges the runs the way both backends do (key order, then run, then
position), groups by the comparator's key, sums the values modulo 2^32 / 2^64 and keeps the first
record's key bytes."""
import math
import random

from uda_amd.utils import datagen
from uda_amd.utils.ifile import decode_stream, encode_stream, text

WIDTH = {"sum.int": 4, "sum.long": 8}


def combine_records(records, key_class, op):
    """records in merged order -> one (key bytes of the first record, summed value) per group."""
    w = WIDTH[op]
    kf = datagen.sort_key(key_class)
    out = []
    last = None
    for k, v in records:
        assert len(v) == w
        ck = kf((k, v))
        if out and ck == last:
            out[-1][1] = (out[-1][1] + int.from_bytes(v, "big")) % (1 << (8 * w))
        else:
            out.append([k, int.from_bytes(v, "big")])
            last = ck
    return [(k, s.to_bytes(w, "big")) for k, s in out]


def merged_records(runs, key_class):
    recs = [kv for r in runs for kv in decode_stream(r, require_eof=False)]
    return sorted(recs, key=datagen.sort_key(key_class))  # stable: ties keep run, then position


def oracle(runs, key_class, op) -> bytes:
    return encode_stream(combine_records(merged_records(runs, key_class), key_class, op), eof=False)


def expected_task(maps, partition, key_class, op):
    recs = [kv for m in maps for kv in m[partition]]
    return combine_records(sorted(recs, key=datagen.sort_key(key_class)), key_class, op)


def _sorted_stream(recs, key_class):
    return encode_stream(sorted(recs, key=datagen.sort_key(key_class)))


def _val(rng, w):
    return rng.getrandbits(8 * w).to_bytes(w, "big")


def group_length_runs(lengths, nruns=3, w=4, seed=7):
    """Groups of exactly these lengths, back to back in key order, each group's records dealt over the runs."""
    rng = random.Random(seed)
    parts = [[] for _ in range(nruns)]
    at = 0
    for g, n in enumerate(lengths):
        for j in range(n):
            parts[(at + j) % nruns].append((text(b"g%06d" % g), _val(rng, w)))
        at += n
    return [encode_stream(p) for p in parts]  # keys ascend with g: every part is already sorted


def boundary_lengths(tile):
    """Group lengths 63..257 and tile +- 1 back to back, then groups ending exactly on, one before and one
    after every multiple (x1..x3) of the wave (64), workgroup (256) and tile sizes."""
    first = [63, 64, 65, 255, 256, 257, tile - 1, tile, tile + 1]
    start = sum(first)
    pad = (-start) % math.lcm(256, tile)  # one group that realigns the series below to every boundary
    ends = sorted({m * b + d for b in (64, 256, tile) for m in (1, 2, 3) for d in (-1, 0, 1)})
    second = [e - s for s, e in zip([0] + ends[:-1], ends)]
    return first + ([pad] if pad else []) + second


def wrap_runs(w):
    """0x7f..f + 1, negative values, and a group whose sum returns to 0, for a W-byte value."""
    key = text
    top = (1 << (8 * w - 1)) - 1
    neg = lambda x: (x % (1 << (8 * w))).to_bytes(w, "big")  # noqa: E731
    a = [(key(b"max"), top.to_bytes(w, "big")), (key(b"neg"), neg(-5)), (key(b"zero"), neg(-(1 << (8 * w - 1))))]
    b = [(key(b"max"), (1).to_bytes(w, "big")), (key(b"neg"), neg(-7)), (key(b"zero"), neg(-(1 << (8 * w - 1))))]
    c = [(key(b"neg"), neg(3)), (key(b"one"), neg(-1)), (key(b"zero"), neg(0))]
    return [encode_stream(sorted(r, key=datagen.sort_key(datagen.TEXT))) for r in (a, b, c)]


def ops_cases(tile):
    """(name, key class, op, runs)"""
    rng = random.Random(12)
    yield "wordcount", datagen.TEXT, "sum.int", [s[0] for s in datagen.streams(datagen.wordcount(9, 1, 4000))]
    one = [encode_stream([(text(b"the-only-key"), _val(rng, 4)) for _ in range(5000)]) for _ in range(6)]
    yield "one-key", datagen.TEXT, "sum.int", one
    distinct = [_sorted_stream([(text(b"d%d-%05d" % (r, i)), _val(rng, 4)) for i in range(2000)], datagen.TEXT)
                for r in range(3)]
    yield "all-distinct", datagen.TEXT, "sum.int", distinct
    yield "group-lengths", datagen.TEXT, "sum.int", group_length_runs(boundary_lengths(tile))
    pref = b"0123456789abcdef-common-prefix-"
    keys = [[text(pref + bytes([rng.randrange(97, 100)]) * rng.randint(0, 3)) for _ in range(200)] for _ in range(4)]
    yield "long-prefix", datagen.TEXT, "sum.int", [_sorted_stream([(k, _val(rng, 4)) for k in ks], datagen.TEXT)
                                                  for ks in keys]
    # equal on more than 16 bytes, differing in byte 20 or only in length, and 8-byte-prefix neighbours
    near = [b"abcdefgh", b"abcdefgh\x00", b"abcdefghi", b"abcdefghijklmnopqrst", b"abcdefghijklmnopqrsu",
            b"abcdefghijklmnopqrstu", b"abcdefg", b"", b"\x00"]
    yield "near-keys", datagen.TEXT, "sum.int", [_sorted_stream([(text(k), _val(rng, 4)) for k in near * 3],
                                                                datagen.TEXT) for _ in range(3)]
    ints = [_sorted_stream([(rng.randrange(0, 50).to_bytes(4, "big"), _val(rng, 4)) for _ in range(400)], datagen.INT)
            for _ in range(6)]
    yield "int-keys", datagen.INT, "sum.int", ints
    bw = lambda s: len(s).to_bytes(4, "big") + s  # noqa: E731
    byt = [_sorted_stream([(bw(bytes(rng.getrandbits(2) for _ in range(rng.randint(0, 6)))), _val(rng, 4))
                           for _ in range(300)] + [(bw(b""), _val(rng, 4))], datagen.BYTES) for _ in range(5)]
    yield "bytes-keys", datagen.BYTES, "sum.int", byt
    yield "wrap-int", datagen.TEXT, "sum.int", wrap_runs(4)
    yield "wrap-long", datagen.TEXT, "sum.long", wrap_runs(8)
    longs = [_sorted_stream([(text(b"w%03d" % rng.randrange(120)), _val(rng, 8)) for _ in range(700)], datagen.TEXT)
             for _ in range(4)]
    yield "long-values", datagen.TEXT, "sum.long", longs
    some = _sorted_stream([(text(b"k%02d" % (i % 7)), _val(rng, 4)) for i in range(40)], datagen.TEXT)
    yield "empty-runs", datagen.TEXT, "sum.int", [b"", encode_stream([]), some, encode_stream([]), some[:-2], b""]
    yield "nothing", datagen.TEXT, "sum.int", [b"", encode_stream([])]


def huge_key_runs():
    """Three keys of content length 65 535, 65 536 and 65 537 with identical leading bytes (the 16-bit length
    field of the merge element clamps at 0xFFFF), each in two runs: three groups."""
    keys = [text(b"z" * n) for n in (65535, 65536, 65537)]
    return [encode_stream([(k, (i + 1).to_bytes(4, "big")) for k in keys]) for i in range(2)]
