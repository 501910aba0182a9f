"""The round plan of the streaming block decode (csrc/gpu/block_rounds.cc) without a GPU, on the block
geometries of stream_cases: the plan's spans against bisect over each whole run's keys, the layout of the
round input, and `first` against a walk of the record starts. The inputs are checked first: every case's
streams decode to their partitions and the host framing walk sees the blocks that were framed."""
import bisect

import pytest

from tests import decode_cases as dc
from tests import stream_cases as sc

L = sc.L
IDS = [c.name for c in sc.CASES]


def _built(native, name):
    return sc.build(native, sc.BY_NAME[name])


def test_the_case_list_covers_what_it_promises():
    pats = {c.pattern for c in sc.CASES}
    assert pats == set(sc.PATTERNS)
    for pat in sc.PATTERNS:
        tied = [c for c in sc.CASES if c.pattern == pat and c.shape in ("heavy_key", "hi_tie")]
        assert tied, pat
        if min(pat) < 52:
            assert all(c.n <= 60 for c in sc.CASES if c.pattern == pat), pat
    assert {(c.shape, c.codec) for c in sc.CASES if c.pattern == sc.MID} >= {(s, k) for s in sc.SHAPES for k in sc.ROTATION}
    for codec in sc.ROTATION:
        mine = [c for c in sc.CASES if c.codec == codec]
        assert any(c.trailer for c in mine) and any(c.zeros for c in mine), codec
    assert any(c.split and c.codec == "snappy" for c in sc.CASES)


@pytest.mark.parametrize("name", IDS)
def test_streams_decode_to_their_partitions(native, name):
    b = _built(native, name)
    c = b.case
    assert 4 <= b.Q <= 8
    for stream, part, sizes in zip(b.streams, b.parts, b.blocks):
        body = stream[:-4] if c.trailer else stream
        got, blocks = dc.stream_decode(c.codec, body)
        assert got == part and blocks == len(sizes)
        assert native.block_decompress(sc.CODEC_ID[c.codec], body, 1 << 16) == part
    if c.split:  # the prefix decode of some block crosses a chunk
        bodies = [s[:-4] if c.trailer else s for s in b.streams]
        firsts = [len(dc.snappy_decode(chunks[0])) for s in bodies for raw, chunks in dc.blocks_of("snappy", s)
                  if len(chunks) > 1]
        assert firsts and min(firsts) < sc.PREFIX_SLOT


@pytest.mark.parametrize("name", IDS)
def test_host_walk_sees_the_framed_blocks(native, name):
    b = _built(native, name)
    c = b.case
    for tails in (c.trailer, True):
        got = native.plan_block_streams_descs(sc.CODEC_ID[c.codec], list(b.streams), tails)
        want = sc.walk(c.codec, b.streams, tails)
        assert got is not None and want is not None
        descs, raw_offset, tl = got
        assert [list(map(int, d)) for d in descs] == [list(d) for d in want[0]]
        assert list(raw_offset) == want[1] and list(tl) == want[2]
        assert tl == ([4 if c.trailer else 0] * len(b.streams) if tails else [])
        per = [[d[4] for d in descs if d[0] == k] for k in range(len(b.streams))]
        assert per == [list(s) for s in b.blocks]
        assert [raw_offset[k + 1] - raw_offset[k] for k in range(len(b.parts))] == [len(p) for p in b.parts]


def _check_plan(b, plan, round_bytes):
    K = len(b.runs)
    nrec = [len(r) // L for r in b.runs]
    total = sum(nrec) * L
    Q = plan["Q"]
    assert plan["sorted"] and Q == max(1, -(-total // round_bytes))
    bounds = plan["bounds"]
    assert len(bounds) == Q - 1 and bounds == sorted(bounds)
    blk0, rel = [0], []
    for sizes in b.blocks:
        r = 0
        for raw in sizes:
            rel.append(r)
            r += raw
        blk0.append(len(rel))
    raws = [raw for sizes in b.blocks for raw in sizes]
    keys = [sc.run_keys(r) for r in b.runs]
    assert len(plan["spans"]) == Q and len(plan["in_bytes"]) == Q and len(plan["in_recs"]) == Q
    prev_hi = [0] * K
    for q in range(Q):
        row = plan["spans"][q]
        assert len(row) == K
        end, recs = 0, 0
        for k, sp in enumerate(row):
            if nrec[k] == 0:
                continue  # nothing decoded for an EOF-only stream; its cut is [0, 0)
            b0, b1, rec0, rec1, in_off = sp["b0"], sp["b1"], sp["rec0"], sp["rec1"], sp["in_off"]
            assert blk0[k] <= b0 <= b1 < blk0[k + 1], (q, k, sp)
            r0, r1 = rel[b0], rel[b1] + raws[b1]
            assert 0 <= rec0 <= rec1 <= nrec[k] and r0 <= rec0 * L and rec1 * L <= max(r1, rec0 * L), (q, k, sp)
            # the whole records of the decoded bytes, all of them
            assert rec0 == -(-r0 // L) and (rec1 == min(r1 // L, nrec[k]) or rec1 == rec0), (q, k, sp)
            assert (in_off + rec0 * L - r0) % 16 == 0, (q, k, sp)
            assert in_off >= end, (q, k, sp)
            end = in_off + (r1 - r0)
            recs += rec1 - rec0
            # the records of the span cut at the round's bounds are the round's records of the whole run
            span = keys[k][rec0:rec1]
            a = bisect.bisect_left(span, bounds[q - 1]) if q > 0 else 0
            e = bisect.bisect_left(span, bounds[q]) if q + 1 < Q else len(span)
            lo = bisect.bisect_left(keys[k], bounds[q - 1]) if q > 0 else 0
            hi = bisect.bisect_left(keys[k], bounds[q]) if q + 1 < Q else nrec[k]
            assert (rec0 + a, rec0 + max(e, a)) == (lo, hi), (q, k, sp, a, e, lo, hi)
            assert lo == prev_hi[k], (q, k)
            prev_hi[k] = hi
        assert plan["in_bytes"][q] % 256 == 0 and plan["in_bytes"][q] >= end, q
        assert plan["in_recs"][q] == recs, q
    assert prev_hi == nrec


@pytest.mark.parametrize("name", IDS)
def test_round_plan_against_bisect(native, name):
    b = _built(native, name)
    total = b.N * L
    for rb in (b.round_bytes, -(-total // 4), -(-total // 8), total + 1):
        _check_plan(b, sc.plan_of(native, b, rb), rb)


@pytest.mark.parametrize("name", IDS)
def test_first_offsets(native, name):
    b = _built(native, name)
    plan = sc.plan_of(native, b)
    want = sc.first_offsets(b.parts, b.blocks)
    assert plan["first"] == want
    raws = [raw for sizes in b.blocks for raw in sizes]
    if max(raws) < 13:
        assert set(want) == {-1}
    if b.case.pattern in ((104,), (208,)):
        assert set(want) <= {0, -1} and want.count(-1) == sum(1 for p in b.parts if len(p) > 2)  # the EOF's block


def test_descending_block_keys_are_not_planned(native):
    b = _built(native, "uniform-lz4-mid")
    parts = list(b.parts)
    recs = [parts[0][i:i + L] for i in range(0, len(parts[0]) - 2, L)]
    parts[0] = b"".join(reversed(recs)) + sc.EOF
    plan = native.block_round_plan([len(r) // L for r in b.runs], [list(x) for x in b.blocks],
                                   sc.first_keys(parts, b.blocks), b.round_bytes)
    assert plan["sorted"] is False and "spans" not in plan


def test_plan_of_eof_only_streams(native):
    plan = native.block_round_plan([0, 0, 0], [[2], [1, 1], [2]], [None] * 4, 1000)
    assert plan["first"] == [-1] * 4 and plan["Q"] == 1 and plan["in_recs"] == [0] and plan["in_bytes"] == [0]


def test_plan_rejects_blocks_that_do_not_hold_the_stream(native):
    with pytest.raises(ValueError):
        native.block_round_plan([1], [[104]], [None], 1000)
    with pytest.raises(ValueError):
        native.block_round_plan([1], [[106]], [None], 1000)  # a record starts in the block: its key is needed
