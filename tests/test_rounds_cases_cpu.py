"""The round-planning cases of tests/rounds_cases.py on the host: every family still has the property it was
built for (the boundaries come from native.gpu_generic_geometry() and native.gpu_rounds_geometry()), the
oracle's searches agree with a brute-force walk, expected_split is safe and maximal, and check_plan rejects
plans that are wrong in the ways the planner could be."""
import copy

import pytest

from tests import generic_cases as gc
from tests import rounds_cases as rc


@pytest.fixture(scope="module")
def geo(native):
    return {**native.gpu_generic_geometry(), **native.gpu_rounds_geometry()}


def _records(s):
    return rc.records_below(s, rc.record_bytes(s))


def _chunks_without_start(s, chunk):
    starts = {st // chunk for st, _, _ in _records(s)}
    return [c for c in range((rc.record_bytes(s) + chunk - 1) // chunk) if c not in starts]


def test_rounds_geometry_binding(native):
    g = native.gpu_rounds_geometry()
    assert set(g) == {"sample_key", "samples_per_round"}
    assert all(isinstance(v, int) and v > 0 for v in g.values())
    assert g["sample_key"] < 127  # the shared-prefix lengths straddle it below the 2-byte Text VInt


# ------------------------------------------------------------------------------------------------ families
@pytest.mark.parametrize("name", rc.PLAN_NAMES)
def test_case_shape(geo, name):
    """Several rounds wanted, and runs of a size the GPU tests stay quick on."""
    c = rc.plan_case(name, geo)
    if name == "strided-sample":  # the one case large enough for the planner to sample fewer chunks than there are
        chunks = sum(-(-len(s) // geo["f1_chunk"]) for s in c.streams)
        assert c.want == 2 and chunks > c.want * geo["samples_per_round"]
        assert all(_chunks_without_start(s, geo["f1_chunk"]) for s in c.streams)
        return
    assert c.want >= 3 and sum(len(s) for s in c.streams) < 2 << 20
    if not name.startswith("reused-"):  # (those runs are as long as tests/generic_cases.py needs them)
        assert max(len(s) for s in c.streams) <= 60 << 10 and c.want <= 16


def test_uniform_text(geo):
    c = rc.plan_case("uniform-text", geo)
    keys = [rc.sort_content(c.cls, k) for s in c.streams for _, _, k in _records(s)]
    assert len(c.streams) == 5 and len(set(keys)) == len(keys)
    assert min(map(len, keys)) >= 22 and max(map(len, keys)) <= 62 < geo["sample_key"] + 1
    assert all(8 << 10 <= len(s) <= 60 << 10 for s in c.streams)


def test_long_records(geo):
    c = rc.plan_case("long-records", geo)
    chunk = geo["f1_chunk"]
    sizes = [[e - s for s, e, _ in _records(st)] for st in c.streams]
    assert all(5000 <= n <= 13 << 10 for run in sizes for n in run if n > 200)
    assert sizes[0][0] > 5000 and sizes[1][-1] > 5000 and max(sizes[4]) < 200
    two = [i for i, n in enumerate(sizes[2]) if n > 5000]
    assert len(two) == 2 and two[1] == two[0] + 1
    assert max(sizes[3]) > 3 * chunk  # spans three chunks wherever it starts
    # chunks in which no record starts, in every run that has a long record
    assert all(_chunks_without_start(s, chunk) for s in c.streams[:4]) and not _chunks_without_start(c.streams[4], chunk)
    # the serial re-index and the parallel index both take some of the runs
    serial = [gc.f1_goes_serial(s, geo) for s in c.streams]
    assert serial[0] is False and serial[4] is False and 1 <= sum(serial) < len(serial), serial
    # the record after a long one leads its chunk
    for st in c.streams:
        recs = _records(st)
        for (s, e, _), nxt in zip(recs, recs[1:]):
            if e - s > 5000:
                assert rc.sort_content(c.cls, nxt[2])[:geo["sample_key"]] in rc.chunk_leading_keys([st], c.cls, geo)


def test_shared_prefix(geo):
    c = rc.plan_case("shared-prefix", geo)
    n, body = geo["sample_key"], rc.shared_prefix_body(geo)
    contents = {rc.sort_content(c.cls, k) for s in c.streams for _, _, k in _records(s)}
    assert {len(x) for x in contents} == {n - 1, n, n + 1, n + 2, 127, 128, 300}
    assert all(x[:n] == body[:n] for x in contents if len(x) >= n) and body[:n - 1] in contents and body[:n] in contents
    # one shared truncated sample; the shorter key leads run 0 alone
    assert rc.chunk_leading_keys(c.streams[1:], c.cls, geo) == {body[:n]}
    assert rc.chunk_leading_keys(c.streams, c.cls, geo) == {body[:n - 1], body[:n]}
    assert body[:n - 1] < body[:n] < body[:n] + b"\x00" and len(gc.text(body[:128])) == 130
    # split by it, the equal key is not below the bound and the shorter one is
    plan = rc.make_plan(c.streams, c.cls, [body[:n]])
    assert plan["pos"][0][1] == 5 * len(gc.record(gc.text(body[:n - 1]), b"short.0"))
    assert [p[1] for p in plan["pos"][1:]] == [0, 0, 0]
    rc.check_plan(c.streams, c.cls, sum(map(len, c.streams)) // 2 + 1, plan, geo)


def test_heavy_key(geo):
    c = rc.plan_case("heavy-key", geo)
    keys = [rc.sort_content(c.cls, k) for s in c.streams for _, _, k in _records(s)]
    heavy = sum(len(rc.record(*kv)) for s in c.streams for kv in rc._slice_records(s, 0, rc.record_bytes(s))
                if rc.sort_content(c.cls, kv[0]) == rc.HEAVY)
    assert 0.65 <= keys.count(rc.HEAVY) / len(keys) <= 0.75
    assert heavy > 3 * c.round_bytes  # several rounds' worth of one key
    assert min(keys) < rc.HEAVY < max(keys)


def test_tiny_runs(geo):
    c = rc.plan_case("tiny-runs", geo)
    s = c.streams
    assert len(s) == 7 and s[0] == b"" and s[1] == gc.EOF and s[2] == s[3] + gc.EOF and len(_records(s[3])) == 1
    keys = [[rc.sort_content(c.cls, k) for _, _, k in _records(x)] for x in s]
    others = [k for i in (2, 3, 6) for k in keys[i] if k]
    assert max(keys[c.meta["below"]]) < min(others) and min(keys[c.meta["above"]]) > max(others)
    assert keys[6][0] == b"" and b"" in rc.chunk_leading_keys(s, c.cls, geo)


def test_eof_at_chunk_edge(geo):
    c = rc.plan_case("eof-at-chunk-edge", geo)
    chunk = geo["f1_chunk"]
    got = {(rc.record_bytes(s) % chunk, len(s) - rc.record_bytes(s)) for s in c.streams}
    assert got == {(m, e) for m in (0, 1, chunk - 1, chunk - 2) for e in (0, 2)}


def test_numeric_bytes_raw_and_fan_in(geo):
    for name in ("numeric-int", "numeric-long", "numeric-vlong", "numeric-float"):
        c = rc.plan_case(name, geo)
        keys = [k for s in c.streams for _, _, k in _records(s)]
        words = [rc.sort_content(c.cls, k) for k in keys]
        assert all(len(w) == 8 for w in words) and rc.key_order(c.cls) == "hadoop"
        assert any(w < b"\x80" for w in words) and any(w >= b"\x80" for w in words)  # both signs
        assert sorted(keys) != sorted(keys, key=lambda k: rc.sort_content(c.cls, k))  # byte order is not key order
    raw = rc.plan_case("raw", geo)
    assert rc.key_order(raw.cls) == "reference" and rc.sort_content(raw.cls, b"\xff" * 8) == b"\xff" * 8
    fan = rc.plan_case("fan-in", geo)
    assert len(fan.streams) == 130 and len(fan.streams) * (fan.want - 1) > 64
    assert b"" in fan.streams and gc.EOF in fan.streams


# ------------------------------------------------------------------------------------------------ oracle
def _brute_records(s):
    """(start, content) by another road: generic_cases.parse and the sizes of the re-encoded records."""
    out, pos = [], 0
    for k, v in gc.parse(s, require_eof=False):
        out.append((pos, k))
        pos += len(gc.record(k, v))
    return out, pos


@pytest.mark.parametrize("name", ["long-records", "shared-prefix", "tiny-runs", "numeric-vlong", "bytes"])
def test_first_not_below_against_brute_force(geo, name):
    c = rc.plan_case(name, geo)
    n = geo["sample_key"]
    for s in c.streams:
        recs, end = _brute_records(s)
        assert end == rc.record_bytes(s)
        contents = [rc.sort_content(c.cls, k) for _, k in recs]
        probes = {b"", b"\xff" * 9} | {x for x in contents[::17]} | {x[:n] for x in contents[::13]}
        probes |= {x + b"\x00" for x in contents[::29]} | {x[:-1] for x in contents[::31] if x}
        for b in probes:
            want = next((st for (st, _), x in zip(recs, contents) if not x < b), end)
            assert rc.first_not_below(s, end, c.cls, b) == want
        if len(recs) > 3:  # a limit below the run's end hides the records from it on
            lim = recs[len(recs) // 2][0]
            assert rc.first_not_below(s, lim, c.cls, b"\xff" * 9) == lim
            assert rc.first_not_below(s, lim, c.cls, contents[-1]) == min(
                lim, next(st for (st, _), x in zip(recs, contents) if not x < contents[-1]))


def test_complete_prefix_against_brute_force(geo):
    for name in ("eof-at-chunk-edge", "reused-hdr-straddle", "numeric-vlong"):
        c = rc.plan_case(name, geo)
        s = c.streams[0][:3000] if len(c.streams[0]) > 3000 else c.streams[0]
        s = s[:rc.complete_prefix(s, len(s))] + gc.EOF
        ends = [0] + [e for _, e, _ in _records(s)]
        for avail in range(len(s) + 1):
            assert rc.complete_prefix(s, avail) == max(e for e in ends if e <= avail), (name, avail)
    w = gc.record(gc.text(b"k" * 200), b"v" * 300) + gc.EOF  # multi-byte VInts in the header
    for avail in range(len(w) + 1):
        assert rc.complete_prefix(w, avail) == (len(w) - 2 if avail >= len(w) - 2 else 0)


def test_split_calls_cover_the_cuts(geo):
    calls = rc.split_calls(geo)
    chunk = geo["f1_chunk"]
    assert max(len(c.windows) for c in calls) > 48 and sum(len(c.windows) for c in calls) > 600
    flags = {(all(c.final), any(c.final)) for c in calls}
    assert flags == {(True, True), (False, True), (False, False)}
    # a window that is not final and holds no whole record
    assert sum(any(x == 0 and not f for x, f in zip(c.expected["complete"], c.final)) for c in calls) >= 6
    # cuts inside a header, a key and a value, on a record's end, and with half a marker or none
    kinds = set()
    for c in calls:
        for w, a, done in zip(c.windows, c.avail, c.expected["complete"]):
            if a == len(w) - 1 and w.endswith(gc.EOF):
                kinds.add("half-marker")
            if a == len(w) - 2 and w.endswith(gc.EOF):
                kinds.add("no-marker")
            if a == done and a < len(w) - 2:
                kinds.add("on-a-record-end")
            if done < a < len(w) - 2:
                h = rc._header(w, done)
                kl = gc.read_vlong(w, done)[0]
                kinds.add("in-header" if a < done + h else "in-key" if a < done + h + kl else "in-value")
                if a - done > 2 * chunk:
                    kinds.add("deep-in-a-long-record")
    assert kinds == {"half-marker", "no-marker", "on-a-record-end", "in-header", "in-key", "in-value",
                     "deep-in-a-long-record"}
    # windows begin at a record start that is not the run's first byte
    lr = rc.plan_case("long-records", geo).streams
    assert all(not any(s.startswith(c.windows[0]) for s in lr) for c in calls if c.name.startswith("long-records"))


def test_expected_split_is_safe_and_maximal(geo):
    """Merging [0, split) of every window and then the rest gives the merge of everything the runs hold (so no
    record that is still to land, which is not below its window's last landed key, can precede a merged one),
    and the first record left behind in a window is not below the bound."""
    merged_something = 0
    for c in rc.split_calls(geo):
        if c.name.startswith("len-edges"):
            continue  # (the same code on 200 KB windows: the time goes to the other calls)
        exp = c.expected
        n = geo["sample_key"]
        ends = [rc.record_bytes(w) for w in c.windows]
        assert all(0 <= s <= done <= a for s, done, a in zip(exp["split"], exp["complete"], c.avail))
        if not exp["bounded"]:
            assert exp["bound"] == b""
            assert exp["split"] == (exp["complete"] if all(c.final) else [0] * len(c.windows))
            continue
        head = [rc._slice_records(w, 0, s) for w, s in zip(c.windows, exp["split"])]
        rest = [rc._slice_records(w, s, e) for w, s, e in zip(c.windows, exp["split"], ends)]
        whole = [rc._slice_records(w, 0, e) for w, e in zip(c.windows, ends)]
        assert rc._merged(head, c.cls) + rc._merged(rest, c.cls) == rc._merged(whole, c.cls), c.name
        merged_something += any(head)  # (a bound that is the least key of all lets nothing through)
        lasts = []
        for w, s, done, f in zip(c.windows, exp["split"], exp["complete"], c.final):
            if s < done:
                assert not rc.sort_content(c.cls, rc.records_below(w, done)[len(rc.records_below(w, s))][2]) < exp["bound"]
            if not f:
                lasts.append(rc.sort_content(c.cls, rc.records_below(w, done)[-1][2])[:n])
        assert exp["bound"] == min(lasts)
    assert merged_something >= 20


# ------------------------------------------------------------------------------------------------ check_plan
def _good_plan(c, geo, nb=3):
    leading = sorted(rc.chunk_leading_keys(c.streams, c.cls, geo))
    bounds = [leading[(i + 1) * len(leading) // (nb + 1)] for i in range(nb)]
    assert len(set(bounds)) == nb
    return rc.make_plan(c.streams, c.cls, bounds)


@pytest.mark.parametrize("name", ["uniform-text", "long-records", "numeric-int", "bytes"])
def test_check_plan_accepts_a_right_plan(geo, name):
    c = rc.plan_case(name, geo)
    rc.check_plan(c.streams, c.cls, c.round_bytes, _good_plan(c, geo), geo)


def test_check_plan_rejects_wrong_plans(geo):
    c = rc.plan_case("uniform-text", geo)
    good = _good_plan(c, geo)

    def rejected(plan, case=c):
        with pytest.raises(AssertionError):
            rc.check_plan(case.streams, case.cls, case.round_bytes, plan, geo)

    # a position off by one record, either way
    recs = _records(c.streams[2])
    i = [s for s, _, _ in recs].index(good["pos"][2][2])
    for j in (i - 1, i + 1):
        bad = copy.deepcopy(good)
        bad["pos"][2][2] = recs[j][0]
        bad["max_round_bytes"] = rc.make_plan(c.streams, c.cls, good["bounds"])["max_round_bytes"]
        rejected(bad)
    # a bound that no chunk leads (the positions follow it faithfully)
    leading = rc.chunk_leading_keys(c.streams, c.cls, geo)
    other = next(x for x in (rc.sort_content(c.cls, k) for _, _, k in recs) if x not in leading and x > good["bounds"][0]
                 and x < good["bounds"][1])
    rejected(rc.make_plan(c.streams, c.cls, [good["bounds"][0], other, good["bounds"][2]]))
    # bounds out of order, a missing bound, more rounds than wanted, a wrong maximum
    rejected(dict(good, bounds=good["bounds"][::-1]))
    rejected(dict(good, bounds=good["bounds"][:2]))
    rejected(dict(good, max_round_bytes=good["max_round_bytes"] + 1))
    with pytest.raises(AssertionError):
        rc.check_plan(c.streams, c.cls, sum(map(len, c.streams)) // 2, good, geo)
    # an equal key split over two rounds: the heavy key, cut in the middle of run 1's group
    h = rc.plan_case("heavy-key", geo)
    plan = rc.make_plan(h.streams, h.cls, [rc.HEAVY])
    rc.check_plan(h.streams, h.cls, h.round_bytes, plan, geo)
    group = [s for s, _, k in _records(h.streams[1]) if rc.sort_content(h.cls, k) == rc.HEAVY]
    plan["pos"][1][1] = group[len(group) // 2]
    rejected(plan, h)
