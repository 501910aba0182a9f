"""GPU: the key-range round planner (csrc/gpu/generic_rounds.hip: gr_sample_kernel, gr_split_kernel,
gr_lastkey_kernel, over the F1 index in its whole and its partial mode, parallel and serial) on the cases of
tests/rounds_cases.py. Every position, bound and split is compared exactly with that module's pure-Python
oracle, never with the CPU merge or another device path."""
import pytest

from tests import generic_cases as gc
from tests import rounds_cases as rc
from uda_amd import ops

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def geo(native):
    return {**native.gpu_generic_geometry(), **native.gpu_rounds_geometry()}


def _plan(c, misalign=0, round_bytes=None):
    return ops.plan_generic_rounds(list(c.streams), str(c.cls), round_bytes or c.round_bytes,
                                   key_order=rc.key_order(c.cls), misalign=misalign)


# ------------------------------------------------------------------------------------------------ rounds
@pytest.mark.parametrize("name", rc.PLAN_NAMES)
def test_plan_satisfies_the_oracle(require_gpu, geo, name):
    c = rc.plan_case(name, geo)
    plan = _plan(c)
    print(name, "want", c.want, "rounds", plan["rounds"], "max_round_bytes", plan["max_round_bytes"])
    rc.check_plan(c.streams, c.cls, c.round_bytes, plan, geo)
    if name == "uniform-text":  # distinct keys: nothing keeps a bound from being its own
        assert plan["rounds"] == c.want
    elif name == "heavy-key":  # most samples are the one key: bounds collapse (check_plan: it sits in one round)
        assert 2 <= plan["rounds"] < c.want and rc.HEAVY in plan["bounds"]
    elif name == "shared-prefix":  # only the two truncated samples there are
        n, body = geo["sample_key"], rc.shared_prefix_body(geo)
        assert body[:n] in plan["bounds"] and set(plan["bounds"]) <= {body[:n - 1], body[:n]}
    elif name == "tiny-runs":
        assert plan["bounds"][0] == b"" and plan["rounds"] >= 3
        ends = [rc.record_bytes(s) for s in c.streams]
        below, above = c.meta["below"], c.meta["above"]
        assert plan["pos"][below][2:-1] == [ends[below]] * (plan["rounds"] - 2)
        assert plan["pos"][above][:-1] == [0] * plan["rounds"]
        assert all(p[1] == 0 for p in plan["pos"])  # nothing is below the empty string
    elif name.startswith("numeric"):
        assert all(len(b) == 8 for b in plan["bounds"]) and plan["rounds"] >= 3
    elif name == "strided-sample":
        assert plan["rounds"] >= 2
    else:
        assert plan["rounds"] >= 3


@pytest.mark.parametrize("misalign", rc.MISALIGN)
@pytest.mark.parametrize("name", rc.MISALIGNED)
def test_misaligned_runs(require_gpu, geo, name, misalign):
    c = rc.plan_case(name, geo)
    plan = _plan(c, misalign=misalign)
    rc.check_plan(c.streams, c.cls, c.round_bytes, plan, geo)
    assert plan["rounds"] >= 3


def test_trivial_plans(require_gpu, geo):
    c = rc.plan_case("uniform-text", geo)
    total = sum(len(s) for s in c.streams)
    trivial = {"rounds": 1, "pos": [[0, len(s)] for s in c.streams], "bounds": [], "max_round_bytes": total}
    for round_bytes in (total, total + 1, 1 << 40):
        assert _plan(c, round_bytes=round_bytes) == trivial
    rc.check_plan(c.streams, c.cls, total, trivial, geo)
    assert _plan(c, round_bytes=total - 1)["rounds"] >= 2  # one byte more than a round: distinct keys, a bound
    assert ops.plan_generic_rounds([], gc.TEXT, 1024) == {"rounds": 1, "pos": [], "bounds": [], "max_round_bytes": 0}
    # runs without a record have no key to split by
    empty = ops.plan_generic_rounds([b"", gc.EOF, gc.EOF], gc.TEXT, 1)
    assert empty == {"rounds": 1, "pos": [[0, 0], [0, 2], [0, 2]], "bounds": [], "max_round_bytes": 4}


def test_a_truncated_whole_run_is_an_error(require_gpu, geo):
    """Only the partial mode forgives a record cut by the end: a whole run that ends inside a record, in its
    header or with half a marker fails the plan (parallel index and serial re-index)."""
    for name in ("uniform-text", "long-records"):
        c = rc.plan_case(name, geo)
        k = 2
        assert gc.f1_goes_serial(c.streams[k], geo) == (name == "long-records")
        recs = rc.records_below(c.streams[k], rc.record_bytes(c.streams[k]))
        s, e, key = recs[-1]
        for cut in (e - 1, (s + e) // 2, s + 1, len(c.streams[k]) - 1):
            streams = list(c.streams)
            streams[k] = streams[k][:cut]
            with pytest.raises(RuntimeError, match=f"corrupt or truncated IFile run {k}"):
                ops.plan_generic_rounds(streams, str(c.cls), c.round_bytes)
    assert _plan(c)["rounds"] >= 3  # and the planner is usable afterwards


# ------------------------------------------------------------------------------------------------ split
def _split(call, fill):
    return ops.plan_progressive_split(call.with_tail(fill), list(call.avail), list(call.final), str(call.cls),
                                      key_order=rc.key_order(call.cls))


@pytest.mark.parametrize("family", rc.SPLIT_FAMILIES)
def test_progressive_splits_equal_the_oracle(require_gpu, geo, family):
    """Every call of rounds_cases.split_calls, three times: the bytes that have not landed being the true
    continuation, all 0xFF and all 0x00. All three results are the oracle's, exactly."""
    calls = [c for c in rc.split_calls(geo) if c.name.startswith(family)]
    assert calls
    cuts = 0
    for call in calls:
        for fill in rc.TAILS:
            got = _split(call, fill)
            assert got == call.expected, (call.name, fill, _first_difference(got, call.expected, call))
        cuts += len(call.windows)
    print(len(calls), "calls,", cuts, "cuts")


def _first_difference(got, want, call):
    for key in ("bounded", "bound"):
        if got[key] != want[key]:
            return key, got[key], want[key]
    for key in ("complete", "split"):
        for k, (a, b) in enumerate(zip(got[key], want[key])):
            if a != b:
                return key, k, "avail", call.avail[k], "final", call.final[k], "got", a, "want", b
    return None


def test_progressive_split_of_misaligned_windows(require_gpu, geo):
    calls = [c for c in rc.split_calls(geo) if c.name.endswith("-arriving")]
    for call, misalign in zip(calls, rc.MISALIGN * len(calls)):
        got = ops.plan_progressive_split(list(call.windows), list(call.avail), list(call.final), str(call.cls),
                                         key_order=rc.key_order(call.cls), misalign=misalign)
        assert got == call.expected, (call.name, misalign, _first_difference(got, call.expected, call))


def test_progressive_split_of_nothing(require_gpu, geo):
    assert ops.plan_progressive_split([], [], [], gc.TEXT) == {"complete": [], "split": [], "bounded": False, "bound": b""}
    w = rc.plan_case("uniform-text", geo).streams[0]
    for final in (False, True):
        got = ops.plan_progressive_split([w, w], [0, 0], [final, final], gc.TEXT)
        assert got == {"complete": [0, 0], "split": [0, 0], "bounded": False, "bound": b""}
