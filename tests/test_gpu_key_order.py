"""GPU: mapred.uda.key.order=hadoop in the generic device merge (normalize_numeric_kernel of csrc/gpu/generic.hip,
the key-range rounds of generic_rounds.hip, the combiner's side-table reads) against the pure-Python oracle of
tests/key_order_cases.py, byte for byte: the order at the kernels' boundaries, every path a reduce task can
take, the combiner over VIntWritable keys, a key of the wrong length, and the default order left as it was.
Shapes come from native.gpu_generic_geometry(), so they move with the kernels."""
import functools

import pytest

import uda_amd
from tests import generic_cases as gc
from tests import key_order_cases as ko
from tests.generic_cases import record, write_vlong
from uda_amd import ops
from uda_amd.bridge import UdaConsumer, UdaFallback, UdaProvider, run_reduce
from uda_amd.utils.mof import encode_partitions

pytestmark = pytest.mark.gpu
GPU = {"mapred.uda.merge.backend": "gpu"}
GPU_HADOOP = dict(GPU, **ko.HADOOP)
ORDER_CLASSES = (ko.INT, ko.LONG, ko.VLONG, ko.FLOAT, ko.DOUBLE)
SHAPES = ("k1", "k2", "k3-cap-1", "k3-cap", "k3-cap+1", "k17-20cap", "k-pairwise", "all-equal", "two-values", "one-empty")


def short(cls):
    return cls.rsplit(".", 1)[1]


@functools.lru_cache(maxsize=None)
def geometry():
    return dict(uda_amd.native().gpu_generic_geometry())


def deal(total, K):
    """`total` records over K runs of unequal lengths."""
    weights = [1 + (3 * r) % 5 for r in range(K)]
    counts = [total * w // sum(weights) for w in weights]
    counts[0] += total - sum(counts)
    return tuple(counts)


@functools.lru_cache(maxsize=None)
def shape_runs(cls, shape):
    """The runs of a shape, built once. cap: records of a K-way cell; gk_max_runs: the single-pass limit."""
    geo = geometry()
    cap, kmax = geo["gk_cap"], geo["gk_max_runs"]
    if shape == "k1":
        return ko.make_runs(cls, (cap // 3,), seed=shape)
    if shape == "k2":
        return ko.make_runs(cls, deal(cap // 2, 2), seed=shape)
    if shape.startswith("k3-cap"):
        total = cap + {"k3-cap-1": -1, "k3-cap": 0, "k3-cap+1": 1}[shape]
        return ko.make_runs(cls, deal(total, 3), seed=shape)
    if shape == "k17-20cap":
        return ko.make_runs(cls, deal(20 * cap, 17), seed=shape)
    if shape == "k-pairwise":  # more runs than the K-way cells take: the pairwise passes
        return ko.make_runs(cls, deal(3 * cap, kmax + 1), seed=shape)
    if shape == "all-equal":  # the order comes from the ordinal ties alone
        return ko.make_runs(cls, deal(cap + 1, 3), seed=shape, keys=ko.TWO_VALUES[cls][:1])
    if shape == "two-values":  # -0.0 / +0.0, -1 / 0
        return ko.make_runs(cls, deal(cap + 1, 3), seed=shape, keys=ko.TWO_VALUES[cls])
    if shape == "one-empty":
        counts = list(deal(cap + 1, 3))
        counts[1] = 0
        return ko.make_runs(cls, tuple(counts), seed=shape)
    raise KeyError(shape)


# ------------------------------------------------------------------------------------------------ order
@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("cls", ORDER_CLASSES, ids=[short(c) for c in ORDER_CLASSES])
def test_device_merge_matches_the_oracle(require_gpu, cls, shape):
    """Fails without the feature: the merge has no key_order, Float / Double / VLong keys no kind."""
    runs = shape_runs(cls, shape)
    want = ko.oracle_merge(runs, cls)
    body, cuts = ops.merge_runs([ko.stream(r) for r in runs], cls, "gpu", kv_buf=4096, key_order="hadoop")
    assert body == want
    assert cuts[0] == 0 and cuts[-1] == len(want) and all(0 < b - a <= 4094 for a, b in zip(cuts, cuts[1:]))
    assert ops.last_stats["records"] == sum(len(r) for r in runs)
    if shape == "k-pairwise":
        assert ops.last_stats["passes"] > 1
    if shape == "k1":
        assert ops.last_stats["passes"] == 0


@pytest.mark.parametrize("cls", (ko.BYTE, ko.SHORT, ko.VINT), ids=["ByteWritable", "ShortWritable", "VIntWritable"])
def test_device_merge_of_the_narrow_classes(require_gpu, cls):
    runs = ko.make_runs(cls, deal(geometry()["gk_cap"] + 1, 3), seed="narrow")
    body, _ = ops.merge_runs([ko.stream(r) for r in runs], cls, "gpu", kv_buf=4096, key_order="hadoop")
    assert body == ko.oracle_merge(runs, cls)


def test_streamed_rounds_match_the_oracle(require_gpu):
    """GenericMerger's key-range rounds of cells read the normalized keys through the same side tables."""
    runs = shape_runs(ko.DOUBLE, "k17-20cap")
    want = ko.oracle_merge(runs, ko.DOUBLE)
    body, cuts, st = ops.merge_runs_streamed([ko.stream(r) for r in runs], ko.DOUBLE, kv_buf=4096,
                                             round_bytes=len(want) // 7, key_order="hadoop")
    assert body == want and len(st["rounds"]) >= 4 and sum(n for n, _ in st["rounds"]) == st["records"]


def test_default_order_is_unchanged(require_gpu):
    """The same negative IntWritable keys under the default order: the reference's memcmp, from the oracle of
    tests/generic_cases.py (runs sorted the way that order wants them)."""
    runs = [sorted(r, key=lambda kv: kv[0]) for r in shape_runs(ko.INT, "k3-cap+1")]
    streams = [gc.stream(r) for r in runs]
    want = b"".join(gc.oracle_merge(runs, gc.INT))
    assert want != ko.oracle_merge(shape_runs(ko.INT, "k3-cap+1"), ko.INT)  # negatives present: the orders differ
    body, _ = ops.merge_runs(streams, ko.INT, "gpu", kv_buf=4096)
    assert body == want
    body, _ = ops.merge_runs(streams, ko.INT, "gpu", kv_buf=4096, key_order="reference")
    assert body == want
    with pytest.raises(ValueError, match="unsupported key class"):
        ops.merge_runs(streams, ko.DOUBLE, "gpu")


# ------------------------------------------------------------------------------------------------ combine
def test_sum_vint_folds_two_encodings_of_a_key(require_gpu):
    """VIntWritable keys, VInt values: a key written canonically in one run and with spare magnitude bytes in
    another is one group. The group's head is its first record in run order, so its key bytes are run 0's."""
    values = (-70000, -300, -113, -1, 0, 1, 127, 128, 300, 70000)
    canon = [write_vlong(v) for v in values]
    wide = [ko.noncanonical_vlong(v, 4) for v in values]
    assert all(ko.sortable(ko.VINT, a) == ko.sortable(ko.VINT, b) and a != b for a, b in zip(canon, wide))
    runs = [[(k, write_vlong(3 * i + r)) for i, k in enumerate(keys) for _ in range(40 + r)]
            for r, keys in enumerate((canon, wide, canon))]
    merged = ko.merged_records(runs, ko.VINT)
    want = ko.fold_sum(merged, ko.VINT, "sum.vint")
    assert [k for k, _ in want] == canon
    body, _ = ops.merge_runs([ko.stream(r) for r in runs], ko.VINT, "gpu", kv_buf=4096, combine="sum.vint",
                             key_order="hadoop")
    assert body == b"".join(record(k, v) for k, v in want)
    assert ops.last_stats["records"] == len(values) and ops.last_stats["records_in"] == len(merged)


def test_sum_int_over_negative_int_keys(require_gpu):
    keys = [ko.int_key(ko.INT, v) for v in (-70000, -300, -2, -1, 0, 1, 2, 255, 256, 70000)]
    runs = ko.make_runs(ko.INT, deal(geometry()["gk_cap"] + 1, 3), seed="sum", keys=keys)
    runs = [[(key, (7 * r + i).to_bytes(4, "big")) for i, (key, _) in enumerate(run)] for r, run in enumerate(runs)]
    want = ko.fold_sum(ko.merged_records(runs, ko.INT), ko.INT, "sum.int")
    body, _ = ops.merge_runs([ko.stream(r) for r in runs], ko.INT, "gpu", kv_buf=4096, combine="sum.int",
                             key_order="hadoop")
    assert body == b"".join(record(k, v) for k, v in want) and [k for k, _ in want] == keys


# ------------------------------------------------------------------------------------------------ reduce tasks
@pytest.fixture
def provider():
    p = UdaProvider()
    yield p
    p.close()


def _publish(provider, job, runs, where="host"):
    ids = []
    for i, run in enumerate(runs):
        mid = f"attempt_{job}_m_{i:06d}_0"
        data, index = encode_partitions([ko.stream(run)])
        if where == "device":
            provider.add_mof_device(job, mid, data, index, device=0)
        else:
            provider.add_mof_memory(job, mid, data, index)
        ids.append(mid)
    return ids


@functools.lru_cache(maxsize=None)
def task_runs(cls):
    """9 map outputs of 500 records with values of 40..120 bytes (about 400 KB), keys of both signs; no two
    runs share a key, as a task numbers its map outputs in the order their fetches complete."""
    runs = ko.make_runs(cls, (500,) * 9, seed="task", vbytes=(40, 64, 90, 120), disjoint=True)
    assert all(runs) and any(ko.sortable(cls, k) < ko.SIGN for r in runs for k, _ in r)
    return runs


ROUTES = {
    "whole": ("host", {"mapred.uda.gpu.progressive.phases": 0}),
    "progressive-phases": ("host", {"mapred.uda.gpu.progressive.phases": 3}),
    "inner-rounds": ("host", {"mapred.uda.gpu.progressive.phases": 0, "mapred.uda.gpu.merge.round.bytes": 4096}),
    "device-fetch-rounds": ("device", {"mapred.uda.gpu.fetch": "device", "mapred.uda.gpu.round.bytes": 64 << 10}),
    "over-budget-hybrid": ("host", {"mapred.uda.gpu.merge.bytes": 150_000, "mapred.uda.gpu.spill": "host"}),
}


@pytest.mark.parametrize("cls", (ko.INT, ko.DOUBLE), ids=["IntWritable", "DoubleWritable"])
@pytest.mark.parametrize("route", list(ROUTES))
def test_task_routes_deliver_hadoops_order(require_gpu, provider, route, cls):
    where, extra = ROUTES[route]
    runs = task_runs(cls)
    job = "job_22_%02d%02d" % (list(ROUTES).index(route), ko.KIND[cls])
    ids = _publish(provider, job, runs, where)
    recs, st, c = run_reduce("h", job, ids, 0, cls, conf=dict(GPU_HADOOP, **extra), kv_buf_size=8192,
                             max_buf_kb=16, min_buf_kb=16)
    print({k: st.get(k) for k in ("merge_path", "merge_rounds", "rpq_rounds", "hybrid_direct", "lpqs", "bytes_fetched")})
    assert b"".join(record(k, v) for k, v in recs) == ko.oracle_merge(runs, cls)
    assert st["backend"] == "gpu" and st["key_order"] == "hadoop" and c.failure_calls == 0
    if route == "whole":
        assert st["merge_path"] == "staged" and st["merge_rounds"] == 1, st
    elif route == "progressive-phases":  # (without SDMA staging the phases are not taken: the staged task then)
        assert st["merge_path"] in ("staged-progressive", "staged"), st
    elif route == "inner-rounds":
        assert st["merge_rounds"] >= 4, st
    elif route == "device-fetch-rounds":
        assert st["merge_path"] == "device-generic" and st["rpq_rounds"] >= 3, st
    else:
        assert st["rpq_rounds"] >= 2 and (st["hybrid_direct"] == 1 or st["lpqs"] >= 2), st


def test_a_malformed_key_fails_the_task_once(require_gpu, provider):
    """A 3-byte IntWritable key in the middle of the middle run: one failure that names the class, the length
    and the map output, and nothing delivered."""
    runs = [list(r) for r in ko.make_runs(ko.INT, (300, 300, 300), seed="bad")]
    runs[1].insert(150, (b"\x00\x00\x07", b"v"))
    ids = _publish(provider, "job_22_9000", runs)
    c = UdaConsumer(len(ids), "job_22_9000", "attempt_job_22_9000_r_000000_0", ko.INT, conf=GPU_HADOOP)
    for m in ids:
        c.fetch("h", "job_22_9000", m, 0)
    with pytest.raises(UdaFallback, match=r"IntWritable key of 3 bytes \(4 expected\) in map output"):
        c.wait(60)
    c.close()
    assert c.failure_calls == 1 and c.bytes == 0


def test_a_malformed_key_fails_the_merge(require_gpu):
    runs = [list(r) for r in ko.make_runs(ko.VLONG, (200, 200, 200), seed="badv")]
    runs[1].insert(100, (b"\x8e\x01", b"v"))  # announces 3 bytes, has 2
    with pytest.raises(RuntimeError, match=r"VLongWritable key of 2 bytes .* in run 1 of the merge"):
        ops.merge_runs([ko.stream(r) for r in runs], ko.VLONG, "gpu", key_order="hadoop")
    # the merger is usable afterwards
    good = ko.make_runs(ko.VLONG, (50, 60), seed="goodv")
    body, _ = ops.merge_runs([ko.stream(r) for r in good], ko.VLONG, "gpu", key_order="hadoop")
    assert body == ko.oracle_merge(good, ko.VLONG)
