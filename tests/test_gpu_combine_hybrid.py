"""The over-budget GPU hybrid under mapred.uda.merge.combine.over.budget=combine (gpu_merge_staged.cc): every
RPQ round combines (the host planner never splits equal keys between rounds), and so do the LPQ merges, so
the spills hold one record per key of their group. The task delivers what the oracle delivers; with the
key absent or `skip` it behaves as before (tests/test_gpu_combine.py::test_task_over_budget_skips_the_combiner).

The combined spills of the two LPQ configurations (about 117 000 of 417 350 bytes fetched) would fit one RPQ
round of the budget; they are sampled finely and planned in at least two rounds, so these configurations
too run several combining rounds."""
import pytest

import uda_amd
from tests.combine_cases import combine_records, expected_task
from uda_amd.bridge import UdaProvider, run_reduce
from uda_amd.utils import datagen
from uda_amd.utils.ifile import encode_stream
from uda_amd.utils.mof import encode_partitions

pytestmark = pytest.mark.gpu
BUDGET = 400_000
CONF = {"mapred.uda.merge.backend": "gpu", "mapred.uda.merge.combine": "sum.int",
        "mapred.uda.merge.combine.over.budget": "combine", "mapred.uda.gpu.merge.bytes": BUDGET,
        "mapred.uda.gpu.spill": "host"}
CONFIGS = {
    "progressive-direct": {},
    "direct": {"mapred.uda.gpu.hybrid.progressive": 0},
    "lpq-host": {"mapred.uda.gpu.hybrid.direct": 0},
    "lpq-disk": {"mapred.uda.gpu.spill": "disk"},
}


@pytest.fixture(scope="module")
def maps():
    return datagen.wordcount(num_maps=12, reducers=1, words_per_map=12000, seed=37)


@pytest.fixture(scope="module")
def want(maps):
    return expected_task(maps, 0, datagen.TEXT, "sum.int")


@pytest.fixture
def provider():
    p = UdaProvider()
    yield p
    p.close()


@pytest.mark.parametrize("name", list(CONFIGS))
def test_over_budget_task_combines(require_gpu, provider, tmp_path, maps, want, name):
    job = "job_9_05%02d" % len(name)
    ids = []
    for i, parts in enumerate(datagen.streams(maps)):
        mid = f"attempt_{job}_m_{i:06d}_0"
        provider.add_mof_memory(job, mid, *encode_partitions(parts, None, block_size=64 << 10))
        ids.append(mid)
    kw = dict(local_dirs=(str(tmp_path),)) if name == "lpq-disk" else {}
    recs, st, c = run_reduce("h", job, ids, 0, datagen.TEXT, conf=dict(CONF, **CONFIGS[name]), kv_buf_size=8192, **kw)
    assert recs == want
    assert st["combine"] == "sum.int", st
    assert st["combine_groups"] == st["records"] == len(want)
    assert st["combine_in_records"] == sum(len(m[0]) for m in maps)
    assert st["bytes_fetched"] > BUDGET, st
    print({k: st[k] for k in ("merge_path", "lpqs", "spill_bytes", "rpq_rounds", "bytes_fetched", "bytes_delivered")})
    assert st["bytes_delivered"] == len(encode_stream(want)) == c.bytes
    assert uda_amd.native().hbm_stats(0)["over"] == 0  # hbm_over_budget_bytes of the bench JSON
    if name == "progressive-direct":
        assert st["merge_path"] == "staged-progressive-direct", st
    if name == "direct":
        assert st["hybrid_direct"] == 1 and st["lpqs"] == 0, st
    if name.startswith("lpq"):
        assert st["lpqs"] >= 2 and st["hybrid_direct"] == 0, st
        # An LPQ spill is its group's combined stream. Which maps share a group depends on the order the
        # fetches complete in, so the bound is one that holds for every grouping: a group's combined size is
        # at most the combined sizes of its maps taken alone, and at most the whole task's combined size.
        size = lambda recs_: len(encode_stream(recs_, eof=False))  # noqa: E731
        kf = datagen.sort_key(datagen.TEXT)
        alone = sum(size(combine_records(sorted(m[0], key=kf), datagen.TEXT, "sum.int")) for m in maps)
        bound = min(alone, st["lpqs"] * size(want))
        assert size(want) <= st["spill_bytes"] <= bound < st["bytes_fetched"], (st["spill_bytes"], bound, st)
    assert st["rpq_rounds"] > 1, st["rpq_rounds"]
