"""Configuration of the combiner's newer keys, read at INIT (no GPU needed):
mapred.uda.merge.combine.over.budget (skip | combine) and mapred.uda.gpu.merge.round.bytes."""
import pytest

from tests.combine_cases import expected_task
from uda_amd.bridge import UdaConsumer, UdaProvider, run_reduce
from uda_amd.utils import datagen
from uda_amd.utils.mof import encode_partitions

CPU = {"mapred.uda.merge.backend": "cpu", "mapred.uda.merge.combine": "sum.int"}


def _init(job, **conf):
    c = UdaConsumer(1, job, f"attempt_{job}_r_000000_0", datagen.TEXT, conf=dict(CPU, **conf))
    c.close()


def test_unknown_over_budget_value_fails_init():
    with pytest.raises(RuntimeError, match=r"mapred\.uda\.merge\.combine\.over\.budget \"always\" \(skip or combine\)"):
        _init("job_9_0001", **{"mapred.uda.merge.combine.over.budget": "always"})
    with pytest.raises(RuntimeError, match="skip or combine"):
        _init("job_9_0002", **{"mapred.uda.merge.combine.over.budget": ""})


@pytest.mark.parametrize("value", ["skip", "combine"])
def test_known_over_budget_values_pass_init(value):
    _init("job_9_001" + str(len(value)), **{"mapred.uda.merge.combine.over.budget": value})


def test_cpu_task_ignores_the_gpu_keys():
    """Both keys shape GPU merges only: a CPU task delivers what it delivers without them."""
    maps = datagen.wordcount(num_maps=4, reducers=1, words_per_map=800, seed=5)
    p = UdaProvider()
    try:
        ids = []
        for i, parts in enumerate(datagen.streams(maps)):
            mid = f"attempt_job_9_0020_m_{i:06d}_0"
            p.add_mof_memory("job_9_0020", mid, *encode_partitions(parts))
            ids.append(mid)
        conf = dict(CPU, **{"mapred.uda.merge.combine.over.budget": "combine",
                            "mapred.uda.gpu.merge.round.bytes": 1})  # below the 4 KiB minimum: clamped
        recs, st, _ = run_reduce("h", "job_9_0020", ids, 0, datagen.TEXT, conf=conf, kv_buf_size=4096)
    finally:
        p.close()
    assert recs == expected_task(maps, 0, datagen.TEXT, "sum.int") and st["combine"] == "sum.int"
