"""mapred.uda.ifile.checksum.over.budget (skip | verify), read at INIT (no GPU needed): what the over-budget
GPU hybrid does with the IFile checksum trailers. A CPU task, and a task within the device budget, never
look at it."""
import pytest

from uda_amd.bridge import UdaConsumer, UdaProvider, run_reduce
from uda_amd.utils import datagen
from uda_amd.utils.mof import encode_partitions

CPU = {"mapred.uda.merge.backend": "cpu"}
KEY = "mapred.uda.ifile.checksum.over.budget"


def _init(job, **conf):
    c = UdaConsumer(1, job, f"attempt_{job}_r_000000_0", datagen.TEXT, conf=dict(CPU, **conf))
    c.close()


def test_unknown_over_budget_value_fails_init():
    with pytest.raises(RuntimeError, match=r"mapred\.uda\.ifile\.checksum\.over\.budget \"always\" \(skip or verify\)"):
        _init("job_9_0101", **{KEY: "always"})
    with pytest.raises(RuntimeError, match="skip or verify"):
        _init("job_9_0102", **{KEY: ""})
    with pytest.raises(RuntimeError, match="skip or verify"):  # (also under off, where it has no effect)
        _init("job_9_0103", **{KEY: "auto", "mapred.uda.ifile.checksum": "off"})


@pytest.mark.parametrize("value", ["skip", "verify"])
def test_known_over_budget_values_pass_init(value):
    _init("job_9_011" + str(len(value)), **{KEY: value})


@pytest.mark.parametrize("value", ["skip", "verify"])
def test_cpu_task_verifies_whatever_the_key_says(value):
    maps = datagen.wordcount(num_maps=4, reducers=1, words_per_map=800, seed=7)
    job = "job_9_012" + str(len(value))
    p = UdaProvider()
    try:
        ids = []
        for i, parts in enumerate(datagen.streams(maps)):
            mid = f"attempt_{job}_m_{i:06d}_0"
            p.add_mof_memory(job, mid, *encode_partitions(parts, None, checksum=True))
            ids.append(mid)
        recs, st, _ = run_reduce("h", job, ids, 0, datagen.TEXT, conf=dict(CPU, **{KEY: value}), kv_buf_size=4096)
    finally:
        p.close()
    assert len(recs) == sum(len(m[0]) for m in maps)
    assert st["ifile_checksum"] == "verified" and st["checksum_partitions"] == 4, st
