"""A failing step on the pinned-DRAM tier (where a staging thread runs beside the round loop) joins its
stager, gives its per-step events back and leaves the job usable: the next validated step computes what the
first one did. The failure is a sink's nonzero return code, a host-side error; nothing on the device goes
wrong."""
import pytest

from uda_amd.parallel.dist import DistContext

pytestmark = pytest.mark.gpu

MAPS, ROUNDS, REDUCERS = 3, 3, 2
SMALL = dict(kv_buf_bytes=64 << 10, d2h_piece_bytes=256 << 10)  # test_gpu_terasort.py's delivery geometry


def test_failed_step_leaves_the_host_store_job_usable(require_gpu):
    from uda_amd.models.terasort import TeraSortConfig, TeraSortShuffle
    cfg = TeraSortConfig(rows_per_gpu=20000 * MAPS, maps_per_rank=MAPS, rounds=ROUNDS, reducers=REDUCERS,
                         validate=True, sample_every=64, store="host", **SMALL)
    j = TeraSortShuffle(DistContext(), cfg, device=0)
    j.setup()

    first = j.step()
    j.check(first)
    assert first["validated"] and first["checksum"] == j.expected_checksum
    assert first["bytes_h2d"] == first["bytes_in"] > 0  # the staging thread moved every record
    records = list(j.job.reducer_records())
    assert sum(records) == first["records"] == 20000 * MAPS

    calls = [0] * REDUCERS

    def failing(r, b):
        calls[r] += 1
        return 7 if r == 1 and calls[1] == 2 else None

    j.use_python_sink(failing, with_reducer=True)
    with pytest.raises(RuntimeError, match="delivery sink reported error 7"):
        j.step()
    assert calls[1] >= 2

    j.drop_sink()
    third = j.step()
    j.check(third)
    assert third["validated"] and third["order_errors"] == 0
    assert third["checksum"] == first["checksum"]
    assert third["records"] == first["records"]
    assert list(j.job.reducer_records()) == records
