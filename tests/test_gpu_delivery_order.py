"""Delivery order (ShuffleJob delivery_order): issuing a round's D2H pieces wave by wave hands every
reducer's consumer the same buffers as issuing them reducer by reducer, over both copy paths, packed and
not, with fewer ring slots than reducers, in a validated step, and with uneven cells (a reducer empty in
round 0, one empty in the last round, one holding most of the data). The link-occupancy stats of every
step are consistent: none negative, and lead-in + idle + tail fit into the step's wall time."""
import numpy as np
import pytest

from tests.test_gpu_delivery_pack import SHAPE, Collector
from uda_amd.parallel.dist import DistContext

pytestmark = pytest.mark.gpu

RECORD = 104


def _run(order, validate=False, **kw):
    from uda_amd.models.terasort import TeraSortConfig, TeraSortShuffle
    cfg = TeraSortConfig(**{**SHAPE, **kw}, delivery_order=order, validate=validate, check_delivery=validate)
    j = TeraSortShuffle(DistContext(), cfg, device=0)
    j.setup()
    sink = Collector(cfg.reducers)
    j.use_python_sink(sink, with_reducer=True)
    st = j.step(validate=validate)
    j.check(st)
    return j, st, sink


def _check_stats(st):
    print({k: round(st[k], 3) for k in ("lead_in_ms", "link_idle_ms", "tail_ms", "slot_wait_ms", "wall_ms")})
    assert st["lead_in_ms"] >= 0 and st["link_idle_ms"] >= 0 and st["tail_ms"] >= 0 and st["slot_wait_ms"] >= 0
    assert st["lead_in_ms"] + st["link_idle_ms"] + st["tail_ms"] <= st["wall_ms"]


def _same_streams(validate=False, **kw):
    """One step in each order under the same settings; returns both runs as (job, stats, sink)."""
    ref = _run("reducer", validate=validate, **kw)
    got = _run("wave", validate=validate, **kw)
    assert "order=reducer" in ref[0].job.delivery_name and "order=wave" in got[0].job.delivery_name
    recs = list(got[0].job.reducer_records())
    assert recs == list(ref[0].job.reducer_records())
    for r in range(SHAPE["reducers"]):
        assert got[2].lens[r] == ref[2].lens[r]
        assert bytes(got[2].data[r]) == bytes(ref[2].data[r])
        # one EOF, at the very end: the records account for every other byte
        assert len(got[2].data[r]) == recs[r] * RECORD + 2 and got[2].data[r][-2:] == b"\xff\xff"
    for _, st, _ in (ref, got):
        assert st["packed_pieces"] + st["raw_pieces"] >= 3 * SHAPE["reducers"] * SHAPE["rounds"]
        _check_stats(st)
    assert got[1]["packed_pieces"] == ref[1]["packed_pieces"] and got[1]["raw_pieces"] == ref[1]["raw_pieces"]
    assert got[1]["d2h_bytes"] == ref[1]["d2h_bytes"]
    return ref, got


@pytest.mark.parametrize("d2h", ["sdma", "hip"])
@pytest.mark.parametrize("pack", ["auto", "off"])
def test_wave_order_delivers_the_same_streams(require_gpu, pack, d2h):
    _, (j, st, _) = _same_streams(delivery_pack=pack, d2h=d2h)
    assert (st["raw_pieces"] == 0) if pack == "auto" else (st["packed_pieces"] == 0)
    assert j.job.delivery_name.startswith(d2h)


@pytest.mark.parametrize("slots", [2, 16])
def test_fewer_ring_slots_than_reducers(require_gpu, slots):
    """2 slots for 3 reducers: a wave does not fit into the ring; slots are taken in issue order."""
    _same_streams(pinned_slots=slots)


def test_validated_step(require_gpu):
    ref, got = _same_streams(validate=True)
    for _, st, _ in (ref, got):
        assert st["validated"] and st["delivery_errors"] == 0 and st["pre_d2h_errors"] == 0
    assert got[1]["checksum"] == ref[1]["checksum"]


def test_uneven_cells(require_gpu, monkeypatch):
    """Cell c = reducer * 2 + round. Reducer 0 is empty in round 0 and has a sixth of the data in round 1;
    reducer 1 has two thirds of it, a third per round (twice the pieces of anyone else: the late waves are
    its alone); reducer 2 has a sixth in round 0 and nothing in the last round, so its EOF travels alone."""
    import uda_amd.models.terasort as ts
    orig = ts.round_bounds

    def uneven_bounds(per_dest, cells):
        s = orig(per_dest, cells)  # (1, 5, 2): the sextiles
        b = s.copy()
        b[0, 0] = 0
        b[0, 1] = s[0, 0]
        b[0, 2] = s[0, 2]
        b[0, 3] = s[0, 4]
        b[0, 4] = (np.uint64(0xFFFFFFFFFFFFFFFF), np.uint64(0xFFFF) << np.uint64(48))
        return b

    monkeypatch.setattr(ts, "round_bounds", uneven_bounds)
    ref, got = _same_streams(validate=True)
    recs = list(got[0].job.reducer_records())
    total = sum(recs)
    assert all(n > 0 for n in recs) and recs[1] > 0.6 * total and recs[0] < 0.2 * total and recs[2] < 0.2 * total
    from uda_amd.utils.ifile import J2CQueueReader
    for r in range(SHAPE["reducers"]):
        reader = J2CQueueReader(max_len=SHAPE["kv_buf_bytes"])  # raises on a second EOF or bytes after the first
        data, pos = bytes(got[2].data[r]), 0
        for n in got[2].lens[r]:
            reader.feed(data[pos:pos + n])
            pos += n
        assert reader.eof and len(reader.records) == recs[r]
    for _, st, _ in (ref, got):
        assert st["delivery_errors"] == 0 and st["pre_d2h_errors"] == 0
