"""Delivery bit-packing (ShuffleJob delivery_pack): the consumers hand the sink the same buffers with
pack on as with pack off, over both D2H copy paths; the link carries at most 0.66 of the bytes; a
reducer without records in a round still gets exactly one EOF."""
import numpy as np
import pytest

from uda_amd.parallel.dist import DistContext

pytestmark = pytest.mark.gpu

# 78-record buffers; 256 KiB pieces: about 14 per (reducer, round) of 3.4 MB, the last one short
SHAPE = dict(rows_per_gpu=200_000, maps_per_rank=4, reducers=3, rounds=2, sample_every=64,
             kv_buf_bytes=8 << 10, d2h_piece_bytes=256 << 10)


class Collector:
    """Python sink: per reducer, the delivered bytes and every buffer's length."""

    def __init__(self, reducers):
        self.data = [bytearray() for _ in range(reducers)]
        self.lens = [[] for _ in range(reducers)]

    def __call__(self, r, b):
        self.data[r] += b
        self.lens[r].append(len(b))


def _run(delivery_pack, d2h, validate=False, bounds_fn=None, **kw):
    from uda_amd.models.terasort import TeraSortConfig, TeraSortShuffle
    cfg = TeraSortConfig(**{**SHAPE, **kw}, delivery_pack=delivery_pack, d2h=d2h, validate=validate,
                         check_delivery=validate)
    j = TeraSortShuffle(DistContext(), cfg, device=0)
    j.setup(bounds_fn=bounds_fn)
    sink = Collector(cfg.reducers)
    j.use_python_sink(sink, with_reducer=True)
    st = j.step(validate=validate)
    j.check(st)
    return j, st, sink


@pytest.fixture(scope="module")
def unpacked(require_gpu):
    """The reference streams: pack off, computed once (the data depends on the seed alone)."""
    j, st, sink = _run("off", "sdma")
    assert st["packed_pieces"] == 0 and st["raw_pieces"] > 0
    assert st["d2h_bytes"] == st["bytes_in"]
    assert "pack=off" in j.job.delivery_name
    return sink


@pytest.mark.parametrize("d2h", ["sdma", "hip"])
def test_packed_delivery_hands_over_the_same_buffers(require_gpu, unpacked, d2h):
    j, st, sink = _run("auto", d2h, validate=True)
    assert st["validated"] and st["delivery_errors"] == 0 and st["pre_d2h_errors"] == 0
    for r in range(SHAPE["reducers"]):
        assert sink.lens[r] == unpacked.lens[r]
        assert bytes(sink.data[r]) == bytes(unpacked.data[r])
        assert sink.data[r][-2:] == b"\xff\xff"
    assert sum(len(d) for d in sink.data) == st["bytes_in"] + 2 * SHAPE["reducers"]
    # every (reducer, round) has several pieces and a short last one
    assert st["packed_pieces"] >= 3 * SHAPE["reducers"] * SHAPE["rounds"]
    assert st["raw_pieces"] == 0
    print(f"d2h_bytes / bytes_in = {st['d2h_bytes'] / st['bytes_in']:.4f}, unpack_ms = {st['unpack_ms']:.2f}")
    assert st["d2h_bytes"] <= 0.66 * st["bytes_in"]
    name = j.job.delivery_name
    assert name.startswith(d2h) and "pack=colbits" in name and f"d2h/in={st['d2h_bytes'] / st['bytes_in']:.3f}" in name


def test_pack_off_over_hip_matches_too(require_gpu, unpacked):
    _, st, sink = _run("off", "hip")
    assert st["packed_pieces"] == 0
    for r in range(SHAPE["reducers"]):
        assert sink.lens[r] == unpacked.lens[r] and bytes(sink.data[r]) == bytes(unpacked.data[r])


def test_environment_switch_forces_pack_off(require_gpu, monkeypatch):
    monkeypatch.setenv("UDA_DELIVERY_PACK", "0")
    j, st, _ = _run("auto", "sdma", rows_per_gpu=20_000)
    assert st["packed_pieces"] == 0 and "pack=off" in j.job.delivery_name


def test_reducer_without_records_in_a_round_gets_one_eof(require_gpu):
    """Cells (reducer 0, round 0), (reducer 1, round 1) and (reducer 2, round 1) are empty: an empty
    first round, an empty final round after data, and a final round whose EOF travels alone."""
    from uda_amd.parallel.plan import round_bounds

    def bounds_with_empty_cells(per_dest, cells):
        b = round_bounds(per_dest, cells).copy()  # (1, 5, 2): cell c = [bound c-1, bound c), c = reducer * 2 + round
        b[0, 0] = 0
        b[0, 3] = b[0, 2]
        b[0, 4] = (np.uint64(0xFFFFFFFFFFFFFFFF), np.uint64(0xFFFF) << np.uint64(48))
        return b

    j, st, sink = _run("auto", "sdma", validate=True, bounds_fn=bounds_with_empty_cells, rows_per_gpu=60_000)
    from uda_amd.utils.ifile import J2CQueueReader
    recs = list(j.job.reducer_records())
    assert all(n > 0 for n in recs)
    for r in range(SHAPE["reducers"]):
        data = bytes(sink.data[r])
        assert len(data) == recs[r] * 104 + 2 and data[-2:] == b"\xff\xff"
        reader = J2CQueueReader(max_len=8 << 10)  # raises on a second EOF or bytes after the first
        pos = 0
        for n in sink.lens[r]:
            reader.feed(data[pos:pos + n])
            pos += n
        assert reader.eof and len(reader.records) == recs[r]
    assert st["raw_pieces"] == 0 and st["delivery_errors"] == 0
