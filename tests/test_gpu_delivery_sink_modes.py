"""What ShuffleJob's consumers make of the job's sink, with delivery_pack on and off. Without a sink the
pieces are still checked and their buffers counted, nothing is unpacked, and a check_delivery step still
checksums what would have been delivered. A sink that returns nonzero fails that step with its code and
leaves the delivery threads running: the next step delivers everything again."""
import pytest

from tests.test_gpu_delivery_pack import SHAPE, Collector
from uda_amd.parallel.dist import DistContext

pytestmark = pytest.mark.gpu

ROWS = 60_000


def _job(delivery_pack):
    from uda_amd.models.terasort import TeraSortConfig, TeraSortShuffle
    cfg = TeraSortConfig(**{**SHAPE, "rows_per_gpu": ROWS}, delivery_pack=delivery_pack, check_delivery=True)
    j = TeraSortShuffle(DistContext(), cfg, device=0)
    j.setup()
    return j


def _collect(j):
    sink = Collector(SHAPE["reducers"])
    j.use_python_sink(sink, with_reducer=True)
    st = j.step()
    j.check(st)
    return st, sink


@pytest.fixture(scope="module", params=["auto", "off"])
def fresh(request, require_gpu):
    """A fresh job's step into a Collector: (delivery_pack, its stats, the sink)."""
    st, sink = _collect(_job(request.param))
    assert (st["packed_pieces"] > 0) == (request.param == "auto")
    return request.param, st, sink


def test_without_a_sink_pieces_are_counted_not_unpacked(fresh):
    pack, want, _ = fresh
    j = _job(pack)
    j.drop_sink()
    st = j.step()
    j.check(st)
    print({k: st[k] for k in ("buffers", "d2h_bytes", "packed_pieces", "unpack_ms")})
    for k in ("buffers", "d2h_bytes", "packed_pieces"):
        assert st[k] == want[k], k
    assert st["unpack_ms"] == 0
    # the delivery checksum does not need a sink
    st = j.step(validate=True)
    j.check(st)
    assert st["validated"] and st["delivery_errors"] == 0
    assert st["buffers"] == want["buffers"]


def test_sink_error_fails_the_step_and_the_next_one_delivers(fresh):
    pack, _, want = fresh
    j = _job(pack)
    calls = [0] * SHAPE["reducers"]

    def failing(r, b):
        calls[r] += 1
        return 7 if r == 1 and calls[1] == 2 else None

    j.use_python_sink(failing, with_reducer=True)
    with pytest.raises(RuntimeError, match="delivery sink reported error 7"):
        j.step()
    assert calls[1] >= 2 and calls[0] == len(want.lens[0]) and calls[2] == len(want.lens[2])
    _, sink = _collect(j)
    for r in range(SHAPE["reducers"]):
        assert sink.lens[r] == want.lens[r]
        assert bytes(sink.data[r]) == bytes(want.data[r])
