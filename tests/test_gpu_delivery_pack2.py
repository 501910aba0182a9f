"""Delivery bit-packing with colpack version 2 (ShuffleJob delivery_pack="auto"): over both D2H copy
paths the sink receives the same buffers as with pack off, every packed piece is a delta piece, and
the link carries fewer bytes than with version 1 ("v1") on the same shape, which still delivers the
same streams."""
import pytest

from tests.test_gpu_delivery_pack import SHAPE, _run

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def unpacked(require_gpu):
    """The reference streams: pack off, computed once."""
    _, st, sink = _run("off", "sdma")
    assert st["packed_pieces"] == 0 and st["pack_delta_pieces"] == 0
    return sink


@pytest.fixture(scope="module")
def v1_run(require_gpu):
    """Version 1 on the same shape: the reference for d2h_bytes."""
    j, st, sink = _run("v1", "sdma", validate=True)
    return j.job.delivery_name, st, sink


def _same_streams(sink, ref):
    for r in range(SHAPE["reducers"]):
        assert sink.lens[r] == ref.lens[r]
        assert bytes(sink.data[r]) == bytes(ref.data[r])


def test_v1_still_delivers_the_same_streams(require_gpu, unpacked, v1_run):
    name, st, sink = v1_run
    assert st["validated"] and st["delivery_errors"] == 0 and st["pre_d2h_errors"] == 0
    _same_streams(sink, unpacked)
    assert st["raw_pieces"] == 0 and st["packed_pieces"] > 0 and st["pack_delta_pieces"] == 0
    assert "pack=colbits v1" in name and "plain" in name


@pytest.mark.parametrize("d2h", ["sdma", "hip"])
def test_v2_delivery_hands_over_the_same_buffers_in_fewer_bytes(require_gpu, unpacked, v1_run, d2h):
    j, st, sink = _run("auto", d2h, validate=True)
    assert st["validated"] and st["delivery_errors"] == 0 and st["pre_d2h_errors"] == 0
    _same_streams(sink, unpacked)
    assert st["raw_pieces"] == 0
    assert st["packed_pieces"] >= 3 * SHAPE["reducers"] * SHAPE["rounds"]
    assert st["pack_delta_pieces"] == st["packed_pieces"]
    v1 = v1_run[1]
    print(f"d2h_bytes v2 {st['d2h_bytes']} v1 {v1['d2h_bytes']} of {st['bytes_in']}; "
          f"stride {st['pack_stride_min']}..{st['pack_stride_max']} (v1 {v1['pack_stride_min']}..{v1['pack_stride_max']})")
    assert st["bytes_in"] == v1["bytes_in"] and st["packed_pieces"] == v1["packed_pieces"]
    assert st["d2h_bytes"] < v1["d2h_bytes"]
    assert 0 < st["pack_stride_min"] <= st["pack_stride_max"] < v1["pack_stride_max"]
    name = j.job.delivery_name
    assert "pack=colbits v2 delta" in name and f"d2h/in={st['d2h_bytes'] / st['bytes_in']:.3f}" in name


def test_unknown_delivery_pack_value_throws(require_gpu):
    with pytest.raises(Exception, match="delivery_pack"):
        _run("v3", "sdma", rows_per_gpu=20_000)
