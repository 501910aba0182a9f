"""The combiner's further ops on the device (csrc/gpu/combine.hip: min / max over an order-preserving image,
sums of one VInt / VLong with the record re-encoded in the gather): the GPU merge under
mapred.uda.merge.combine = min.int, max.int, min.long, max.long, sum.vint, sum.vlong must deliver, byte for
byte, what the CPU backend and the pure-Python oracle of tests/combine_ops_cases.py deliver."""
import pytest

import uda_amd
from tests.combine_ops_cases import BAD_VALUES, bad_value_runs, ops_cases, oracle
from uda_amd import ops
from uda_amd.utils import datagen
from uda_amd.utils.ifile import J2CQueueReader, decode_stream, encode_stream, text, vint_encode

pytestmark = pytest.mark.gpu
TILE = uda_amd.native().combine_tile()  # the segmented fold's elements per workgroup: the group lengths are built on it
CASES = list(ops_cases(TILE))


def _check(runs, key_class, op, kv_buf):
    want = oracle(runs, key_class, op)
    g_body, g_cuts = ops.merge_runs(runs, key_class, "gpu", kv_buf=kv_buf, combine=op)
    stats = dict(ops.last_stats)
    c_body, _ = ops.merge_runs(runs, key_class, "cpu", kv_buf=kv_buf, combine=op)
    assert c_body == want
    assert g_body == want
    assert all(b - a <= kv_buf - 2 for a, b in zip(g_cuts[:-1], g_cuts[1:]))  # (2: the EOF marker's room)
    r = J2CQueueReader(max_len=kv_buf)
    for b in ops.buffers(g_body, g_cuts):
        r.feed(b)
    assert r.eof and encode_stream(r.records, eof=False) == want
    assert stats["records"] == len(r.records)
    return stats, r.records


@pytest.mark.parametrize("name,key_class,op,runs", CASES, ids=[c[0] for c in CASES])
def test_gpu_combine_op_matches_cpu_and_oracle(require_gpu, name, key_class, op, runs):
    for kv_buf in (4096, 256):
        st, recs = _check(runs, key_class, op, kv_buf)
    records_in = sum(len(decode_stream(r, require_eof=False)) for r in runs)
    assert st["records_in"] == records_in
    if name.startswith("short-heads"):
        assert recs[-1][1] == vint_encode(381) and len(recs[-1][1]) == 3
    if name.startswith("non-canonical"):
        assert (text(b"only"), b"\x05") in recs and (text(b"a"), b"\x06") in recs
    if name == "all-distinct-sum.vint":  # canonical values, no two keys equal: the plain merge, byte for byte
        assert st["records"] == records_in == 6000
        assert ops.merge_runs(runs, key_class, "gpu", combine=op) == ops.merge_runs(runs, key_class, "gpu")


def test_gpu_combine_op_pairwise_tree(require_gpu, monkeypatch):
    """The pairwise merge tree (no single-pass K-way) leaves the same order for the combiner."""
    monkeypatch.setenv("UDA_GKWAY", "0")
    for name in ("length-steps-grow-sum.vlong", "signs-min.int"):
        _, key_class, op, runs = next(c for c in CASES if c[0] == name)
        _check(runs, key_class, op, 4096)


@pytest.mark.parametrize("name", list(BAD_VALUES))
def test_gpu_combine_op_refuses_the_value(require_gpu, name):
    op, bad, says = BAD_VALUES[name]
    runs = bad_value_runs(op, bad)
    with pytest.raises(RuntimeError, match=says):
        ops.merge_runs(runs, datagen.TEXT, "gpu", combine=op)
    # the merger is as good as before: the same runs without the bad record
    good = [runs[0], encode_stream(decode_stream(runs[1])[:1])]
    st, _ = _check(good, datagen.TEXT, op, 4096)
    assert st["records"] == 300 and st["records_in"] == 301
