"""The GPU generic merge on the boundary cases of tests/generic_cases.py against that module's pure-Python
oracle (not the CPU merge, which shares the VInt and key-offset code with the kernels): the single-pass K-way
cells and the pairwise tree (UDA_GKWAY=0), the parallel and the serial F1 index, whole and streamed in rounds,
with and without the combiner. Every merged stream must equal the oracle's byte for byte."""
import hashlib
import json
import os
import subprocess
import sys

import pytest

from tests import generic_cases as gc
from uda_amd import ops
from uda_amd.utils.ifile import J2CQueueReader

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def geo(native):
    return native.gpu_generic_geometry()


def _delivered(body, cuts, kv_buf):
    """The records a J2CQueue reads from the buffers: whole records, no buffer above kv_buf, EOF at the end."""
    r = J2CQueueReader(max_len=kv_buf)
    for b in ops.buffers(body, cuts):
        r.feed(b)
    assert r.eof
    return r


def _merge_and_check(c, kv_buf, f3):
    body, cuts = ops.merge_runs(list(c.streams), c.key_class, "gpu", kv_buf=kv_buf)
    stats = dict(ops.last_stats)
    assert body == c.expected
    assert stats["f1_serial_runs"] == c.expect["f1_serial_runs"]
    if f3 == "kway" and "passes" in c.expect:
        assert stats["passes"] == c.expect["passes"]
    if f3 == "tree" and len(c.runs) > 2:
        assert stats["passes"] > 1
    assert stats["records"] == stats["records_in"] == c.records
    assert len(_delivered(body, cuts, kv_buf).records) == c.records
    return cuts


@pytest.mark.parametrize("f3", ["kway", "tree"])
@pytest.mark.parametrize("name", gc.NAMES)
def test_case_equals_oracle(require_gpu, geo, monkeypatch, name, f3):
    if f3 == "tree":
        monkeypatch.setenv("UDA_GKWAY", "0")
    _merge_and_check(gc.case(name, geo), 1 << 20, f3)


@pytest.mark.parametrize("f3", ["kway", "tree"])
@pytest.mark.parametrize("name", ["gather-lengths-raw", "gather-lengths-text"])
def test_gather_lengths_one_record_fills_a_buffer(require_gpu, geo, monkeypatch, name, f3):
    """kv_buf = the longest record and the EOF marker: that record is a buffer of its own, filled to the last
    byte, and a cut is searched at every byte of the stream."""
    if f3 == "tree":
        monkeypatch.setenv("UDA_GKWAY", "0")
    c = gc.case(name, geo)
    cuts = _merge_and_check(c, c.longest + 2, f3)
    assert max(b - a for a, b in zip(cuts, cuts[1:])) == c.longest and len(cuts) > c.records // 2


@pytest.mark.parametrize("round_bytes", [16 << 10, 300 << 10])
@pytest.mark.parametrize("name", ["hdr-straddle", "run-lengths", "big-groups-text-one", "big-groups-text-three",
                                  "big-groups-int-one", "big-groups-int-three"])
def test_streamed_rounds_equal_oracle(require_gpu, geo, name, round_bytes):
    c = gc.case(name, geo)
    body, cuts, st = ops.merge_runs_streamed(list(c.streams), c.key_class, round_bytes=round_bytes)
    assert body == c.expected
    assert st["records"] == st["records_in"] == c.records
    assert sum(n for n, _ in st["rounds"]) == c.records
    if len(c.expected) > 4 * round_bytes:
        assert len(st["rounds"]) > 1
    # the rounds' cuts continue each other and end where the stream does
    at = 0
    for _, rc in st["rounds"]:
        assert rc[0] == at and list(rc) == sorted(rc)
        at = rc[-1]
    assert at == len(c.expected)
    assert len(_delivered(body, cuts, 1 << 20).records) == c.records


@pytest.mark.parametrize("f3", ["kway", "tree"])
@pytest.mark.parametrize("name,op", [("big-groups-int-one", "sum.int"), ("big-groups-int-three", "sum.int"),
                                     ("big-groups-text-one", "sum.vint"), ("big-groups-text-three", "sum.vint")])
def test_big_groups_combined(require_gpu, geo, monkeypatch, name, op, f3):
    """Groups longer than a cell and a tile folded on the device: the oracle's order folded in Python."""
    if f3 == "tree":
        monkeypatch.setenv("UDA_GKWAY", "0")
    c = gc.case(name, geo)
    want = gc.fold(c.merged, c.key_class, op)
    body, cuts = ops.merge_runs(list(c.streams), c.key_class, "gpu", combine=op)
    assert body == gc.stream(want, eof=False)
    assert ops.last_stats["records"] == len(want) and ops.last_stats["records_in"] == c.records
    assert _delivered(body, cuts, 1 << 20).records == want


CHILD = """
import hashlib, json, sys
sys.path.insert(0, sys.argv[1])
import uda_amd
from tests import generic_cases as gc
from uda_amd import ops
geo = uda_amd.native().gpu_generic_geometry()
out = {}
for name in sys.argv[2:]:
    c = gc.case(name, geo)
    body, _ = ops.merge_runs(list(c.streams), c.key_class, "gpu")
    out[name] = [hashlib.sha256(body).hexdigest(), ops.last_stats["records"]]
print("RESULT " + json.dumps(out))
"""


def test_serial_f1_index_in_a_child_process(require_gpu, geo):
    """UDA_F1_SERIAL=1 (every run indexed by the serial walk) is read once per process, so a fresh child merges
    the F1 cases under it and reports a hash of each merged stream."""
    names = ["hdr-straddle", "hdr-straddle-keys", "entry-edge", "run-lengths", "raw-wide-long", "raw-wide-int"]
    env = dict(os.environ, UDA_F1_SERIAL="1")
    p = subprocess.run([sys.executable, "-c", CHILD, ROOT] + names, env=env, cwd=ROOT, timeout=240,
                       capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-2000:]
    got = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])
    for name in names:
        c = gc.case(name, geo)
        assert got[name] == [hashlib.sha256(c.expected).hexdigest(), c.records], name
