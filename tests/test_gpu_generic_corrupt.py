"""Corrupt and truncated runs on the GPU generic path: what a reduce task holds when a provider dies in the
middle of its answer. The contract is one clean failure ("corrupt or truncated IFile run k", which the consumer
turns into failureInUda), never a wrong stream, and the process merges on afterwards. The cases and what each
must do (fixed by the CPU merge's behaviour, tests/test_generic_cases_cpu.py) are in tests/generic_cases.py:
the broken run lies between two good ones and is about three F1 chunks long, so the parallel index walks it."""
import hashlib
import json
import os
import subprocess
import sys

import pytest

from tests import generic_cases as gc
from uda_amd import ops
from uda_amd.utils import datagen

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MESSAGE = "corrupt or truncated IFile run 1"


@pytest.fixture(scope="module")
def geo(native):
    return native.gpu_generic_geometry()


@pytest.fixture(scope="module")
def wordcount():
    """The wordcount shape of tests/test_gpu_generic.py and the oracle's merge of it."""
    streams = [s[0] for s in datagen.streams(datagen.wordcount(9, 1, 4000))]
    return streams, b"".join(gc.oracle_merge([gc.parse(s) for s in streams], gc.TEXT))


@pytest.mark.parametrize("name", list(gc.CORRUPT))
def test_corrupt_run_fails_cleanly(require_gpu, geo, wordcount, name):
    good, streams, raises = gc.corrupt_case(name, geo)
    if raises:
        with pytest.raises(RuntimeError, match=MESSAGE):
            ops.merge_runs(list(streams), gc.TEXT, "gpu")
    else:  # a run that ends on a record boundary without EOF marker is merged, as on the CPU
        body, _ = ops.merge_runs(list(streams), gc.TEXT, "gpu")
        assert body == b"".join(gc.oracle_merge(good, gc.TEXT))
        assert ops.last_stats["f1_serial_runs"] == 0 and ops.last_stats["records"] == sum(len(r) for r in good)
    # the merger cached for the device is the same one after the failure
    body, _ = ops.merge_runs(wordcount[0], gc.TEXT, "gpu")
    assert body == wordcount[1]


CHILD = """
import hashlib, json, sys
sys.path.insert(0, sys.argv[1])
import uda_amd
from tests import generic_cases as gc
from uda_amd import ops
geo = uda_amd.native().gpu_generic_geometry()
out = {}
for name in gc.CORRUPT:
    _, streams, _ = gc.corrupt_case(name, geo)
    try:
        body, _ = ops.merge_runs(list(streams), gc.TEXT, "gpu")
        out[name] = hashlib.sha256(body).hexdigest()
    except RuntimeError as e:
        out[name] = "raised: " + str(e)
print("RESULT " + json.dumps(out))
"""


def test_corrupt_runs_with_the_serial_index(require_gpu, geo):
    """The same runs under UDA_F1_SERIAL=1 (read once per process): one fresh child merges them all."""
    env = dict(os.environ, UDA_F1_SERIAL="1")
    p = subprocess.run([sys.executable, "-c", CHILD, ROOT], env=env, cwd=ROOT, timeout=240, capture_output=True,
                       text=True)
    assert p.returncode == 0, p.stderr[-2000:]
    got = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])
    for name, raises in gc.CORRUPT.items():
        good, _, _ = gc.corrupt_case(name, geo)
        if raises:
            assert got[name].startswith("raised: ") and MESSAGE in got[name], name
        else:
            assert got[name] == hashlib.sha256(b"".join(gc.oracle_merge(good, gc.TEXT))).hexdigest(), name
