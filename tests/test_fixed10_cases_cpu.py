"""CPU: the FIXED10 case generator (fixed10_cases.py), its pure-Python oracle and the project's CPU heap
merge agree byte for byte on duplicate, tied, all-ones and skewed keys. The GPU tests compare both device
merges with the same oracle (test_gpu_fixed10_keys.py)."""
import numpy as np
import pytest

from tests import fixed10_cases as fc
from uda_amd.utils import datagen


def cpu_merge(native, runs):
    out, _ = native.cpu_merge([bytes(r) + fc.EOF for r in runs], datagen.TEXT, 1 << 20)
    return out


def cpu_merge_groups(native, runs, group_first):
    gf = [0, len(runs)] if group_first is None else group_first
    out = b""
    for g0, g1 in zip(gf[:-1], gf[1:]):
        merged = cpu_merge(native, runs[g0:g1])
        assert merged.endswith(fc.EOF)
        out += merged[:-2]
    return out


def check_shape(runs):
    """Every run is whole TeraSort-shaped records in key order, and no two records of the case are equal."""
    seen = set()
    for r in runs:
        assert len(r) % fc.L == 0
        a = np.frombuffer(r, np.uint8).reshape(-1, fc.L)
        assert (a[:, 0:3] == (0x0B, 0x5B, 0x0A)).all() and (a[:, 13] == 0x5A).all()
        assert ((a[:, 14:] >= 65) & (a[:, 14:] <= 90)).all()
        keys = [rec[fc.KEY] for rec in fc.records(r)]
        assert keys == sorted(keys)
        seen.update(fc.records(r))
    assert len(seen) == sum(len(r) for r in runs) // fc.L


@pytest.mark.parametrize("name", fc.CASES)
def test_cases_cpu_merge_is_the_stable_sort(native, name):
    runs, gf = fc.case(name)
    check_shape(runs)
    want = fc.expected(name)
    assert len(want) == sum(len(r) for r in runs)
    assert cpu_merge_groups(native, runs, gf) == want


@pytest.mark.parametrize("name", ("heavy_key", "all_equal", "hi_tie", "uniform"))
def test_grouped_cases(native, name):
    runs, gf = fc.grouped(name)
    check_shape(runs)
    assert gf[2] - gf[1] == 3 and all(len(r) == 0 for r in runs[gf[1]:gf[2]])
    assert cpu_merge_groups(native, runs, list(gf)) == fc.oracle(runs, gf)


@pytest.mark.parametrize("K", fc.K_SWEEP)
@pytest.mark.parametrize("name", ("heavy_key", "identical_runs"))
def test_sweep_cases(native, name, K):
    runs, gf = fc.sweep_case(name, K)
    assert len(runs) == K and sum(len(r) for r in runs) // fc.L <= 40000
    assert cpu_merge_groups(native, runs, gf) == fc.oracle(runs, gf)


def test_case_properties():
    """What the GPU tests rely on: which cases hold a key with more copies than a cell can take."""
    copies = {name: fc.max_copies(*fc.case(name)) for name in fc.CASES}
    assert copies["all_equal"] == 15000 and copies["heavy_key"] == 6000
    assert copies["extremes"] > 2048 and copies["few_distinct"] > 2048
    for name in ("identical_runs", "disjoint_runs", "ragged", "uniform"):
        assert copies[name] == (6 if name == "identical_runs" else 1), name
    assert 24 <= copies["hi_tie"] <= 40  # 0000 and ffff, 4 per run, and chance collisions
    runs, _ = fc.case("extremes")
    keys = [rec[fc.KEY] for r in runs for rec in fc.records(r)]
    assert keys.count(fc.ZERO_KEY) > 2048 and keys.count(fc.ONES_KEY) > 2048
    runs, _ = fc.case("hi_tie")
    tails = {rec[11:13] for r in runs for rec in fc.records(r)}
    assert len({rec[3:11] for r in runs for rec in fc.records(r)}) == 1
    assert b"\x00\x00" in tails and b"\xff\xff" in tails and len(tails) > 10000
    runs, _ = fc.case("ragged")
    lens = [len(r) // fc.L for r in runs]
    assert max(lens) >= 0.9 * sum(lens) and lens.count(0) >= 3 and lens.count(1) >= 3
    assert sum(1 for n in lens if 1 < n < 5) >= 2  # shorter than half the sample step at every capacity
    runs, _ = fc.case("disjoint_runs")
    for a, b in zip(runs[:-1], runs[1:]):
        assert a[-fc.L:][fc.KEY] < b[:fc.L][fc.KEY]
