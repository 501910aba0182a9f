"""GPU: the FIXED10 merge paths on duplicate, tied, all-ones and skewed keys (tests/fixed10_cases.py).

Every comparison is byte equality with the Python stable sort of the runs (key, then run, then position).
native.gpu_merge_fixed builds a DeviceMerger per call, so the UDA_KWAY* environment of each test applies;
its overflow_cells says how many cells the wave-level priority queue of kway.hip merged, which proves
that path ran on its natural input (a key with more copies than a cell holds) and did not run where the
planner's bound (target + runs * step <= capacity) says it cannot."""
import functools

import numpy as np
import pytest

from tests import fixed10_cases as fc
from uda_amd.bridge import UdaProvider, run_reduce
from uda_amd.utils import datagen
from uda_amd.utils.mof import encode_partitions

pytestmark = pytest.mark.gpu
L = fc.L
EOF = fc.EOF
KWAY_ENV = ("UDA_KWAY", "UDA_KWAY_CAP", "UDA_KWAY_STAGED", "UDA_KWAY_TARGET", "UDA_KWAY_FILL")
# name -> (environment, pad, cell capacity in force; None: the pairwise tree)
VARIANTS = {
    "default": ({}, 0, 2048),
    "tree": ({"UDA_KWAY": "0"}, 0, None),
    "cap512": ({"UDA_KWAY_CAP": "512"}, 0, 512),
    "staged": ({"UDA_KWAY_STAGED": "1"}, 0, 1024),
    "staged-pad8": ({"UDA_KWAY_STAGED": "1"}, 8, 1024),
    "pad2": ({}, 2, 2048),
    "staged-pad2": ({"UDA_KWAY_STAGED": "1"}, 2, 1024),  # unaligned runs: the plain kernel at the staged capacity
}
NEVER_OVERFLOW = ("uniform", "disjoint_runs", "identical_runs")
GPU = {"mapred.uda.merge.backend": "gpu"}
CPU = {"mapred.uda.merge.backend": "cpu"}
KV = 8192
PIECE = 32 << 10
MODES = ("auto", "v1", "off")


def set_env(monkeypatch, env):
    for k in KWAY_ENV:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def log2_ceil(k):
    return (k - 1).bit_length()


def overflow_expected(name, copies, K, cap):
    """True: some cell must take the priority queue (a key has more copies than a cell holds, and equal
    keys share a cell). False: none can (distinct-key cases by the planner's bound; others when the bound
    plus every copy of the most frequent key still fits). None: the case decides nothing."""
    if copies > cap:
        return True
    if name in NEVER_OVERFLOW:
        return False
    target = cap * 65 // 100
    step = max(1, (cap - target) // (K + 2))
    return False if target + K * step + copies <= cap else None


def merge_and_check(native, monkeypatch, name, runs, gf, want, variant, kmax=None):
    env, pad, cap = VARIANTS[variant]
    set_env(monkeypatch, env)
    out, st = native.gpu_merge_fixed(list(runs), None if gf is None else list(gf), 0, pad)
    assert len(out) == len(want)
    assert out == want, f"{name} {variant}: first difference in record {first_difference(out, want)}"
    assert st["bad_layout"] is False
    kmax = len(runs) if kmax is None else kmax
    if cap is None or kmax > 256:
        assert st["passes"] == log2_ceil(kmax) and st["overflow_cells"] == 0, st
        assert st["kway"] is (cap is not None)
        return st
    assert st["kway"] is True and st["passes"] == 1, st
    expect = overflow_expected(name, fc.max_copies(runs, gf), kmax, cap)
    if expect is True:
        assert st["overflow_cells"] > 0, st
    elif expect is False:
        assert st["overflow_cells"] == 0, st
    return st


def first_difference(a, b):
    for i in range(0, min(len(a), len(b)), L):
        if a[i:i + L] != b[i:i + L]:
            return i // L
    return min(len(a), len(b)) // L


@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("name", fc.CASES)
def test_merge_variants(require_gpu, native, monkeypatch, name, variant):
    runs, gf = fc.case(name)
    merge_and_check(native, monkeypatch, name, runs, gf, fc.expected(name), variant)


def test_case_table_covers_both_overflow_answers():
    """The path proof above is not vacuous: at every capacity some cases must overflow and the others
    cannot, and no case of the default shape is undecided."""
    for cap in (512, 1024, 2048):
        got = {name: overflow_expected(name, fc.max_copies(*fc.case(name)), len(fc.case(name)[0]), cap)
               for name in fc.CASES}
        assert {n for n, v in got.items() if v is True} == {"all_equal", "few_distinct", "extremes", "heavy_key"}, got
        assert {n for n, v in got.items() if v is False} == {"hi_tie", "identical_runs", "disjoint_runs", "ragged",
                                                             "uniform"}, got


@pytest.mark.parametrize("staged", [False, True])
def test_forced_target_sends_every_cell_through_the_queue(require_gpu, native, monkeypatch, staged):
    """UDA_KWAY_TARGET=5000 plans cells of 5000 distinct keys, above every capacity: the overflow count is
    the planned cell count."""
    runs, _ = fc.case("uniform")
    set_env(monkeypatch, {"UDA_KWAY_TARGET": "5000", **({"UDA_KWAY_STAGED": "1"} if staged else {})})
    out, st = native.gpu_merge_fixed(list(runs))
    assert out == fc.expected("uniform") and st["bad_layout"] is False
    total = sum(len(r) for r in runs) // L
    assert st["passes"] == 1 and st["overflow_cells"] == -(-total // 5000) == 3, st


@pytest.mark.parametrize("K", fc.K_SWEEP)
@pytest.mark.parametrize("name", ("heavy_key", "identical_runs"))
def test_k_sweep(require_gpu, native, monkeypatch, name, K):
    """1 pass up to 256 runs, the 9-pass tree at 257. heavy_key at 130 and 256 runs puts a key with more
    copies than a cell into the priority queue's lanes of several slices each."""
    runs, gf = fc.sweep_case(name, K)
    st = merge_and_check(native, monkeypatch, name, runs, gf, fc.oracle(runs, gf), "default")
    assert st["passes"] == (9 if K == 257 else 1)
    if name == "heavy_key" and 6 <= K <= 256:
        assert fc.max_copies(runs) > 2048 and st["overflow_cells"] > 0, st


@pytest.mark.parametrize("variant", ("cap512", "staged-pad8"))
@pytest.mark.parametrize("K", (130, 256))
def test_many_slices_per_lane_other_kernels(require_gpu, native, monkeypatch, K, variant):
    runs, gf = fc.sweep_case("heavy_key", K)
    st = merge_and_check(native, monkeypatch, "heavy_key", runs, gf, fc.oracle(runs, gf), variant)
    assert st["overflow_cells"] > 0


@functools.lru_cache(maxsize=None)
def _grouped_want(name):
    return fc.oracle(*fc.grouped(name))


@pytest.mark.parametrize("variant", ("default", "tree", "cap512", "staged-pad8", "pad2"))
@pytest.mark.parametrize("name", ("heavy_key", "all_equal", "hi_tie", "uniform"))
def test_groups(require_gpu, native, monkeypatch, name, variant):
    """A group of one run, a group whose runs are all empty (it contributes nothing and shifts nothing),
    and the named case: the per-group oracles back to back."""
    runs, gf = fc.grouped(name)
    merge_and_check(native, monkeypatch, name, runs, gf, _grouped_want(name), variant, kmax=6)


def test_nothing_and_single_records(require_gpu, native, monkeypatch):
    set_env(monkeypatch, {})
    out, st = native.gpu_merge_fixed([])
    assert out == b"" and st["passes"] == 0 and st["overflow_cells"] == 0
    out, st = native.gpu_merge_fixed([b"", b""], [0, 1, 2])
    assert out == b"" and st["passes"] == 0
    one = fc.case("uniform")[0][0][:L]
    for pad in (0, 8, 2):
        out, st = native.gpu_merge_fixed([b"", one, b""], None, 0, pad)
        assert out == one and st["passes"] == 1 and st["bad_layout"] is False


@pytest.mark.parametrize("variant", ("default", "staged", "staged-pad8"))
@pytest.mark.parametrize("name", ("heavy_key", "ragged", "extremes"))
def test_no_write_past_the_buffers(require_gpu, native, monkeypatch, name, variant):
    """UDA_DEVICE_GUARD=1: the input, the output and every buffer of the merger carry a guard tail that is
    checked when the call frees them."""
    runs, gf = fc.case(name)
    before = native.device_guard_violations()
    monkeypatch.setenv("UDA_DEVICE_GUARD", "1")
    merge_and_check(native, monkeypatch, name, runs, gf, fc.expected(name), variant)
    assert native.device_guard_violations() == before


# ---------------------------------------------------------------- device_reduce_fixed: key-range rounds

ROUND_BYTES = 260_000


@pytest.mark.parametrize("name", ("all_equal", "heavy_key", "hi_tie", "extremes", "ragged"))
def test_device_reduce_rounds(require_gpu, native, monkeypatch, name):
    """Round bounds are quantiles of a key sample: with duplicated keys several bounds coincide, rounds in
    front of them are empty (delivered with 0 records) and one round holds far more than round_bytes."""
    set_env(monkeypatch, {})
    runs = list(fc.case(name)[0])
    total = sum(len(r) for r in runs)
    Q = -(-total // ROUND_BYTES)
    assert 4 <= Q <= 8
    over = native.hbm_stats(0)["over"]
    res = {m: native.gpu_device_reduce_fixed(runs, KV, ROUND_BYTES, PIECE, m, 0) for m in MODES}
    first = res[MODES[0]][0]
    want = fc.expected(name)
    for m in MODES:
        bufs, st = res[m]
        assert bufs == first, m
        assert st["rounds"] == Q and st["bytes"] == total and st["records"] == total // L, st
        assert st["buffers"] == len(bufs) and st["pieces"] == st["packed_pieces"] + st["raw_pieces"], st
        assert all(0 < len(b) <= KV for b in bufs)
    joined = b"".join(first)
    assert joined == want + EOF
    # whole records in every buffer, and the one EOF marker closes the last
    assert all(len(b) % L == 0 for b in first[:-1]) and len(first[-1]) % L == 2 and first[-1].endswith(EOF)
    assert native.hbm_stats(0)["over"] == over
    off = res["off"][1]
    assert off["d2h_bytes"] == total and off["packed_pieces"] == 0, off


# ---------------------------------------------------------------- through the C ABI

def _kv(run):
    """A run's records as the (key, value) writables the bridge delivers."""
    return [(rec[2:13], rec[13:]) for rec in fc.records(run)]


@functools.lru_cache(maxsize=None)
def _api_maps(stream):
    """4 maps x 3 reducers. Reducer 1's partitions are heavy_key and hi_tie runs, 2 maps each (in the
    streaming shape with a block of ff*10 keys at the end of every map); reducer 0's 37 records put them at
    a partition base of 2 modulo 8."""
    rng = np.random.RandomState(5)
    heavy, _ = fc.case("heavy_key", 2, 1200)  # 480 copies of the heavy key per map: 10 blocks of 48 records
    tie, _ = fc.case("hi_tie", 2, 1200)
    maps = []
    for i, run in enumerate(heavy + tie):
        if stream:
            run += fc.make_run(np.tile(np.frombuffer(fc.ONES_KEY, np.uint8), (60, 1)), 10 + i, rng)
        lead = fc.make_run(fc.distinct_keys(rng, 37), 20 + i, rng)
        trail = fc.make_run(fc.distinct_keys(rng, 5), 30 + i, rng)
        maps.append([_kv(lead), _kv(run), _kv(trail)])
    return maps


def _publish(provider, job, maps, codec=None, **kw):
    ids = []
    for i, parts in enumerate(datagen.streams(maps)):
        mid = f"attempt_{job}_m_{i:06d}_0"
        data, index = encode_partitions(parts, codec, **kw)
        if codec is None:
            assert index[1][0] % 8 == 2  # partition 1 starts 2 past a multiple of 8, as in a Hadoop MOF
        provider.add_mof_device(job, mid, data, index, device=0)
        ids.append(mid)
    return ids


@pytest.fixture
def provider():
    p = UdaProvider()
    yield p
    p.close()


def _same_merge(recs, cpu, maps):
    """Equal key sequences and equal record multisets (equal keys arrive in fetch order on both sides,
    which the two backends need not share), and both are the maps' records."""
    assert [k for k, _ in recs] == [k for k, _ in cpu]
    assert sorted(recs) == sorted(cpu) == sorted(kv for m in maps for kv in m[1])


def test_api_device_fetch(require_gpu, provider, monkeypatch):
    set_env(monkeypatch, {})
    maps = _api_maps(False)
    job = "job_10_0101"
    ids = _publish(provider, job, maps)
    cpu, _, _ = run_reduce("h", job, ids, 1, datagen.TEXT, conf=CPU, kv_buf_size=KV)
    conf = dict(GPU, **{"mapred.uda.gpu.fetch": "device", "mapred.uda.gpu.round.bytes": 100_000,
                        "mapred.uda.gpu.delivery.piece.bytes": PIECE})
    recs, st, _ = run_reduce("h", job, ids, 1, datagen.TEXT, conf=conf, kv_buf_size=KV)
    assert st["merge_path"] == "device-fixed10" and st["rpq_rounds"] > 1, st
    _same_merge(recs, cpu, maps)


def test_api_streaming_decode(require_gpu, provider, monkeypatch):
    """Blocks of about 48 records: the heavy key's 480 copies per map span 10 blocks, so several blocks in
    a row start with the same key as a round bound, and the last blocks hold ff*10 keys only."""
    set_env(monkeypatch, {})
    maps = _api_maps(True)
    job = "job_10_0102"
    ids = _publish(provider, job, maps, codec="snappy", block_size=5000)
    cpu, _, _ = run_reduce("h", job, ids, 1, datagen.TEXT, codec="snappy", conf=CPU, kv_buf_size=KV)
    for pack in ("auto", "off"):
        conf = dict(GPU, **{"mapred.uda.gpu.fetch": "device", "mapred.uda.gpu.round.bytes": 96 << 10,
                            "mapred.uda.gpu.delivery.piece.bytes": PIECE, "mapred.uda.gpu.delivery.pack": pack})
        recs, st, _ = run_reduce("h", job, ids, 1, datagen.TEXT, codec="snappy", conf=conf, kv_buf_size=KV)
        assert st["merge_path"] == "device-fixed10-stream" and st["rpq_rounds"] > 4, (pack, st)
        _same_merge(recs, cpu, maps)
