"""ShuffleJob on empty, one-record and lopsided key-range cells (tests/shuffle_bounds_cases.py).

Every other test of the job cuts uniform TeraGen keys at quantile bounds, so every (reducer, round) cell is
full, every rank sends every peer something in every round and every reducer has data in the last round.
Here crafted bounds over the same store (ShuffleJob.set_bounds takes any ascending bounds) leave cells empty,
holding one record or holding everything, and every reducer's delivered bytes are compared byte for byte
with a Python oracle that cuts the store's records at those bounds: a reducer must receive exactly the keys
of its range (a key equal to a bound opens the upper cell; the low 16 key bits decide too), in order, with
one EOF marker, in both of two steps (both slot parities are reused after empty rounds).

Also here: ShuffleJob.sample_keys against the oracle's positions, and index_record / mof_bytes /
peer_send_bytes against the store layout."""
import gc

import numpy as np
import pytest

from tests import shuffle_bounds_cases as sb
from uda_amd.parallel.dist import DistContext

pytestmark = pytest.mark.gpu

MAPS, ROWS, KV_BUF, PIECE = 3, 12_000, 8192, 32 << 10
SHAPE = dict(maps_per_rank=MAPS, rows_per_gpu=ROWS, kv_buf_bytes=KV_BUF, d2h_piece_bytes=PIECE, sample_every=64,
             validate=True, check_delivery=True)
PIECE_RECORDS = sb.piece_records(KV_BUF, PIECE)  # 312: a full cell of (3, 4) is about 1000 records, 4 pieces


class Collector:
    """Python sink: per reducer, the delivered bytes and every buffer's length."""

    def __init__(self, reducers):
        self.data = [bytearray() for _ in range(reducers)]
        self.lens = [[] for _ in range(reducers)]

    def __call__(self, r, b):
        self.data[r] += b
        self.lens[r].append(len(b))


def _bare_jobs(world, group):
    """`world` generated ShuffleJobs of the tests' shape: a store and nothing else (no bounds, no plan)."""
    from uda_amd import native
    from uda_amd.models.terasort import TeraSortConfig
    jobs = [native().ShuffleJob(dict(device=0, rank=r, world=world, maps_per_rank=MAPS, records_per_map=ROWS // MAPS,
                                     seed=TeraSortConfig().seed, local_group=group, deliver_host=False))
            for r in range(world)]
    for j in jobs:
        j.generate()
    return jobs


def _parts(jobs):
    """parts[d]: every partition for destination d, from every rank and map."""
    return [[j.read_partition(m, d) for j in jobs for m in range(MAPS)] for d in range(len(jobs))]


_STORES = {}


def _store(world):
    """The store of a `world`-rank job of this shape, read once (it depends on the seed, the world and the
    shape alone; _run checks that for every job it builds): (parts[d], sorted keys[d])."""
    if world not in _STORES:
        jobs = _bare_jobs(world, f"sbstore{world}")
        parts = _parts(jobs)
        del jobs
        gc.collect()
        _STORES[world] = (parts, [sb.sorted_records(p)[1] for p in parts])
    return _STORES[world]


def _run(case, world, R, Q, store="hbm", tmp_path=None, steps=2, **kw):
    """A job of `world` ranks under the named bounds, `steps` validated steps into collector sinks, everything
    checked against the oracle."""
    from uda_amd.models.terasort import TeraSortConfig, TeraSortShuffle, check_stats, make_local_group, run_collective
    parts, keys = _store(world)
    built = []

    def bounds_fn(per_dest, cells):
        assert cells == R * Q and len(per_dest) == world
        built.append(sb.BUILDERS[case](keys, R, Q))
        return built[-1]

    if tmp_path is not None:
        kw = dict(kw, local_dirs=str(tmp_path))
    cfg = TeraSortConfig(**SHAPE, reducers=R, rounds=Q, store=store, **kw)
    tag = "".join(f"{k}{v}" for k, v in sorted(kw.items()) if k != "local_dirs")
    if world == 1:
        top = TeraSortShuffle(DistContext(), cfg, device=0)
        top.setup(bounds_fn=bounds_fn)
        jobs, ck, rec = [top.job], [top.expected_checksum], [top.expected_records]
    else:
        jobs, ck, rec = make_local_group(world, cfg, group=f"sb{case}{world}{R}{Q}{store}{tag}", bounds_fn=bounds_fn)
    assert len(built) == 1
    bounds = built[0]
    assert _parts(jobs) == parts, "the job's store is not the one the bounds and the oracle were built from"
    streams, counts = sb.oracle(parts, bounds, R, Q)
    sb.check_case(case, counts, R, Q)  # the case holds what its name says on the real store
    if case == "key_hit":  # every bound outside the triple is a record's key: that record opens the upper cell
        j = sb.key_hit_triple_at(R * Q)
        for d in range(world):
            have = {(int(h), int(l)) for h, l in keys[d]}
            assert all((int(h), int(l)) in have for c, (h, l) in enumerate(bounds[d]) if j is None or not j <= c < j + 3)
    for d in range(world):
        assert list(jobs[d].reducer_records()) == [sum(row) for row in counts[d]]
        assert rec[d] == sum(map(sum, counts[d])) == len(parts[d]) * -(-(ROWS // MAPS - d) // world)
    for step in range(steps):
        sinks = [Collector(R) for _ in range(world)]
        for d in range(world):
            jobs[d].set_python_sink(sinks[d], True)
        stats = run_collective(jobs, lambda j: j.run_step(True))
        for d, st in enumerate(stats):
            where = f"step {step} rank {d}"
            for i in range(R):
                lens, data = sinks[d].lens[i], bytes(sinks[d].data[i])
                assert data == streams[d][i], f"{where} reducer {i}: {len(data)} bytes, expected {len(streams[d][i])}"
                assert lens and all(0 < n <= KV_BUF for n in lens), (where, i, lens)
                assert all(n % sb.RECORD == 0 for n in lens[:-1]) and lens[-1] % sb.RECORD == 2, (where, i, lens)
            assert st["validated"]
            check_stats(st, rec[d], ck[d], jobs[d].reducer_records())
            assert st["packed_pieces"] + st["raw_pieces"] == sb.pieces_needed(counts[d], PIECE_RECORDS), where
            if kw.get("delivery_pack") == "off":
                assert st["packed_pieces"] == 0
    return jobs, stats, counts


# ------------------------------------------------------------------------------------------------ the matrix
@pytest.mark.parametrize("R,Q", [(1, 5), (3, 4), (4, 1), (2, 2)])
@pytest.mark.parametrize("case", sb.CASES)
def test_one_rank_hbm(require_gpu, case, R, Q):
    _run(case, 1, R, Q)


@pytest.mark.parametrize("store", ["host", "disk"])
@pytest.mark.parametrize("case", ["all_low", "collapsed", "key_hit"])
def test_one_rank_spill_tiers(require_gpu, tmp_path, case, store):
    _, stats, _ = _run(case, 1, 3, 4, store=store, tmp_path=tmp_path)
    assert stats[0]["bytes_h2d"] == stats[0]["bytes_in"]


@pytest.mark.parametrize("store,R,Q", [("hbm", 2, 3), ("host", 2, 5), ("disk", 2, 5)])
@pytest.mark.parametrize("world", [2, 3])
@pytest.mark.parametrize("case", ["mixed", "collapsed", "key_hit", "all_high"])
def test_local_group(require_gpu, tmp_path, case, world, store, R, Q):
    """Ranks as threads on one GPU. `mixed`: the ranks disagree about which rounds are empty, so in one round
    some pairs exchange nothing and one rank merges nothing while its peers do."""
    _, stats, counts = _run(case, world, R, Q, store=store, tmp_path=tmp_path)
    for d, st in enumerate(stats):
        assert st["exchange_errors"] == 0 and st["bytes_sent"] > 0
    if case == "mixed":
        for q in range(Q):
            busy = [any(counts[d][i][q] for i in range(R)) for d in range(world)]
            assert busy[0] == (q == Q - 1) and busy[-1] == (q == 0)


@pytest.mark.parametrize("env", [("UDA_KWAY", "0"), ("UDA_KWAY_STAGED", "1")])
@pytest.mark.parametrize("case", ["collapsed", "key_hit"])
def test_other_merge_kernels(require_gpu, monkeypatch, case, env):
    """The merge tree (UDA_KWAY=0) and the LDS-staged K-way kernel see the same empty and one-record groups."""
    monkeypatch.setenv(*env)
    _, stats, _ = _run(case, 1, 3, 4)
    assert (stats[0]["merge_passes"] > 1) == (env[0] == "UDA_KWAY")


@pytest.mark.parametrize("kw", [dict(delivery_pack="off"), dict(delivery_order="reducer")], ids=["pack-off", "by-reducer"])
@pytest.mark.parametrize("case", ["collapsed", "all_high"])
def test_delivery_variants(require_gpu, case, kw):
    _run(case, 1, 3, 4, **kw)


@pytest.mark.parametrize("world,R,Q", [(1, 3, 4), (2, 2, 3)])
def test_replan_compares_splits_and_counts_with_zeros(require_gpu, world, R, Q):
    _, stats, _ = _run("collapsed", world, R, Q, replan=True)
    assert all(st["plan_ms"] > 0 for st in stats)


# ------------------------------------------------------------------------------------------------ related checks
@pytest.mark.parametrize("world", [1, 3])
def test_sample_keys_against_the_store(require_gpu, world):
    """Run r = m * W + d contributes its keys at positions every // 2 + k * every < n, grouped by destination
    in run order."""
    jobs = _bare_jobs(world, f"sbsample{world}")
    run_keys = [[[sb.record_keys(sb.partition_records(j.read_partition(m, d))) for d in range(world)]
                 for m in range(MAPS)] for j in jobs]
    n = max(len(k) for per_map in run_keys[0] for k in per_map)
    assert n == -(-(ROWS // MAPS) // world)
    for every in (1, 2, 64, n - 1, n, 2 * n + 1):
        for r, j in enumerate(jobs):
            got = [np.asarray(a) for a in j.sample_keys(every)]
            assert len(got) == world
            for d in range(world):
                want = [run_keys[r][m][d][every // 2::every] for m in range(MAPS)]
                want = np.concatenate(want).reshape(-1, 2)
                assert got[d].reshape(-1, 2).tolist() == want.tolist(), (every, r, d)
        if every >= n:  # a run shorter than every // 2 + 1 contributes nothing
            assert sum(len(np.asarray(a)) for a in jobs[0].sample_keys(every)) == (MAPS * world if every == n else 0)


@pytest.mark.parametrize("world", [1, 3])
def test_index_records_and_send_bytes_against_the_store_layout(require_gpu, world):
    """Every run starts 16-byte aligned behind its predecessor's EOF marker, every MOF 256-byte aligned; a
    part is its records and the marker; a rank sends a peer every record it holds for it."""
    from uda_amd.models.terasort import TeraSortConfig, TeraSortShuffle, make_local_group
    R, Q = 2, 3
    cfg = TeraSortConfig(**SHAPE, reducers=R, rounds=Q)
    bounds_fn = lambda per_dest, cells: sb.collapsed(_store(world)[1], R, Q)  # noqa: E731
    if world == 1:
        top = TeraSortShuffle(DistContext(), cfg, device=0)
        top.setup(bounds_fn=bounds_fn)
        jobs = [top.job]
    else:
        jobs, _, _ = make_local_group(world, cfg, group=f"sbindex{world}", bounds_fn=bounds_fn)
    per_map = ROWS // MAPS
    nrec = [per_map // world + (1 if d < per_map % world else 0) for d in range(world)]
    for r, j in enumerate(jobs):
        store = 0
        for m in range(MAPS):
            off = 0
            for d in range(world):
                part = nrec[d] * sb.RECORD + 2
                assert list(j.index_record(m, d)) == [off, part, part]
                assert len(j.read_partition(m, d)) == part
                end = off + part
                off = -(-end // 16) * 16
            assert j.mof_bytes(m) == -(-end // 256) * 256
            store += j.mof_bytes(m)
        assert j.store_bytes == store
        assert list(j.peer_send_bytes()) == [0 if p == r else MAPS * nrec[p] * sb.RECORD for p in range(world)]
        for bad in [(-1, 0), (MAPS, 0), (0, world), (0, -1)]:
            with pytest.raises(IndexError):
                j.index_record(*bad)
