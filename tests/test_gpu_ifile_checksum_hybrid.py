"""IFile checksums in the over-budget GPU hybrid under mapred.uda.ifile.checksum.over.budget=verify
(gpu_merge_staged.cc). LPQ groups lie whole in HBM and are verified as any device merge's runs, before any RPQ
round delivers. Direct RPQ rounds copy contiguous slices of the pinned partitions: every round leaves one raw
CRC state per slice (launch_crc32_states), the delivering thread folds a partition's states in round order
and compares when its body is complete, before that round is delivered (earlier key ranges may be out already,
as on the progressive staged path). With the key absent the trailers are stripped unverified, as before.
"""
import pytest

from tests.combine_cases import expected_task
from uda_amd.bridge import UdaConsumer, UdaFallback, UdaProvider, run_reduce
from uda_amd.utils import datagen
from uda_amd.utils.ifile import encode_stream
from uda_amd.utils.mof import encode_partitions

pytestmark = pytest.mark.gpu
BUDGET = 400_000
KEY = "mapred.uda.ifile.checksum.over.budget"
BASE = {"mapred.uda.merge.backend": "gpu", "mapred.uda.gpu.merge.bytes": BUDGET, "mapred.uda.gpu.spill": "host"}
CONF = dict(BASE, **{KEY: "verify"})
CONFIGS = {
    "progressive-direct": {},
    "direct": {"mapred.uda.gpu.hybrid.progressive": 0},
    "lpq-host": {"mapred.uda.gpu.hybrid.direct": 0},
    "lpq-disk": {"mapred.uda.gpu.spill": "disk"},
}
VICTIM = 5
NUM = {name: i for i, name in enumerate(CONFIGS)}  # (job ids)


@pytest.fixture(scope="module")
def maps():
    return datagen.wordcount(num_maps=12, reducers=1, words_per_map=12000, seed=91)


@pytest.fixture(scope="module")
def want(maps):
    recs = [kv for m in maps for kv in m[0]]
    return sorted(recs, key=datagen.sort_key(datagen.TEXT))


@pytest.fixture
def provider():
    p = UdaProvider()
    yield p
    p.close()


def same_records(recs, want):
    """The sorted oracle: keys in order, and the same records (equal keys come in fetch order)."""
    kf = datagen.sort_key(datagen.TEXT)
    assert [kf(kv) for kv in recs] == [kf(kv) for kv in want]
    assert sorted(recs) == sorted(want)


def flip(victim, partition, where):
    """One flipped bit in a value of one partition of one map, so that the framing stays valid. where >= 0:
    from the partition's start; < 0: from the end of its records (the EOF marker is 2 bytes, a trailer 4);
    "trailer": in the stored checksum itself."""
    def corrupt(i, data, index):
        if i != victim:
            return data
        start, raw, plen = index[partition]
        out = bytearray(data)
        if where == "trailer":
            assert plen == raw + 4
            out[start + plen - 1] ^= 0x01
        else:
            out[start + where if where >= 0 else start + raw - 2 + where] ^= 0x01
        return bytes(out)
    return corrupt


def publish(provider, job, maps, trailers=None, corrupt=None):
    """-> map ids, body bytes of the partitions that carry a trailer"""
    ids, bodies = [], 0
    for i, parts in enumerate(datagen.streams(maps)):
        mid = f"attempt_{job}_m_{i:06d}_0"
        has = trailers is None or i in trailers
        data, index = encode_partitions(parts, None, checksum=has)
        if has:
            bodies += index[0][1]
        if corrupt:
            data = corrupt(i, data, index)
        provider.add_mof_memory(job, mid, data, index)
        ids.append(mid)
    return ids, bodies


def run(job, ids, name, tmp_path, conf=CONF):
    kw = dict(local_dirs=(str(tmp_path),)) if name == "lpq-disk" else {}
    return run_reduce("h", job, ids, 0, datagen.TEXT, conf=dict(conf, **CONFIGS[name]), kv_buf_size=8192, **kw)


def check_path(st, name):
    assert st["bytes_fetched"] > BUDGET and st["rpq_rounds"] > 1, st
    if name == "progressive-direct":
        assert st["merge_path"] == "staged-progressive-direct" and st["hybrid_direct"] == 1 and st["lpqs"] == 0, st
    if name == "direct":
        assert st["merge_path"] == "staged" and st["hybrid_direct"] == 1 and st["lpqs"] == 0, st
    if name.startswith("lpq"):
        assert st["merge_path"] == "staged" and st["lpqs"] >= 2 and st["hybrid_direct"] == 0, st


# 1
@pytest.mark.parametrize("name", list(CONFIGS))
def test_intact_input_is_verified(require_gpu, provider, tmp_path, maps, want, name):
    job = "job_ckh_01%02d" % NUM[name]
    ids, bodies = publish(provider, job, maps)
    recs, st, c = run(job, ids, name, tmp_path)
    print({k: st[k] for k in ("merge_path", "lpqs", "rpq_rounds", "bytes_fetched", "checksum_partitions",
                              "checksum_bytes", "gpu_checksum_ms")})
    same_records(recs, want)
    assert st["ifile_checksum"] == "verified", st
    assert st["checksum_partitions"] == 12 and st["checksum_bytes"] == bodies, (st, bodies)
    assert st["gpu_checksum_ms"] > 0, st
    check_path(st, name)
    assert c.bytes == len(encode_stream(want)) and c.failure_calls == 0


# 2
@pytest.mark.parametrize("name", list(CONFIGS))
def test_only_the_partitions_with_a_trailer_are_verified(require_gpu, provider, tmp_path, maps, want, name):
    job = "job_ckh_02%02d" % NUM[name]
    ids, bodies = publish(provider, job, maps, trailers={0, 2, 4, 6, 8, 10})
    recs, st, _ = run(job, ids, name, tmp_path)
    same_records(recs, want)
    assert st["ifile_checksum"] == "verified" and st["checksum_partitions"] == 6, st
    assert st["checksum_bytes"] == bodies, (st, bodies)
    check_path(st, name)


def test_a_job_without_trailers_launches_nothing(require_gpu, provider, tmp_path, maps, want):
    ids, _ = publish(provider, "job_ckh_0290", maps, trailers=set())
    for name in ("progressive-direct", "direct"):
        recs, st, _ = run("job_ckh_0290", ids, name, tmp_path)
        same_records(recs, want)
        assert st["ifile_checksum"] == "none" and st["gpu_checksum_ms"] == 0 and st["checksum_partitions"] == 0, st


# 3
@pytest.mark.parametrize("where", [60, -1, "trailer"])
@pytest.mark.parametrize("name", list(CONFIGS))
def test_one_flipped_bit_fails_the_task(require_gpu, provider, tmp_path, maps, want, name, where):
    job = "job_ckh_03%02d%s" % (NUM[name], {60: "0", -1: "1", "trailer": "2"}[where])
    ids, _ = publish(provider, job, maps, corrupt=flip(VICTIM, 0, where))
    kw = dict(local_dirs=(str(tmp_path),)) if name == "lpq-disk" else {}
    conf = dict(CONF, **CONFIGS[name])
    c = UdaConsumer(len(ids), job, f"attempt_{job}_r_000000_0", datagen.TEXT, conf=conf, kv_buf_size=8192, **kw)
    for m in ids:
        c.fetch("h", job, m, 0)
    with pytest.raises(UdaFallback, match=f"checksum mismatch in map output attempt_{job}_m_{VICTIM:06d}_0"):
        c.wait(60)
    c.close()
    assert c.failure_calls == 1
    full = len(encode_stream(want))
    print(name, where, "delivered before the failure:", c.buffers, "buffers,", c.bytes, "of", full, "bytes")
    if name.startswith("lpq"):
        assert c.buffers == 0 and c.bytes == 0  # every LPQ merge precedes the first RPQ round
    else:
        assert c.bytes < full  # the round the mismatch is found in is not delivered
    # off delivers the flipped bit
    recs, st, c = run(job, ids, name, tmp_path, conf=dict(CONF, **{"mapred.uda.ifile.checksum": "off"}))
    assert st["ifile_checksum"] == "off" and c.failure_calls == 0, st
    assert st["checksum_partitions"] == 0 and st["gpu_checksum_ms"] == 0, st
    assert len(recs) == len(want) and c.bytes == full


# 4
@pytest.mark.parametrize("name", ["direct", "lpq-host"])
def test_verify_together_with_the_over_budget_combiner(require_gpu, provider, tmp_path, maps, name):
    job = "job_ckh_04%02d" % NUM[name]
    ids, bodies = publish(provider, job, maps)
    conf = dict(CONF, **{"mapred.uda.merge.combine": "sum.int", "mapred.uda.merge.combine.over.budget": "combine"})
    recs, st, _ = run(job, ids, name, tmp_path, conf=conf)
    assert recs == expected_task(maps, 0, datagen.TEXT, "sum.int")
    assert st["combine"] == "sum.int" and st["ifile_checksum"] == "verified", st
    assert st["checksum_partitions"] == 12 and st["checksum_bytes"] == bodies, st
    check_path(st, name)


# 6 (5, the unknown value, needs no GPU: tests/test_ifile_checksum_conf.py)
@pytest.mark.parametrize("extra", [{}, {KEY: "skip"}], ids=["absent", "skip"])
def test_the_default_still_strips_and_says_so(require_gpu, provider, tmp_path, maps, want, extra):
    job = "job_ckh_06%02d" % len(extra)
    ids, _ = publish(provider, job, maps)
    for name in CONFIGS:
        recs, st, _ = run(job, ids, name, tmp_path, conf=dict(BASE, **extra))
        same_records(recs, want)
        assert st["ifile_checksum"] == "skipped-over-budget", st
        assert st["checksum_partitions"] == 0 and st["checksum_bytes"] == 0 and st["gpu_checksum_ms"] == 0, st
        check_path(st, name)
