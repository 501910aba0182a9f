"""The reduce-side combiner on the device (csrc/gpu/combine.hip: heads, segmented sum, compacting
gather): the GPU merge under mapred.uda.merge.combine must deliver, byte for byte, what the CPU backend
and a pure-Python oracle deliver (tests/combine_cases.py), one record per distinct key, on every GPU
path that combines; the over-budget hybrid delivers the uncombined stream and says so."""
import collections

import pytest

import uda_amd
from tests.combine_cases import combine_records, expected_task, huge_key_runs, ops_cases, oracle
from uda_amd import ops
from uda_amd.bridge import UdaConsumer, UdaFallback, UdaProvider, run_reduce
from uda_amd.utils import datagen
from uda_amd.utils.ifile import J2CQueueReader, encode_stream, text
from uda_amd.utils.mof import encode_partitions

pytestmark = pytest.mark.gpu
GPU = {"mapred.uda.merge.backend": "gpu"}
SUM = {"mapred.uda.merge.backend": "gpu", "mapred.uda.merge.combine": "sum.int"}
TILE = uda_amd.native().combine_tile()  # the segmented sum's elements per workgroup: the group-length case is built on it
CASES = list(ops_cases(TILE))


def _check(runs, key_class, op, kv_buf):
    want = oracle(runs, key_class, op)
    g_body, g_cuts = ops.merge_runs(runs, key_class, "gpu", kv_buf=kv_buf, combine=op)
    stats = dict(ops.last_stats)
    c_body, _ = ops.merge_runs(runs, key_class, "cpu", kv_buf=kv_buf, combine=op)
    assert c_body == want
    assert g_body == want
    r = J2CQueueReader(max_len=kv_buf)
    for b in ops.buffers(g_body, g_cuts):
        r.feed(b)
    assert r.eof and encode_stream(r.records, eof=False) == want
    assert stats["records"] == len(r.records)
    return stats


@pytest.mark.parametrize("name,key_class,op,runs", CASES, ids=[c[0] for c in CASES])
def test_gpu_combine_matches_cpu_and_oracle(require_gpu, name, key_class, op, runs):
    for kv_buf in (4096, 256):
        st = _check(runs, key_class, op, kv_buf)
    if name == "one-key":
        assert st["records"] == 1 and st["records_in"] == 30000
    if name == "all-distinct":
        assert st["records"] == st["records_in"] == 6000
        assert ops.merge_runs(runs, key_class, "gpu", combine=op) == ops.merge_runs(runs, key_class, "gpu")


def test_gpu_combine_pairwise_tree(require_gpu, monkeypatch):
    """The pairwise merge tree (no single-pass K-way) leaves the same order for the combiner."""
    monkeypatch.setenv("UDA_GKWAY", "0")
    name, key_class, op, runs = CASES[0]
    _check(runs, key_class, op, 4096)


def test_gpu_combine_huge_keys_stay_three_groups(require_gpu):
    """Content lengths 65 535 / 65 536 / 65 537 share the clamped 16-bit length field and every leading byte."""
    st = _check(huge_key_runs(), datagen.TEXT, "sum.int", 1 << 20)
    assert st["records"] == 3 and st["records_in"] == 6


def test_gpu_combine_wrong_value_length_raises(require_gpu):
    runs = [encode_stream([(text(b"a%03d" % i), b"\0\0\0\1") for i in range(300)]),
            encode_stream([(text(b"a007"), b"\0\0\0\2"), (text(b"bad-key"), b"12345"), (text(b"c"), b"\0\0\0\3")])]
    with pytest.raises(RuntimeError, match=r"value of 5 bytes.*bad-key"):
        ops.merge_runs(runs, datagen.TEXT, "gpu", combine="sum.int")
    with pytest.raises(RuntimeError, match=r"value of 4 bytes \(8 expected\)"):
        ops.merge_runs(runs[:1], datagen.TEXT, "gpu", combine="sum.long")
    # the merger is as good as before: the same runs without the bad record
    _check([runs[0], encode_stream([(text(b"a007"), b"\0\0\0\2")])], datagen.TEXT, "sum.int", 4096)


# ---------------------------------------------------------------------------------------- reduce tasks
@pytest.fixture
def provider():
    p = UdaProvider()
    yield p
    p.close()


def _publish(provider, job, maps, where="device", codec=None):
    ids = []
    for i, parts in enumerate(datagen.streams(maps)):
        mid = f"attempt_{job}_m_{i:06d}_0"
        data, index = encode_partitions(parts, codec, block_size=64 << 10)
        if where == "device":
            provider.add_mof_device(job, mid, data, index, device=0)
        else:
            provider.add_mof_memory(job, mid, data, index)
        ids.append(mid)
    return ids


def _combined_ok(recs, st, maps, partition, c):
    want = expected_task(maps, partition, datagen.TEXT, "sum.int")
    assert recs == want
    assert st["combine"] == "sum.int" and st["combine_groups"] == len(want) == st["records"]
    assert st["combine_in_records"] == sum(len(m[partition]) for m in maps)
    assert st["bytes_delivered"] == len(encode_stream(want)) == c.bytes


@pytest.mark.parametrize("round_bytes", [64 << 10, 1 << 30])
def test_task_device_mofs_combine_in_key_range_rounds(require_gpu, provider, round_bytes):
    maps = datagen.wordcount(num_maps=9, reducers=1, words_per_map=6000, seed=17)
    job = f"job_8_01{round_bytes % 7}"
    ids = _publish(provider, job, maps)
    conf = dict(SUM, **{"mapred.uda.gpu.fetch": "device", "mapred.uda.gpu.round.bytes": round_bytes})
    recs, st, c = run_reduce("h", job, ids, 0, datagen.TEXT, conf=conf, kv_buf_size=8192)
    assert st["merge_path"] == "device-generic", st
    if round_bytes == 64 << 10:
        assert st["rpq_rounds"] > 1
    _combined_ok(recs, st, maps, 0, c)
    # the CPU backend over the same MOFs delivers the same records
    cpu, st_cpu, _ = run_reduce("h", job, ids, 0, datagen.TEXT, kv_buf_size=8192,
                                conf={"mapred.uda.merge.backend": "cpu", "mapred.uda.merge.combine": "sum.int"})
    assert cpu == recs and st_cpu["bytes_delivered"] == st["bytes_delivered"]


def test_task_snappy_device_mofs_decoded_then_combined(require_gpu, provider):
    maps = datagen.wordcount(num_maps=6, reducers=2, words_per_map=5000, seed=19)
    ids = _publish(provider, "job_8_0200", maps, codec="snappy")
    conf = dict(SUM, **{"mapred.uda.gpu.fetch": "device"})
    for r in range(2):
        recs, st, c = run_reduce("h", "job_8_0200", ids, r, datagen.TEXT, codec="snappy", conf=conf, kv_buf_size=8192)
        assert st["device_decoded_blocks"] > 0 and st["merge_path"] == "device-generic", st
        _combined_ok(recs, st, maps, r, c)


@pytest.mark.parametrize("phases", [None, 3])
def test_task_host_mofs_within_budget_combine(require_gpu, provider, phases):
    maps = datagen.wordcount(num_maps=9, reducers=1, words_per_map=6000, seed=23)
    job = f"job_8_030{phases or 0}"
    ids = _publish(provider, job, maps, where="host")
    conf = dict(SUM)
    if phases:
        conf["mapred.uda.gpu.progressive.phases"] = phases
    recs, st, c = run_reduce("h", job, ids, 0, datagen.TEXT, conf=conf, max_buf_kb=16, min_buf_kb=16, kv_buf_size=8192)
    assert st["merge_path"] in ("staged", "staged-progressive"), st
    _combined_ok(recs, st, maps, 0, c)


@pytest.mark.parametrize("where", ["device", "host"])
def test_task_terasort_with_sum_int_fails_once(require_gpu, provider, where):
    """TeraSort-shaped input never takes the FIXED10 paths under combine: its 90-byte values fail the task
    through failureInUda, once, and nothing is delivered."""
    maps = datagen.terasort(num_maps=4, reducers=1, rows_per_map=1500, seed=29)
    job = "job_8_040" + str(len(where))
    ids = _publish(provider, job, maps, where=where)
    conf = dict(SUM, **({"mapred.uda.gpu.fetch": "device"} if where == "device" else {}))
    c = UdaConsumer(len(ids), job, f"attempt_{job}_r_000000_0", datagen.TEXT, conf=conf, kv_buf_size=64 << 10)
    for m in ids:
        c.fetch("h", job, m, 0)
    with pytest.raises(UdaFallback, match="value of 91 bytes"):
        c.wait(60)
    c.close()
    assert c.failure_calls == 1 and c.bytes == 0 and c.buffers == 0


def test_task_over_budget_skips_the_combiner(require_gpu, provider):
    maps = datagen.wordcount(num_maps=12, reducers=1, words_per_map=12000, seed=37)
    ids = _publish(provider, "job_8_0500", maps, where="host")
    conf = dict(SUM, **{"mapred.uda.gpu.merge.bytes": 400_000, "mapred.uda.gpu.spill": "host"})
    recs, st, _ = run_reduce("h", "job_8_0500", ids, 0, datagen.TEXT, conf=conf, kv_buf_size=8192)
    assert st["bytes_fetched"] > 400_000
    assert st["combine"] == "skipped-over-budget", st
    kf = datagen.sort_key(datagen.TEXT)
    keys = [kf(kv) for kv in recs]
    assert keys == sorted(keys) and len(recs) == sum(len(m[0]) for m in maps)
    sums = collections.Counter()
    for k, v in recs:
        sums[k] += int.from_bytes(v, "big")
    assert [(k, s.to_bytes(4, "big")) for k, s in sorted(sums.items(), key=lambda kv: kf(kv))] == \
        expected_task(maps, 0, datagen.TEXT, "sum.int")


@pytest.mark.parametrize("shape", ["terasort", "wordcount"])
def test_task_combine_none_is_the_task_without_the_key(require_gpu, provider, shape):
    maps = (datagen.terasort(num_maps=4, reducers=1, rows_per_map=1500, seed=41) if shape == "terasort" else
            datagen.wordcount(num_maps=5, reducers=1, words_per_map=3000, seed=41))
    job = "job_8_060" + str(len(shape))
    ids = _publish(provider, job, maps)
    base = dict(GPU, **{"mapred.uda.gpu.fetch": "device"})
    a, st_a, _ = run_reduce("h", job, ids, 0, datagen.TEXT, conf=base, kv_buf_size=64 << 10)
    b, st_b, _ = run_reduce("h", job, ids, 0, datagen.TEXT, conf=dict(base, **{"mapred.uda.merge.combine": "none"}),
                            kv_buf_size=64 << 10)
    # (equal keys of different maps may come in either map order; TeraSort keys are distinct)
    assert [k for k, _ in a] == [k for k, _ in b] and sorted(a) == sorted(b)
    assert st_a["merge_path"] == st_b["merge_path"]
    assert st_a["merge_path"] == ("device-fixed10" if shape == "terasort" else "device-generic")
    assert st_a["combine"] == st_b["combine"] == "none" and st_b["combine_groups"] == 0
    assert st_a["bytes_delivered"] == st_b["bytes_delivered"] and st_a["buffers"] == st_b["buffers"]
    if shape == "wordcount":  # and the combiner would have had work to do
        assert len(combine_records(a, datagen.TEXT, "sum.int")) < len(a)
