"""Hadoop's IFile checksum trailer through the GPU consumer paths (mapred.uda.ifile.checksum): stripped
where a partition's span is made, so TeraSort-shaped input keeps the FIXED10 merge and compressed input
its device framing walk, and verified on the device (csrc/gpu/crc32.hip) before any record is delivered.
"""
import pytest

from uda_amd.bridge import UdaConsumer, UdaFallback, UdaProvider, run_reduce
from uda_amd.utils import datagen
from uda_amd.utils.mof import encode_partitions, write_mof

pytestmark = pytest.mark.gpu

GPU = {"mapred.uda.merge.backend": "gpu"}
DEV = dict(GPU, **{"mapred.uda.gpu.fetch": "device"})
CPU = {"mapred.uda.merge.backend": "cpu"}
OFF = {"mapred.uda.ifile.checksum": "off"}
SUM = {"mapred.uda.merge.combine": "sum.int"}


def expected(maps, partition, key_class):
    recs = [kv for m in maps for kv in m[partition]]
    return sorted(recs, key=datagen.sort_key(key_class))


def same_records(recs, want):
    kf = datagen.sort_key(datagen.TEXT)
    assert [kf(kv) for kv in recs] == [kf(kv) for kv in want]
    assert sorted(recs) == sorted(want)


@pytest.fixture
def provider():
    p = UdaProvider()
    yield p
    p.close()


def publish_device(provider, job, maps, codec=None, block_size=5000, trailers=None, corrupt=None):
    """HBM-resident MOFs; trailers: the map numbers that get one (None: all); corrupt(i, data, index)."""
    ids = []
    for i, parts in enumerate(datagen.streams(maps)):
        mid = f"attempt_{job}_m_{i:06d}_0"
        data, index = encode_partitions(parts, codec, block_size, checksum=trailers is None or i in trailers)
        if corrupt:
            data = corrupt(i, data, index)
        provider.add_mof_device(job, mid, data, index, device=0)
        ids.append(mid)
    return ids


def publish_files(provider, tmp_path, job, maps, codec=None, checksum=True, corrupt=None):
    ids = []
    for i, parts in enumerate(datagen.streams(maps)):
        mid = f"attempt_{job}_m_{i:06d}_0"
        path, index = write_mof(str(tmp_path), mid, parts, codec=codec, block_size=16 << 10, checksum=checksum)
        if corrupt:
            with open(path, "rb") as f:
                data = f.read()
            with open(path, "wb") as f:
                f.write(corrupt(i, data, index))
        provider.add_mof_file(job, mid, path)
        ids.append(mid)
    return ids


def flip(victim, partition, where):
    """One flipped bit in a value of one partition of one map, so that the framing stays valid. where >= 0:
    from the partition's start; < 0: from the end of its records (the EOF marker is 2 bytes, a trailer 4)."""
    def corrupt(i, data, index):
        if i != victim:
            return data
        start, raw, plen = index[partition]
        out = bytearray(data)
        out[start + where if where >= 0 else start + raw - 2 + where] ^= 0x01
        return bytes(out)
    return corrupt


def failing_task(job, ids, partition, conf, **kw):
    c = UdaConsumer(len(ids), job, f"attempt_{job}_r_{partition:06d}_0", datagen.TEXT, conf=conf, **kw)
    for m in ids:
        c.fetch("h", job, m, partition)
    with pytest.raises(UdaFallback, match="checksum") as e:
        c.wait(60)
    st = c.close()
    assert c.failure_calls == 1
    return str(e.value), st, c


# ------------------------------------------------------------------------------ device fetch, TeraSort
def test_terasort_with_trailers_keeps_the_fixed10_merge(require_gpu, provider):
    maps = datagen.terasort(num_maps=7, reducers=2, rows_per_map=3000, seed=71)
    ids = publish_device(provider, "job_ck_0001", maps)
    for r in range(2):
        recs, st, _ = run_reduce("h", "job_ck_0001", ids, r, datagen.TEXT, conf=DEV, kv_buf_size=32 << 10)
        assert recs == expected(maps, r, datagen.TEXT)
        assert st["merge_path"] == "device-fixed10", st
        assert st["ifile_checksum"] == "verified" and st["checksum_partitions"] == 7, st
        assert st["checksum_bytes"] == sum(len(p[r]) for p in datagen.streams(maps)) and st["gpu_checksum_ms"] > 0, st


@pytest.mark.parametrize("codec", ["lz4", "snappy"])
def test_compressed_terasort_with_trailers_streams_and_decodes_whole(require_gpu, provider, codec):
    maps = datagen.terasort(num_maps=7, reducers=2, rows_per_map=4000, seed=73)
    job = f"job_ck_02{len(codec):02d}"
    ids = publish_device(provider, job, maps, codec)
    base = dict(DEV, **{"mapred.uda.gpu.round.bytes": 96 << 10})
    for r in range(2):
        recs, st, _ = run_reduce("h", job, ids, r, datagen.TEXT, codec=codec, conf=base, kv_buf_size=32 << 10)
        assert recs == expected(maps, r, datagen.TEXT)
        assert st["merge_path"] == "device-fixed10-stream" and st["device_decoded_blocks"] > 0, st
        assert st["ifile_checksum"] == "verified" and st["checksum_partitions"] == 7 and st["gpu_checksum_ms"] > 0, st
        whole, st2, _ = run_reduce("h", job, ids, r, datagen.TEXT, codec=codec, kv_buf_size=32 << 10,
                                   conf=dict(base, **{"mapred.uda.gpu.decode.stream": 0}))
        assert st2["merge_path"] == "device-fixed10" and whole == recs, st2
        assert st2["ifile_checksum"] == "verified" and st2["checksum_partitions"] == 7, st2


def test_mixed_job_verifies_the_partitions_that_have_a_trailer(require_gpu, provider):
    maps = datagen.terasort(num_maps=6, reducers=2, rows_per_map=2000, seed=75)
    ids = publish_device(provider, "job_ck_0003", maps, trailers={0, 2, 4})
    recs, st, _ = run_reduce("h", "job_ck_0003", ids, 1, datagen.TEXT, conf=DEV, kv_buf_size=32 << 10)
    assert recs == expected(maps, 1, datagen.TEXT)
    assert st["merge_path"] == "device-fixed10" and st["ifile_checksum"] == "verified", st
    assert st["checksum_partitions"] == 3, st


def test_job_without_trailers_launches_nothing(require_gpu, provider):
    maps = datagen.terasort(num_maps=6, reducers=2, rows_per_map=2000, seed=77)
    ids = publish_device(provider, "job_ck_0004", maps, trailers=set())
    recs, st, _ = run_reduce("h", "job_ck_0004", ids, 0, datagen.TEXT, conf=DEV, kv_buf_size=32 << 10)
    assert recs == expected(maps, 0, datagen.TEXT)
    assert st["merge_path"] == "device-fixed10", st
    assert st["ifile_checksum"] == "none" and st["gpu_checksum_ms"] == 0 and st["checksum_partitions"] == 0, st
    ids = publish_device(provider, "job_ck_0005", maps, "lz4", trailers=set())
    recs, st, _ = run_reduce("h", "job_ck_0005", ids, 0, datagen.TEXT, codec="lz4", conf=DEV, kv_buf_size=32 << 10)
    assert recs == expected(maps, 0, datagen.TEXT)
    assert st["ifile_checksum"] == "none" and st["gpu_checksum_ms"] == 0, st


# ------------------------------------------------------------------------------ generic keys, combiner
def test_combining_job_with_trailers_equals_the_job_without(require_gpu, provider):
    maps = datagen.wordcount(num_maps=6, reducers=2, words_per_map=4000, seed=79)
    with_t = publish_device(provider, "job_ck_0006", maps, block_size=64 << 10)
    without = publish_device(provider, "job_ck_0007", maps, block_size=64 << 10, trailers=set())
    conf = dict(DEV, **SUM)
    for r in range(2):
        a, st_a, _ = run_reduce("h", "job_ck_0006", with_t, r, datagen.TEXT, conf=conf, kv_buf_size=8192)
        b, st_b, _ = run_reduce("h", "job_ck_0007", without, r, datagen.TEXT, conf=conf, kv_buf_size=8192)
        assert a == b and len(a) < sum(len(m[r]) for m in maps)
        assert st_a["merge_path"] == st_b["merge_path"] == "device-generic", (st_a, st_b)
        assert st_a["combine_groups"] == st_b["combine_groups"] == len(a)
        assert st_a["ifile_checksum"] == "verified" and st_a["checksum_partitions"] == 6, st_a
        assert st_b["ifile_checksum"] == "none", st_b


# ------------------------------------------------------------------------------ staged path
@pytest.mark.parametrize("phases", [4, 0])
@pytest.mark.parametrize("codec", [None, "lzo"], ids=["none", "lzo"])
def test_wordcount_from_mof_files_staged(require_gpu, provider, tmp_path, codec, phases):
    maps = datagen.wordcount(num_maps=6, reducers=2, words_per_map=5000, seed=81)
    job = f"job_ck_1{phases}{len(codec or '')}"
    ids = publish_files(provider, tmp_path, job, maps, codec)
    conf = dict(GPU, **{"mapred.uda.gpu.progressive.phases": phases})
    recs, st, _ = run_reduce("h", job, ids, 1, datagen.TEXT, codec=codec, conf=conf, kv_buf_size=8192)
    cpu, st_cpu, _ = run_reduce("h", job, ids, 1, datagen.TEXT, codec=codec, conf=CPU, kv_buf_size=8192)
    assert st["backend"] == "gpu" and st["merge_path"].startswith("staged") and st["device_descriptors"] == 0, st
    same_records(recs, cpu)
    same_records(recs, expected(maps, 1, datagen.TEXT))
    assert st["ifile_checksum"] == "verified" and st["checksum_partitions"] == 6 and st["gpu_checksum_ms"] > 0, st
    assert st_cpu["ifile_checksum"] == "verified" and st_cpu["checksum_bytes"] == st["checksum_bytes"], (st, st_cpu)
    if codec:
        assert st["device_decoded_blocks"] > 0, st


def test_over_budget_hybrid_strips_and_says_so(require_gpu, provider):
    maps = datagen.wordcount(num_maps=12, reducers=1, words_per_map=12000, seed=83)
    ids = []
    for i, parts in enumerate(datagen.streams(maps)):
        mid = f"attempt_job_ck_0020_m_{i:06d}_0"
        provider.add_mof_memory("job_ck_0020", mid, *encode_partitions(parts, None, checksum=True))
        ids.append(mid)
    base = dict(GPU, **{"mapred.uda.gpu.merge.bytes": 400_000, "mapred.uda.gpu.spill": "host"})
    for extra in ({}, {"mapred.uda.gpu.hybrid.progressive": 0}, {"mapred.uda.gpu.hybrid.direct": 0}):
        recs, st, _ = run_reduce("h", "job_ck_0020", ids, 0, datagen.TEXT, conf=dict(base, **extra), kv_buf_size=8192)
        same_records(recs, expected(maps, 0, datagen.TEXT))
        assert st["bytes_fetched"] > 400_000 and (st["hybrid_direct"] == 1 or st["lpqs"] >= 2), st
        assert st["ifile_checksum"] == "skipped-over-budget" and st["checksum_partitions"] == 0, st


# ------------------------------------------------------------------------------ corruption
def test_corrupt_partition_fails_the_fixed10_task_before_any_delivery(require_gpu, provider):
    maps = datagen.terasort(num_maps=7, reducers=2, rows_per_map=3000, seed=85)
    ids = publish_device(provider, "job_ck_0030", maps, corrupt=flip(4, 0, 60))
    why, st, c = failing_task("job_ck_0030", ids, 0, DEV, kv_buf_size=32 << 10)
    assert "IFile checksum mismatch in map output attempt_job_ck_0030_m_000004_0: stored 0x" in why, why
    assert c.buffers == 0 and c.bytes == 0
    # the other partition is intact; and off delivers the flipped byte
    recs, st, _ = run_reduce("h", "job_ck_0030", ids, 1, datagen.TEXT, conf=DEV, kv_buf_size=32 << 10)
    assert recs == expected(maps, 1, datagen.TEXT) and st["ifile_checksum"] == "verified"
    recs, st, c = run_reduce("h", "job_ck_0030", ids, 0, datagen.TEXT, conf=dict(DEV, **OFF), kv_buf_size=32 << 10)
    want = expected(maps, 0, datagen.TEXT)
    assert st["merge_path"] == "device-fixed10" and st["ifile_checksum"] == "off", st
    assert st["checksum_partitions"] == 0 and st["gpu_checksum_ms"] == 0 and c.failure_calls == 0, st
    assert len(recs) == len(want) and sorted(recs) != sorted(want)


def test_corrupt_partition_fails_the_generic_device_task_before_any_delivery(require_gpu, provider):
    maps = datagen.wordcount(num_maps=6, reducers=2, words_per_map=4000, seed=87)
    ids = publish_device(provider, "job_ck_0031", maps, block_size=64 << 10, corrupt=flip(1, 1, -1))
    why, st, c = failing_task("job_ck_0031", ids, 1, DEV, kv_buf_size=8192)
    assert "checksum mismatch in map output attempt_job_ck_0031_m_000001_0" in why, why
    assert c.buffers == 0 and c.bytes == 0
    recs, st, c = run_reduce("h", "job_ck_0031", ids, 1, datagen.TEXT, conf=dict(DEV, **OFF), kv_buf_size=8192)
    assert st["merge_path"] == "device-generic" and st["ifile_checksum"] == "off" and c.failure_calls == 0, st
    assert len(recs) == len(expected(maps, 1, datagen.TEXT))


@pytest.mark.parametrize("phases", [0, 4])
def test_corrupt_partition_fails_the_staged_task(require_gpu, provider, tmp_path, phases):
    maps = datagen.wordcount(num_maps=6, reducers=2, words_per_map=5000, seed=89)
    job = f"job_ck_004{phases}"
    ids = publish_files(provider, tmp_path, job, maps, corrupt=flip(5, 0, -1))
    conf = dict(GPU, **{"mapred.uda.gpu.progressive.phases": phases})
    why, st, c = failing_task(job, ids, 0, conf, kv_buf_size=8192)
    assert f"checksum mismatch in map output attempt_{job}_m_000005_0" in why, why
    assert st["merge_path"].startswith("staged"), st
    if phases == 0:
        assert c.buffers == 0 and c.bytes == 0  # (a progressive task may have delivered earlier key ranges)
    recs, st, c = run_reduce("h", job, ids, 0, datagen.TEXT, conf=dict(conf, **OFF), kv_buf_size=8192)
    assert st["ifile_checksum"] == "off" and c.failure_calls == 0, st
    assert len(recs) == len(expected(maps, 0, datagen.TEXT))
