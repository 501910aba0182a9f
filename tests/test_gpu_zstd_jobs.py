"""ZStandardCodec jobs through the GPU consumer paths: HBM-resident map outputs on the descriptor path, host map
outputs on the staged path and in the over-budget hybrid's LPQ merges, the host decoder under
mapred.uda.gpu.decompress=0, FIXED10 and generic merges, a combiner, IFile checksum trailers (found only once a
frame is decoded), corrupt frames, which fail the task once, naming the map output, before any record is
delivered, and partitions of two frames, which the device decode refuses by name and the host decoder takes."""
import struct
import zlib

import pytest

from tests.combine_cases import expected_task
from uda_amd._native import native as load_native
from uda_amd.bridge import UdaConsumer, UdaFallback, UdaProvider, run_reduce
from uda_amd.utils import datagen
from uda_amd.utils.mof import encode_partitions, write_mof

pytestmark = pytest.mark.gpu

GPU = {"mapred.uda.merge.backend": "gpu"}
DEV = dict(GPU, **{"mapred.uda.gpu.fetch": "device"})
OFF = {"mapred.uda.ifile.checksum": "off"}


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


def two_frame_partitions(parts, checksum):
    """(file bytes, index) with every partition written as two zstd frames."""
    n = load_native()
    data, index = bytearray(), []
    for p in parts:
        cut = len(p) // 3
        body = n.zstd_compress(p[:cut]) + n.zstd_compress(p[cut:])
        if checksum:
            body += struct.pack(">I", zlib.crc32(body))
        index.append((len(data), len(p), len(body)))
        data += body
    return bytes(data), index


def publish(provider, job, maps, where, checksum=False, corrupt=None, tmp_path=None, two_frames=False):
    ids = []
    for i, parts in enumerate(datagen.streams(maps)):
        mid = f"attempt_{job}_m_{i:06d}_0"
        data, index = two_frame_partitions(parts, checksum) if two_frames else encode_partitions(parts, "zstd", checksum=checksum)
        if corrupt:
            data = corrupt(i, data, index)
        if where == "device":
            provider.add_mof_device(job, mid, data, index, device=0)
        elif where == "memory":
            provider.add_mof_memory(job, mid, data, index)
        else:
            path, _ = write_mof(str(tmp_path), mid, parts, codec="zstd", checksum=checksum)
            provider.add_mof_file(job, mid, path)
        ids.append(mid)
    return ids


def flip_mid_frame(victim, partition):
    def corrupt(i, data, index):
        if i != victim:
            return data
        start, _, plen = index[partition]
        out = bytearray(data)
        out[start + plen // 2] ^= 0x10
        return bytes(out)
    return corrupt


def break_descriptor(victim, partition):
    """Sets the frame's reserved descriptor bit: a frame every decoder refuses whatever follows."""
    def corrupt(i, data, index):
        if i != victim:
            return data
        out = bytearray(data)
        out[index[partition][0] + 4] |= 0x08
        return bytes(out)
    return corrupt


@pytest.mark.parametrize("checksum", [False, True], ids=["no-trailers", "trailers"])
def test_terasort_device_mofs_reach_the_fixed10_merge(require_gpu, provider, checksum):
    job = f"job_s_001{int(checksum)}"
    maps = datagen.terasort(num_maps=7, reducers=2, rows_per_map=4000, seed=61)
    ids = publish(provider, job, maps, "device", checksum=checksum)
    for r in range(2):
        recs, st, c = run_reduce("h", job, ids, r, datagen.TEXT, codec="zstd", conf=DEV, kv_buf_size=32 << 10)
        assert recs == expected(maps, r, datagen.TEXT)
        assert st["merge_path"] == "device-fixed10", st  # no per-round streaming decode for zstd
        assert st["device_descriptors"] == 7 and st["device_decoded_streams"] == 7 and st["device_decoded_blocks"] == 0, st
        assert st["ifile_checksum"] == ("verified" if checksum else "none"), st
        assert st["checksum_partitions"] == (7 if checksum else 0) and c.failure_calls == 0, st


@pytest.mark.parametrize("checksum", [False, True], ids=["no-trailers", "trailers"])
def test_secondary_sort_device_mofs_take_the_generic_merge(require_gpu, provider, checksum):
    job = f"job_s_002{int(checksum)}"
    maps = datagen.secondary_sort(num_maps=9, reducers=2, rows_per_map=600, seed=7)
    ids = publish(provider, job, maps, "device", checksum=checksum)
    conf = dict(DEV, **{"mapred.uda.gpu.round.bytes": 64 << 10})
    recs, st, _ = run_reduce("h", job, ids, 1, datagen.TEXT, codec="zstd", conf=conf, kv_buf_size=8192)
    same_records(recs, expected(maps, 1, datagen.TEXT))
    assert st["merge_path"] == "device-generic" and st["device_decoded_streams"] == 9, st
    assert st["ifile_checksum"] == ("verified" if checksum else "none"), st


@pytest.mark.parametrize("checksum", [False, True], ids=["no-trailers", "trailers"])
def test_host_mofs_staged_path(require_gpu, provider, tmp_path, checksum):
    job = f"job_s_003{int(checksum)}"
    maps = datagen.secondary_sort(num_maps=12, reducers=2, rows_per_map=500, seed=5)
    ids = publish(provider, job, maps, "file", checksum=checksum, tmp_path=tmp_path)
    recs, st, _ = run_reduce("h", job, ids, 1, datagen.TEXT, codec="zstd", conf=GPU, kv_buf_size=8192)
    same_records(recs, expected(maps, 1, datagen.TEXT))
    assert st["backend"] == "gpu" and st["merge_path"].startswith("staged"), st
    assert st["device_descriptors"] == 0 and st["device_decoded_streams"] == 12 and st["device_decoded_blocks"] == 0, st
    assert st["ifile_checksum"] == ("verified" if checksum else "none"), st
    cpu, _, _ = run_reduce("h", job, ids, 1, datagen.TEXT, codec="zstd", kv_buf_size=8192)
    assert [k for k, _ in cpu] == [k for k, _ in recs] and sorted(cpu) == sorted(recs)


@pytest.mark.parametrize("where", ["device", "memory"])
def test_host_decoder_when_device_decompress_is_off(require_gpu, provider, where):
    job = "job_s_004" + where[0]
    maps = datagen.wordcount(num_maps=6, reducers=2, words_per_map=4000, seed=13)
    ids = publish(provider, job, maps, where, checksum=True)
    conf = dict(DEV if where == "device" else GPU, **{"mapred.uda.gpu.decompress": 0})
    recs, st, _ = run_reduce("h", job, ids, 0, datagen.TEXT, codec="zstd", conf=conf, kv_buf_size=8192)
    same_records(recs, expected(maps, 0, datagen.TEXT))
    assert st["backend"] == "gpu" and st["device_decoded_streams"] == 0 and st["device_decoded_blocks"] == 0, st
    assert st["ifile_checksum"] == "verified", st


@pytest.mark.parametrize("where", ["device", "memory"])
def test_combiner_over_zstd_input(require_gpu, provider, where):
    job = "job_s_005" + where[0]
    maps = datagen.wordcount(num_maps=8, reducers=1, words_per_map=5000, seed=19)
    ids = publish(provider, job, maps, where)
    conf = dict(DEV if where == "device" else GPU, **{"mapred.uda.merge.combine": "sum.int"})
    recs, st, _ = run_reduce("h", job, ids, 0, datagen.TEXT, codec="zstd", conf=conf, kv_buf_size=8192)
    assert recs == expected_task(maps, 0, datagen.TEXT, "sum.int")
    assert st["combine"] == "sum.int" and st["device_decoded_streams"] == 8, st


@pytest.mark.parametrize("checksum", [False, True], ids=["no-trailers", "trailers"])
def test_over_budget_hybrid_lpq_merges_decode_zstd(require_gpu, provider, checksum):
    job = f"job_s_006{int(checksum)}"
    maps = datagen.wordcount(num_maps=12, reducers=1, words_per_map=12000, seed=83)
    ids = publish(provider, job, maps, "memory", checksum=checksum)
    conf = dict(GPU, **{"mapred.uda.gpu.merge.bytes": 150_000, "mapred.uda.gpu.spill": "host"})
    recs, st, _ = run_reduce("h", job, ids, 0, datagen.TEXT, codec="zstd", conf=conf, kv_buf_size=8192)
    same_records(recs, expected(maps, 0, datagen.TEXT))
    assert st["lpqs"] >= 2 and st["device_decoded_streams"] == 12 and st["device_decoded_blocks"] == 0, st
    assert st["ifile_checksum"] == ("skipped-over-budget" if checksum else "none"), st  # the hybrid's default
    if checksum:
        conf["mapred.uda.ifile.checksum.over.budget"] = "verify"
        recs, st, _ = run_reduce("h", job, ids, 0, datagen.TEXT, codec="zstd", conf=conf, kv_buf_size=8192)
        same_records(recs, expected(maps, 0, datagen.TEXT))
        assert st["ifile_checksum"] == "verified" and st["device_decoded_streams"] == 12, st


def failing_task(job, ids, partition, conf, match):
    c = UdaConsumer(len(ids), job, f"attempt_{job}_r_{partition:06d}_0", datagen.TEXT, codec="zstd", conf=conf,
                    kv_buf_size=8192)
    for m in ids:
        c.fetch("h", job, m, partition)
    with pytest.raises(UdaFallback, match=match) as e:
        c.wait(60)
    c.close()
    assert c.failure_calls == 1
    assert c.buffers == 0 and c.bytes == 0  # nothing was delivered
    return str(e.value)


@pytest.mark.parametrize("where", ["device", "memory"])
def test_broken_frame_fails_the_task_once(require_gpu, provider, where):
    """With the IFile checksum off the frame itself gives the damage away; under auto the CRC over the partition as
    fetched does: the frame that does not decode is held against the trailer its neighbours show it to have."""
    job = "job_s_007" + where[0]
    maps = datagen.secondary_sort(num_maps=5, reducers=1, rows_per_map=800, seed=3)
    ids = publish(provider, job, maps, where, checksum=True, corrupt=break_descriptor(2, 0))
    base = DEV if where == "device" else GPU
    victim = f"attempt_{job}_m_000002_0"
    why = failing_task(job, ids, 0, dict(base, **OFF), "corrupt zstd frame in map output " + victim)
    assert "reserved descriptor bit" in why, why
    why = failing_task(job, ids, 0, base, "checksum mismatch in map output " + victim)


@pytest.mark.parametrize("where", ["device", "memory"])
def test_flipped_mid_frame_byte_fails_the_task_once_under_the_ifile_checksum(require_gpu, provider, where):
    """A flipped byte in the middle of a frame may land in a Raw literal, which no zstd decoder can notice in a
    frame without a content checksum (Hadoop's have none); the IFile checksum over the partition as fetched does,
    before any record is delivered."""
    job = "job_s_008" + where[0]
    maps = datagen.secondary_sort(num_maps=5, reducers=1, rows_per_map=800, seed=3)
    ids = publish(provider, job, maps, where, checksum=True, corrupt=flip_mid_frame(2, 0))
    victim = f"attempt_{job}_m_000002_0"
    failing_task(job, ids, 0, DEV if where == "device" else GPU, "map output " + victim)


@pytest.mark.parametrize("where", ["device", "memory"])
def test_two_frame_partitions(require_gpu, provider, where):
    job = "job_s_009" + where[0]
    maps = datagen.wordcount(num_maps=4, reducers=1, words_per_map=3000, seed=29)
    ids = publish(provider, job, maps, where, checksum=True, two_frames=True)
    base = DEV if where == "device" else GPU
    why = failing_task(job, ids, 0, base, "holds more than one frame")
    assert "mapred.uda.gpu.decompress=0" in why and "zstd map output attempt_" in why, why
    recs, st, _ = run_reduce("h", job, ids, 0, datagen.TEXT, codec="zstd", conf=dict(base, **{"mapred.uda.gpu.decompress": 0}),
                             kv_buf_size=8192)
    same_records(recs, expected(maps, 0, datagen.TEXT))
    assert st["device_decoded_streams"] == 0 and st["ifile_checksum"] == "verified", st
