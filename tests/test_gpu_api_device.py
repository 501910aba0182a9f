"""GPU: the UdaBridge API path with HBM-resident map outputs (descriptor fetch, in-place merge).

The provider registers MOFs that live in device memory; GPU-backend reducers fetch a descriptor
per partition (device address in-process, an IPC handle across processes) and merge the partitions
where they are, delivering through dataFromUda. Oracle: a Python sort of every record.
"""
import json
import os
import subprocess
import sys

import pytest

from uda_amd.bridge import UdaProvider, run_reduce
from uda_amd.utils import datagen
from uda_amd.utils.mof import encode_partitions

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GPU = {"mapred.uda.merge.backend": "gpu"}


def expected(maps, partition, key_class):
    recs = [kv for m in maps for kv in m[partition]]
    return sorted(recs, key=datagen.sort_key(key_class))


def _publish_device(provider, job, maps):
    ids = []
    for i, parts in enumerate(datagen.streams(maps)):
        mid = f"attempt_{job}_m_{i:06d}_0"
        data, index = encode_partitions(parts, None)
        provider.add_mof_device(job, mid, data, index, device=0)
        ids.append(mid)
    return ids


@pytest.fixture
def provider():
    p = UdaProvider()
    yield p
    p.close()


@pytest.mark.parametrize("round_bytes", [1 << 30, 1 << 20])
def test_terasort_device_mofs_merge_in_place(require_gpu, provider, round_bytes):
    maps = datagen.terasort(num_maps=12, reducers=3, rows_per_map=4000, seed=11)
    ids = _publish_device(provider, "job_9_0001", maps)
    conf = dict(GPU, **{"mapred.uda.gpu.fetch": "device", "mapred.uda.gpu.round.bytes": round_bytes})
    for r in range(3):
        recs, st, c = run_reduce("h", "job_9_0001", ids, r, datagen.TEXT, conf=conf, kv_buf_size=64 << 10)
        assert recs == expected(maps, r, datagen.TEXT)
        assert st["merge_path"] == "device-fixed10"
        assert st["device_descriptors"] == 12 and st["host_fetched_bytes"] == 0
        if round_bytes == 1 << 20:
            assert st["rpq_rounds"] > 1  # key-range rounds bound the device memory
    assert json.loads(provider.stats())["descriptors_served"] == 36


def test_generic_keys_device_mofs(require_gpu, provider):
    maps = datagen.wordcount(num_maps=6, reducers=2, words_per_map=3000, seed=3)
    ids = _publish_device(provider, "job_9_0002", maps)
    recs, st, _ = run_reduce("h", "job_9_0002", ids, 1, datagen.TEXT, conf=GPU)
    want = expected(maps, 1, datagen.TEXT)
    kf = datagen.sort_key(datagen.TEXT)
    assert [kf(kv) for kv in recs] == [kf(kv) for kv in want]
    assert sorted(recs) == sorted(want)
    assert st["merge_path"] == "device-generic"


@pytest.mark.parametrize("gen,key_class", [("secondary_sort", datagen.TEXT), ("wordcount", datagen.TEXT),
                                           ("bytes", datagen.BYTES)])
@pytest.mark.parametrize("round_bytes", [64 << 10, 1 << 20])
def test_generic_device_merge_key_range_rounds(require_gpu, provider, gen, key_class, round_bytes):
    """Generic keys over HBM-resident MOFs merged in key-range rounds of at most round_bytes of input:
    the rounds concatenate to the total order (duplicate-heavy keys, long common prefixes, binary
    keys), and the device working set follows the round size, not the partition size."""
    job = f"job_9_02{len(gen)}{round_bytes % 7}"
    if gen == "secondary_sort":
        maps = datagen.secondary_sort(num_maps=9, reducers=1, rows_per_map=3000, seed=41)
    elif gen == "wordcount":
        maps = datagen.wordcount(num_maps=9, reducers=1, words_per_map=4000, seed=41)
    else:
        maps = datagen.bytes_writable(num_maps=9, reducers=1, rows_per_map=2500, seed=41)
    ids = _publish_device(provider, job, maps)
    conf = dict(GPU, **{"mapred.uda.gpu.fetch": "device", "mapred.uda.gpu.round.bytes": round_bytes})
    recs, st, _ = run_reduce("h", job, ids, 0, key_class, conf=conf, kv_buf_size=32 << 10)
    cpu, _, _ = run_reduce("h", job, ids, 0, key_class, kv_buf_size=32 << 10)
    kf = datagen.sort_key(key_class)
    assert [kf(kv) for kv in recs] == [kf(kv) for kv in cpu] and sorted(recs) == sorted(cpu)
    total = st["bytes_fetched"]
    assert st["merge_path"] == "device-generic" and st["device_descriptors"] == 9
    assert st["rpq_rounds"] >= min(4, total // round_bytes), st
    # (the task's workspace comes from the device's pool: after a larger task of another test it holds that
    # task's capacity, so its size says nothing about this task -- the round count above bounds the work
    # per round)


def test_mixed_host_and_device_mofs(require_gpu, provider):
    """Device fetch falls back to bytes for MOFs the provider holds in host memory."""
    maps = datagen.terasort(num_maps=6, reducers=1, rows_per_map=3000, seed=5)
    ids = []
    for i, parts in enumerate(datagen.streams(maps)):
        mid = f"attempt_job_9_0003_m_{i:06d}_0"
        data, index = encode_partitions(parts, None)
        if i % 2:
            provider.add_mof_memory("job_9_0003", mid, data, index)
        else:
            provider.add_mof_device("job_9_0003", mid, data, index)
        ids.append(mid)
    conf = dict(GPU, **{"mapred.uda.gpu.fetch": "device"})
    recs, st, _ = run_reduce("h", "job_9_0003", ids, 0, datagen.TEXT, conf=conf)
    assert recs == expected(maps, 0, datagen.TEXT)
    assert st["device_descriptors"] == 3 and st["host_fetched_bytes"] > 0


def test_auto_mode_keeps_staged_path_for_host_mofs(require_gpu, provider):
    maps = datagen.terasort(num_maps=4, reducers=1, rows_per_map=2000, seed=6)
    ids = []
    for i, parts in enumerate(datagen.streams(maps)):
        mid = f"attempt_job_9_0004_m_{i:06d}_0"
        data, index = encode_partitions(parts, None)
        provider.add_mof_memory("job_9_0004", mid, data, index)
        ids.append(mid)
    recs, st, _ = run_reduce("h", "job_9_0004", ids, 0, datagen.TEXT, conf=GPU)
    assert recs == expected(maps, 0, datagen.TEXT)
    assert st["merge_path"] in ("staged", "staged-progressive")


DEVICE_PROVIDER = r"""
import json, sys
sys.path.insert(0, sys.argv[3])
from uda_amd.bridge import UdaProvider
from uda_amd.utils.mof import encode_partitions
p = UdaProvider(transport="tcp", data_port=int(sys.argv[1]))
with open(sys.argv[2]) as f:
    mofs = json.load(f)
for mid, parts in mofs:
    data, index = encode_partitions([bytes.fromhex(x) for x in parts], None)
    p.add_mof_device("job_9_0005", mid, data, index)
print("READY", flush=True)
sys.stdin.read()
print(p.stats(), flush=True)
p.close()
"""


@pytest.mark.parametrize("service", ["off", "auto"])
def test_cross_process_provider_over_ipc(require_gpu, tmp_path, service):
    """A provider in another process serves descriptors over TCP; the reducer maps the provider's
    HBM with hipIpcOpenMemHandle and merges in place (the registered-MR/rkey analogue). service=off: the
    reducer merges in this process; auto (the default): the provider's node daemon hosts it, and the
    daemon maps the provider's HBM."""
    import socket
    maps = datagen.terasort(num_maps=5, reducers=2, rows_per_map=2000, seed=8)
    payload = [(f"attempt_job_9_0005_m_{i:06d}_0", [p.hex() for p in parts])
               for i, parts in enumerate(datagen.streams(maps))]
    spec = tmp_path / "mofs.json"
    spec.write_text(json.dumps(payload))
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    proc = subprocess.Popen([sys.executable, "-c", DEVICE_PROVIDER, str(port), str(spec), ROOT],
                            stdin=subprocess.PIPE, stdout=subprocess.PIPE, text=True)
    try:
        assert proc.stdout.readline().strip() == "READY"
        ids = [mid for mid, _ in payload]
        conf = dict(GPU, **{"mapred.uda.gpu.fetch": "device", "mapred.uda.gpu.merge.service": service})
        recs, st, _ = run_reduce("127.0.0.1", "job_9_0005", ids, 1, datagen.TEXT, conf=conf, transport="tcp",
                                 data_port=port)
        assert recs == expected(maps, 1, datagen.TEXT)
        brief = {k: st.get(k) for k in ("merge_path", "device_descriptors", "unmapped_descriptors", "unmapped_reason",
                                        "host_fetched_bytes", "merge_service", "descriptor_map_ms")}
        assert st.get("merge_service", False) == (service == "auto"), json.dumps(brief)
        if service == "off":
            assert st["device_descriptors"] == 5 and st["host_fetched_bytes"] == 0, json.dumps(brief)
        else:
            # the daemon (a child of the provider process) maps the provider's HBM where the platform
            # lets it; where hipIpcOpenMemHandle refuses (tools/ipc_lineage_probe.py), the task fetches
            # the bytes instead: every record arrives either way, and the reason is recorded
            assert st["device_descriptors"] + st["unmapped_descriptors"] == 5, json.dumps(brief)
            assert st["device_descriptors"] == 5 or "hipIpcOpenMemHandle" in st["unmapped_reason"], json.dumps(brief)
    finally:
        proc.stdin.close()
        out = proc.stdout.read()
        proc.wait(timeout=60)
    assert json.loads(out.strip().splitlines()[-1])["descriptors_served"] == 5


def test_api_terasort_bench_small(require_gpu, native):
    """The C-ABI-only TeraSort driver: reduce tasks as separate handles, J2C consumers."""
    b = native.ApiTeraSortBench(dict(device=0, maps=6, reducers=3, records_per_map=30000, round_bytes=1 << 20))
    b.setup()
    for validate in (True, False):
        st = b.step(validate)
        assert st["records"] == 6 * 30000
        if validate:
            assert st["order_errors"] == 0
        assert '"merge_path":"device-fixed10"' in st["task0_stats"]


def test_api_bench_two_ranks_share_providers(require_gpu):
    """`bench.py --api --gpus 2 --one-gpu`: two processes, each a MOFSupplier (TCP) with its maps in
    HBM plus reduce tasks that fetch their partition of both ranks' maps as device descriptors (the
    other rank's HBM mapped over hipIpc). Every task's record count is checked against the sum over
    both ranks' maps, key order in the validated step."""
    env = dict(os.environ, MASTER_ADDR="127.0.0.1")
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--full", "--api", "--gpus", "2", "--one-gpu",
                          "--steps", "1", "--warmup", "1", "--rows-per-gpu", "1800000", "--maps-per-gpu", "6",
                          "--reducers", "3", "--round-mb", "16"],
                         capture_output=True, text=True, timeout=110, env=env, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-3000:]
    res = json.loads(out.stdout.strip().splitlines()[-1])
    assert res["ranks"] == 2 and res["validated"] is True
    assert res["config"]["global_batch"] == 2 * 1_800_000
    assert res["task0_stats"]["merge_path"] == "device-fixed10"


@pytest.mark.parametrize("slots", [0, 1, 2, -1])
def test_api_bench_host_mofs_gated(require_gpu, native, slots):
    """Host-resident MOFs through the staged GPU path, with at most `slots` reduce tasks admitted to
    the GPU at once (mapred.uda.gpu.max.concurrent.merges; 0 = no limit, -1 = the default, off): every task
    completes with its full, ordered partition."""
    b = native.ApiTeraSortBench(dict(device=0, maps=6, reducers=4, records_per_map=20000, round_bytes=1 << 20,
                                     host_mofs=True, fetch="host", max_concurrent_merges=slots))
    b.setup()
    st = b.step(True)
    assert st["records"] == 6 * 20000
    assert st["order_errors"] == 0
    t0 = json.loads(st["task0_stats"])
    assert t0["merge_path"] in ("staged", "staged-progressive")
    if slots in (0, -1):
        assert t0["gpu_gate_wait_ms"] == 0


def _publish_files(provider, tmp_path, job, maps):
    from uda_amd.utils.mof import write_mof
    ids = []
    for i, parts in enumerate(datagen.streams(maps)):
        mid = f"attempt_{job}_m_{i:06d}_0"
        path, _ = write_mof(str(tmp_path), mid, parts)
        provider.add_mof_file(job, mid, path)  # found through getPathUda, never registered
        ids.append(mid)
    return ids


@pytest.mark.parametrize("kind", ["terasort", "wordcount"])
def test_provider_hbm_store_serves_file_mofs(require_gpu, tmp_path, kind):
    """Hadoop-written MOF files (resolved through the getPathUda callback) are loaded once into the
    provider's HBM store on first touch and every partition is then served as a device descriptor:
    every reducer merges in place, output identical to the CPU merge, each file read once."""
    p = UdaProvider(conf={"mapred.uda.provider.hbm.bytes": 1 << 30})
    try:
        R = 3
        maps = (datagen.terasort(num_maps=8, reducers=R, rows_per_map=3000, seed=21) if kind == "terasort" else
                datagen.wordcount(num_maps=8, reducers=R, words_per_map=2000, seed=21))
        ids = _publish_files(p, tmp_path, "job_9_0100", maps)
        conf = dict(GPU, **{"mapred.uda.gpu.fetch": "auto"})
        for r in range(R):
            recs, st, _ = run_reduce("h", "job_9_0100", ids, r, datagen.TEXT, conf=conf, kv_buf_size=64 << 10)
            cpu, _, _ = run_reduce("h", "job_9_0100", ids, r, datagen.TEXT, kv_buf_size=64 << 10)
            kf = datagen.sort_key(datagen.TEXT)  # equal keys may tie-break differently: keys + multiset
            assert [kf(kv) for kv in recs] == [kf(kv) for kv in cpu] and sorted(recs) == sorted(cpu), r
            assert st["device_descriptors"] == 8 and st["host_fetched_bytes"] == 0, st
            assert st["merge_path"].startswith("device")
        hs = json.loads(p.stats())["hbm_store"]
        assert hs["loads"] == 8 and hs["hits"] >= 8 * (R - 1) and hs["declined"] == 0, hs
        assert hs["resident_bytes"] == sum(os.path.getsize(tmp_path / m / "file.out") for m in ids), hs
        p.bridge.do_command(__import__("uda_amd").native().form_cmd(6, ["job_9_0100"]))  # JOB_OVER
        hs = json.loads(p.stats())["hbm_store"]
        assert hs["resident_bytes"] == 0 and hs["evictions"] == 8, hs
    finally:
        p.close()


def test_provider_hbm_store_budget_falls_back_to_bytes(require_gpu, tmp_path):
    """A budget that holds only some files: leased entries are never evicted under a reducer, the
    declined MOFs are fetched as bytes, and the output is still exact."""
    maps = datagen.terasort(num_maps=6, reducers=1, rows_per_map=4000, seed=23)
    size = len(datagen.streams(maps)[0][0]) + 64
    p = UdaProvider(conf={"mapred.uda.provider.hbm.bytes": 3 * size})
    try:
        ids = _publish_files(p, tmp_path, "job_9_0101", maps)
        conf = dict(GPU, **{"mapred.uda.gpu.fetch": "device"})
        recs, st, _ = run_reduce("h", "job_9_0101", ids, 0, datagen.TEXT, conf=conf)
        assert recs == expected(maps, 0, datagen.TEXT)
        hs = json.loads(p.stats())["hbm_store"]
        assert 0 < hs["loads"] < 6 and hs["declined"] > 0 and hs["evictions"] == 0, hs
        assert st["device_descriptors"] == hs["loads"] and st["host_fetched_bytes"] > 0, st
    finally:
        p.close()


@pytest.mark.parametrize("streams,local", [(1, 0), (3, 0), (3, 1)])
def test_provider_hbm_store_declines_over_tcp(require_gpu, tmp_path, streams, local):
    """As above, over TCP: a declined descriptor answer carries the partition's length and MOF file on the
    wire, and the declined partitions' bytes come in pipelined chunk requests (mapred.uda.gpu.fetch.bytes.*;
    here 16 KiB chunks, ~26 per partition) from `streams` workers -- or, the provider being on this node
    and the file ours, straight from the file (mapred.uda.gpu.fetch.local.read). The round-5 TCP error ack
    dropped the length and the declined partitions were merged as empty."""
    import socket
    maps = datagen.terasort(num_maps=6, reducers=1, rows_per_map=4000, seed=29)
    size = len(datagen.streams(maps)[0][0]) + 64
    with socket.socket() as so:
        so.bind(("127.0.0.1", 0))
        port = so.getsockname()[1]
    p = UdaProvider(conf={"mapred.uda.provider.hbm.bytes": 3 * size}, transport="tcp", data_port=port)
    try:
        ids = _publish_files(p, tmp_path, "job_9_0102", maps)
        conf = dict(GPU, **{"mapred.uda.gpu.fetch": "device", "mapred.uda.gpu.fetch.bytes.streams": streams,
                            "mapred.uda.gpu.fetch.bytes.chunk": 16384, "mapred.uda.gpu.fetch.local.read": local})
        recs, st, _ = run_reduce("127.0.0.1", "job_9_0102", ids, 0, datagen.TEXT, conf=conf, transport="tcp",
                                 data_port=port, max_buf_kb=16)
        assert recs == expected(maps, 0, datagen.TEXT)
        hs = json.loads(p.stats())["hbm_store"]
        assert 0 < hs["loads"] < 6 and hs["declined"] > 0, hs
        want_bytes = sum(len(part[0]) for part in datagen.streams(maps))
        assert st["device_descriptors"] == hs["loads"] and st["host_fetched_bytes"] > 0, st
        assert st["maps_fetched"] == 6 and st["bytes_fetched"] == want_bytes, st
        assert st["local_read_bytes"] == (st["host_fetched_bytes"] if local else 0), st
    finally:
        p.close()


def test_bench_api_mof_files(require_gpu, tmp_path):
    """bench.py --api --mof-dir: TeraSort with Hadoop-written MOF files through the C ABI."""
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--full", "--api", "--mof-dir", str(tmp_path), "--rows-per-gpu",
           "2000000", "--maps-per-gpu", "4", "--reducers", "4", "--steps", "2", "--warmup", "1"]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    out = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    assert out["validated"] is True and out["mof_files"] is True
    hs = out["provider"]["hbm_store"]
    assert hs["loads"] == 4 and hs["declined"] == 0, hs
    assert out["task0_stats"]["device_descriptors"] == 4
    assert not list(tmp_path.iterdir())  # files removed with the bench


def test_bench_api_secondary_sort_skew(require_gpu):
    """bench.py --api --workload secondary: config #5 through the C ABI (device-generated variable-length
    Text MOFs, 60% of the records in reduce task 0, key-range rounds bounding the merge's HBM)."""
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--full", "--api", "--workload", "secondary", "--rows-per-gpu",
           "6000000", "--maps-per-gpu", "8", "--reducers", "4", "--round-mb", "64", "--steps", "2", "--warmup", "1"]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    out = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    assert out["validated"] is True and out["config"]["model"] == "secondary-sort"
    assert out["task0_stats"]["merge_path"] == "device-generic"
    assert out["max_task_rounds"] > 1 and out["max_task_ws_gb"] > 0
    assert out["config"]["global_batch"] == 6000000


@pytest.mark.parametrize("codec", ["snappy", "lzo"])
@pytest.mark.parametrize("gen", ["terasort", "secondary_sort"])
def test_compressed_device_mofs_decode_in_place(require_gpu, provider, codec, gen):
    """Block-compressed map outputs in the provider's HBM: the reducer walks the block framing on the
    device, decodes (F6) straight from the descriptors and merges; every MOF is a descriptor."""
    job = f"job_9_03{len(codec)}{len(gen)}"
    maps = (datagen.terasort(num_maps=6, reducers=2, rows_per_map=3000, seed=51) if gen == "terasort" else
            datagen.secondary_sort(num_maps=6, reducers=2, rows_per_map=2500, seed=51))
    ids = []
    for i, parts in enumerate(datagen.streams(maps)):
        mid = f"attempt_{job}_m_{i:06d}_0"
        data, index = encode_partitions(parts, codec, block_size=64 << 10)
        provider.add_mof_device(job, mid, data, index, device=0)
        ids.append(mid)
    conf = dict(GPU, **{"mapred.uda.gpu.fetch": "device"})
    for r in range(2):
        recs, st, _ = run_reduce("h", job, ids, r, datagen.TEXT, codec=codec, conf=conf, kv_buf_size=64 << 10)
        want = expected(maps, r, datagen.TEXT)
        kf = datagen.sort_key(datagen.TEXT)
        assert [kf(kv) for kv in recs] == [kf(kv) for kv in want] and sorted(recs) == sorted(want)
        assert st["device_descriptors"] == 6 and st["host_fetched_bytes"] == 0, st
        assert st["device_decoded_blocks"] > 0 and st["merge_path"].startswith("device"), st


@pytest.mark.parametrize("codec", ["snappy", "lzo"])
def test_compressed_terasort_streaming_decode_rounds(require_gpu, provider, codec):
    """compressed TeraSort partitions decoded per key-range round, only the blocks each
    round covers (block first-key index from a prefix decode). Small blocks and rounds put many round
    bounds inside blocks and records across block boundaries; the stream must equal the whole-partition
    decode path's, record for record."""
    job = f"job_9_035{len(codec)}"
    maps = datagen.terasort(num_maps=7, reducers=2, rows_per_map=4000, seed=61)
    ids = []
    for i, parts in enumerate(datagen.streams(maps)):
        mid = f"attempt_{job}_m_{i:06d}_0"
        data, index = encode_partitions(parts, codec, block_size=5000)  # not a multiple of 104
        provider.add_mof_device(job, mid, data, index, device=0)
        ids.append(mid)
    base = dict(GPU, **{"mapred.uda.gpu.fetch": "device", "mapred.uda.gpu.round.bytes": 96 << 10})
    for r in range(2):
        recs, st, _ = run_reduce("h", job, ids, r, datagen.TEXT, codec=codec, conf=base, kv_buf_size=32 << 10)
        assert recs == expected(maps, r, datagen.TEXT)
        assert st["merge_path"] == "device-fixed10-stream" and st["rpq_rounds"] > 4, st
        assert st["device_descriptors"] == 7 and st["device_decoded_blocks"] > 0, st
        whole, st2, _ = run_reduce("h", job, ids, r, datagen.TEXT, codec=codec, kv_buf_size=32 << 10,
                                   conf=dict(base, **{"mapred.uda.gpu.decode.stream": 0}))
        assert st2["merge_path"] == "device-fixed10" and whole == recs, st2


def test_compressed_host_mofs_device_fetch_pipelined(require_gpu, provider):
    """Compressed MOFs in host memory under mapred.uda.gpu.fetch=device: fetched as bytes in pipelined
    chunks (H2D overlapping the next fetch), then decoded and merged on the device."""
    maps = datagen.terasort(num_maps=5, reducers=1, rows_per_map=6000, seed=53)
    ids = []
    for i, parts in enumerate(datagen.streams(maps)):
        mid = f"attempt_job_9_0310_m_{i:06d}_0"
        data, index = encode_partitions(parts, "snappy", block_size=32 << 10)
        provider.add_mof_memory("job_9_0310", mid, data, index)
        ids.append(mid)
    conf = dict(GPU, **{"mapred.uda.gpu.fetch": "device"})
    recs, st, _ = run_reduce("h", "job_9_0310", ids, 0, datagen.TEXT, codec="snappy", conf=conf, max_buf_kb=64)
    assert recs == expected(maps, 0, datagen.TEXT)
    assert st["device_descriptors"] == 0 and st["host_fetched_bytes"] > 0 and st["device_decoded_blocks"] > 0, st


def test_hybrid_task_over_device_mofs_takes_device_path(require_gpu, provider, tmp_path):
    """A hybrid-approach (LPQ/RPQ) reduce task whose map outputs are HBM-resident needs no LPQ spills:
    it merges them in place in key-range rounds."""
    maps = datagen.secondary_sort(num_maps=12, reducers=1, rows_per_map=2000, seed=57)
    ids = _publish_device(provider, "job_9_0320", maps)
    conf = dict(GPU, **{"mapred.uda.gpu.round.bytes": 256 << 10})
    recs, st, _ = run_reduce("h", "job_9_0320", ids, 0, datagen.TEXT, conf=conf, approach=2, lpq_size=4,
                             local_dirs=(str(tmp_path),))
    want = expected(maps, 0, datagen.TEXT)
    kf = datagen.sort_key(datagen.TEXT)
    assert [kf(kv) for kv in recs] == [kf(kv) for kv in want] and sorted(recs) == sorted(want)
    assert st["merge_path"] == "device-generic" and st["device_descriptors"] == 12 and st["lpqs"] == 0, st
    assert st["rpq_rounds"] > 1


@pytest.mark.parametrize("codec", ["snappy", "lzo"])
def test_bench_api_compressed_mofs(require_gpu, codec):
    """bench.py --api --api-codec: compressed TeraSort MOFs in HBM, decoded on the device from the
    descriptors by every reduce task, validated."""
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--full", "--api", "--api-codec", codec, "--rows-per-gpu", "2000000",
           "--maps-per-gpu", "4", "--reducers", "4", "--steps", "2", "--warmup", "1"]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    out = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    assert out["validated"] is True and out["codec"] == codec and 0 < out["compressed_gb"]
    t0 = out["task0_stats"]
    assert t0["device_descriptors"] == 4 and t0["device_decoded_blocks"] > 0, t0
    assert t0["merge_path"] == "device-fixed10-stream", t0
