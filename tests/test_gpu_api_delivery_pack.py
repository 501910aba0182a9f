"""GPU: bit-packed delivery (colpack) on the C ABI's FIXED10 paths, device_reduce_fixed and
device_reduce_fixed_blocks (csrc/gpu/device_reduce.cc, csrc/gpu/fixed_delivery.cc).

mapred.uda.gpu.delivery.pack = auto | v1 | off changes only what crosses the link: with every value the
sink gets the same buffers (same boundaries, same EOF placement, same count), and their concatenation is
the CPU merge of the runs. Generator records (values 'A'..'Z') pack; records whose value bytes are 0..255
do not (a stride above 0.9 of the record) and travel as they are."""
import functools
import json
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

from uda_amd.bridge import UdaConsumer, UdaProvider, run_reduce
from uda_amd.utils import datagen
from uda_amd.utils.mof import encode_partitions

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GPU = {"mapred.uda.merge.backend": "gpu"}
L = 104
EOF = b"\xff\xff"
MODES = ("auto", "v1", "off")
KV = 8192          # 78 records per buffer
PIECE = 32 << 10   # 4 buffers = 312 records per piece
PIECE_RECS = 312


@functools.lru_cache(maxsize=None)
def _pool():
    """Three sorted runs of 2000 generator records each (record bytes, no EOF), made once."""
    maps = datagen.terasort(num_maps=3, reducers=1, rows_per_map=2000, seed=77)
    return tuple(s[0][:-2] for s in datagen.streams(maps))


def tera_runs(counts):
    """Runs of counts[i] records: prefixes of the pool's sorted runs."""
    return [r[:n * L] for r, n in zip(_pool(), counts)]


def split3(n):
    return [n // 3, n // 3, n - 2 * (n // 3)]


def random_values(runs, above=0, seed=5):
    """Value bytes 0..255 in every record whose first key byte is >= above (the runs stay sorted)."""
    rng = np.random.RandomState(seed)
    out = []
    for r in runs:
        a = np.frombuffer(r, np.uint8).reshape(-1, L).copy()
        sel = a[:, 3] >= above
        a[sel, 14:] = rng.randint(0, 256, size=(int(sel.sum()), 90))
        out.append(a.tobytes())
    return out


def cpu_merge(native, runs):
    out, _ = native.cpu_merge([r + EOF for r in runs], datagen.TEXT, 1 << 20)
    return out


def reduce_all(native, runs, kv=KV, round_bytes=1 << 30, piece=PIECE, modes=MODES):
    """Every mode's (buffers, stats); the buffer lists are equal and concatenate to the CPU merge."""
    over = native.hbm_stats(0)["over"]
    res = {m: native.gpu_device_reduce_fixed(runs, kv, round_bytes, piece, m, 0) for m in modes}
    first = res[modes[0]][0]
    for m in modes:
        bufs, st = res[m]
        assert bufs == first, m
        assert st["buffers"] == len(bufs) and st["bytes"] == sum(len(r) for r in runs)
        assert st["pieces"] == st["packed_pieces"] + st["raw_pieces"]
        assert all(len(b) <= kv for b in bufs)
    assert b"".join(first) == cpu_merge(native, runs)
    assert native.hbm_stats(0)["over"] == over  # nothing allocated outside the task's reservation
    return res


def test_slot_reuse_and_short_tails(require_gpu, native):
    """4 rounds of about 1400 records, 5 pieces each over 4 ring slots; every round ends in a short piece
    and a short buffer."""
    runs = tera_runs(split3(5600))
    res = reduce_all(native, runs, round_bytes=150_000)
    for m in MODES:
        st = res[m][1]
        assert st["rounds"] == 4 and st["pieces"] > 4 * 4, st  # some round reuses a ring slot
    auto, v1, off = (res[m][1] for m in MODES)
    assert auto["packed_pieces"] > 0 and auto["raw_pieces"] == 0 and auto["d2h_bytes"] < auto["bytes"], auto
    assert auto["delta_pieces"] > 0, auto
    assert v1["packed_pieces"] > 0 and v1["raw_pieces"] == 0 and v1["delta_pieces"] == 0, v1
    assert v1["d2h_bytes"] < v1["bytes"], v1
    assert off["d2h_bytes"] == off["bytes"] and off["packed_pieces"] == 0 and off["unpack_ms"] == 0, off
    bufs = res["auto"][0]
    assert sum(1 for b in bufs if len(b) < 78 * L) >= 4  # a short last buffer per round


@pytest.mark.parametrize("n,round_bytes,rounds", [(11 * PIECE_RECS + 7, 1 << 30, 1), (5800, 310_000, 2)])
def test_device_ring_reuse(require_gpu, native, n, round_bytes, rounds):
    """Rounds of more than 2 * 4 pieces: the pieces are packed in groups of 4 into a device ring of two
    groups, so the third group of a round takes the place of the first once that has landed on the host."""
    res = reduce_all(native, tera_runs(split3(n)), round_bytes=round_bytes)
    st = res["auto"][1]
    assert st["rounds"] == rounds and st["pieces"] >= 9 * rounds and st["packed_pieces"] == st["pieces"], st
    assert st["d2h_bytes"] < 0.75 * st["bytes"], st


@pytest.mark.parametrize("tail", [1, 2, 19])
def test_pieces_longer_than_their_records(require_gpu, native, tail):
    """A last piece of 1, 2 or 19 records is longer packed (header, restart table) than plain: ring slots
    and packed regions sized by the piece instead of the bound would be overrun."""
    n = 3 * PIECE_RECS + tail
    res = reduce_all(native, tera_runs(split3(n)))
    st = res["auto"][1]
    assert st["rounds"] == 1 and st["pieces"] == 4 and st["packed_pieces"] == 4, st
    assert st["d2h_bytes"] < st["bytes"]
    # two rounds whose last pieces are that short, with round bounds from the key sample
    reduce_all(native, tera_runs(split3(2 * n)), round_bytes=n * L)


@pytest.mark.parametrize("kv,full", [(78 * L, True), (KV, False)])
def test_eof_placement(require_gpu, native, kv, full):
    """kv_buf a multiple of 104 and the final buffer exactly full: EOF in a buffer of its own; kv_buf with
    room: EOF rides in the final buffer. Both packed."""
    n = 78 * 9  # 9 full buffers: 2 pieces of 4 and one of 1
    res = reduce_all(native, tera_runs(split3(n)), kv=kv, piece=4 * 78 * L)
    bufs, st = res["auto"]
    assert st["packed_pieces"] == st["pieces"] == 3, st
    if full:
        assert len(bufs) == 10 and bufs[-1] == EOF and all(len(b) == kv for b in bufs[:-1])
    else:
        assert len(bufs) == 9 and len(bufs[-1]) == 78 * L + 2 and bufs[-1].endswith(EOF)


@pytest.mark.parametrize("n", [0, 1, 50])
def test_edge_sizes(require_gpu, native, n):
    res = reduce_all(native, tera_runs([n, 0, 0]))
    bufs, st = res["auto"]
    if n == 0:
        assert bufs == [EOF] and st["pieces"] == 0 and st["d2h_bytes"] == 0, st
    else:
        assert len(bufs) == 1 and len(bufs[0]) == n * L + 2 and st["packed_pieces"] == 1, st


def test_raw_pieces(require_gpu, native):
    runs = random_values(tera_runs(split3(4 * PIECE_RECS)))
    res = reduce_all(native, runs)
    st = res["auto"][1]
    assert st["pieces"] == 4 and st["raw_pieces"] == 4 and st["packed_pieces"] == 0, st
    assert st["d2h_bytes"] == st["bytes"]


def test_mixed_rounds(require_gpu, native):
    """Keys below the bound carry generator values, keys above it random ones: the low rounds pack, the
    high rounds do not."""
    runs = random_values(tera_runs(split3(5600)), above=128)
    res = reduce_all(native, runs, round_bytes=150_000)
    st = res["auto"][1]
    assert st["rounds"] == 4 and st["packed_pieces"] > 0 and st["raw_pieces"] > 0, st
    assert st["d2h_bytes"] < st["bytes"]


# ---------------------------------------------------------------- through the C ABI

@functools.lru_cache(maxsize=None)
def _api_maps():
    return datagen.terasort(num_maps=4, reducers=1, rows_per_map=1500, seed=78)


def _expected(maps):
    return sorted((kv for m in maps for kv in m[0]), key=datagen.sort_key(datagen.TEXT))


def _publish(provider, job, maps, codec=None, **kw):
    ids = []
    for i, parts in enumerate(datagen.streams(maps)):
        mid = f"attempt_{job}_m_{i:06d}_0"
        data, index = encode_partitions(parts, codec, **kw)
        provider.add_mof_device(job, mid, data, index, device=0)
        ids.append(mid)
    return ids


@pytest.fixture
def provider():
    p = UdaProvider()
    yield p
    p.close()


def _check_pack_stats(st, pack, nbytes):
    for k in ("gpu_d2h_bytes", "gpu_packed_pieces", "gpu_raw_pieces", "gpu_unpack_ms"):
        assert k in st, k
    if pack == "off":
        assert st["gpu_packed_pieces"] == 0 and st["gpu_d2h_bytes"] == nbytes and st["gpu_raw_pieces"] > 0, st
    else:
        assert st["gpu_packed_pieces"] > 0 and st["gpu_d2h_bytes"] < nbytes, st


def test_api_device_mofs(require_gpu, provider):
    maps = _api_maps()
    ids = _publish(provider, "job_9_0601", maps)
    want = _expected(maps)
    for pack in ("auto", "off"):
        conf = dict(GPU, **{"mapred.uda.gpu.fetch": "device", "mapred.uda.gpu.round.bytes": 150_000,
                            "mapred.uda.gpu.delivery.piece.bytes": PIECE, "mapred.uda.gpu.delivery.pack": pack})
        recs, st, _ = run_reduce("h", "job_9_0601", ids, 0, datagen.TEXT, conf=conf, kv_buf_size=KV)
        assert recs == want, pack
        assert st["merge_path"] == "device-fixed10" and st["rpq_rounds"] > 1, st
        _check_pack_stats(st, pack, len(want) * L)


def test_api_compressed_mofs_streaming_decode(require_gpu, provider):
    maps = _api_maps()
    ids = _publish(provider, "job_9_0602", maps, codec="snappy", block_size=5000)
    want = _expected(maps)
    for pack in ("auto", "off"):
        conf = dict(GPU, **{"mapred.uda.gpu.fetch": "device", "mapred.uda.gpu.round.bytes": 96 << 10,
                            "mapred.uda.gpu.delivery.piece.bytes": PIECE, "mapred.uda.gpu.delivery.pack": pack})
        recs, st, _ = run_reduce("h", "job_9_0602", ids, 0, datagen.TEXT, codec="snappy", conf=conf, kv_buf_size=KV)
        assert recs == want, pack
        assert st["merge_path"] == "device-fixed10-stream" and st["rpq_rounds"] > 4, st
        _check_pack_stats(st, pack, len(want) * L)


def test_api_environment_switch_forces_off(require_gpu, provider, monkeypatch):
    monkeypatch.setenv("UDA_DELIVERY_PACK", "0")
    maps = _api_maps()
    ids = _publish(provider, "job_9_0603", maps)
    conf = dict(GPU, **{"mapred.uda.gpu.fetch": "device", "mapred.uda.gpu.delivery.piece.bytes": PIECE})
    recs, st, _ = run_reduce("h", "job_9_0603", ids, 0, datagen.TEXT, conf=conf, kv_buf_size=KV)
    assert recs == _expected(maps)
    _check_pack_stats(st, "off", len(recs) * L)


@pytest.mark.parametrize("key,value", [("mapred.uda.gpu.delivery.pack", "v3"), ("mapred.uda.gpu.delivery.pack", ""),
                                        ("mapred.uda.gpu.delivery.piece.bytes", "0")])
def test_api_bad_value_fails_init(require_gpu, key, value):
    with pytest.raises(Exception, match=key.replace(".", r"\.")):
        UdaConsumer(1, "job_9_0604", "attempt_job_9_0604_r_000000_0", datagen.TEXT, conf=dict(GPU, **{key: value}))


# ---------------------------------------------------------------- hosted by the merge service

HOSTED_PROVIDER = r"""
import json, sys
sys.path.insert(0, sys.argv[3])
from uda_amd.bridge import UdaProvider
from uda_amd.utils.mof import encode_partitions
p = UdaProvider(transport="tcp", data_port=int(sys.argv[1]))
with open(sys.argv[2]) as f:
    mofs = json.load(f)
for mid, parts in mofs:
    data, index = encode_partitions([bytes.fromhex(x) for x in parts], None)
    p.add_mof_device("job_9_0605", mid, data, index)
print("READY", flush=True)
for line in sys.stdin:  # a line in: the provider's statistics out
    print(p.stats(), flush=True)
p.close()
"""


def _service_counters(stats):
    hs = json.loads(stats)["hbm_store"]
    per = [d["merge_service"] for d in hs["daemon_stats"]] if "daemon_stats" in hs else [hs["merge_service"]]
    return {k: sum(int(m[k]) for m in per) for k in ("sessions", "zero_copy_buffers", "bounced_buffers")}


def test_hosted_task_staging_is_shareable(require_gpu, tmp_path):
    """A task hosted by the node's merge service hands its buffers to the client by reference when they
    lie in shareable pinned memory and through a bounce copy otherwise. 6000 records in buffers of 60 in
    one round: 100 full buffers (10 pieces over 4 ring slots) and, the last being exactly kv_buf, EOF in
    a buffer of its own, which both settings send from the same small heap buffer. So packed delivery
    must bounce exactly as many buffers as unpacked delivery: its unpack staging is part of the ring block."""
    maps = datagen.terasort(num_maps=4, reducers=1, rows_per_map=1500, seed=79)
    payload = [(f"attempt_job_9_0605_m_{i:06d}_0", [p.hex() for p in parts])
               for i, parts in enumerate(datagen.streams(maps))]
    spec = tmp_path / "mofs.json"
    spec.write_text(json.dumps(payload))
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    proc = subprocess.Popen([sys.executable, "-c", HOSTED_PROVIDER, str(port), str(spec), ROOT],
                            stdin=subprocess.PIPE, stdout=subprocess.PIPE, text=True)

    def counters():
        proc.stdin.write("stats\n")
        proc.stdin.flush()
        return _service_counters(proc.stdout.readline())

    try:
        assert proc.stdout.readline().strip() == "READY"
        ids = [mid for mid, _ in payload]
        want = _expected(maps)
        kv = 60 * L
        seen = {}
        before = counters()
        for pack in ("auto", "off"):
            conf = dict(GPU, **{"mapred.uda.gpu.fetch": "device", "mapred.uda.gpu.merge.service": "auto",
                                "mapred.uda.gpu.delivery.piece.bytes": 64 << 10, "mapred.uda.gpu.delivery.pack": pack})
            recs, st, _ = run_reduce("127.0.0.1", "job_9_0605", ids, 0, datagen.TEXT, conf=conf, transport="tcp",
                                     data_port=port, kv_buf_size=kv)
            assert recs == want, pack
            assert st.get("merge_service") is True and st["merge_path"] == "device-fixed10", st
            assert st["buffers"] == 101, st
            _check_pack_stats(st, pack, len(want) * L)
            after = counters()
            seen[pack] = {k: after[k] - before[k] for k in after}
            before = after
        assert seen["auto"]["sessions"] == seen["off"]["sessions"] == 1, seen
        assert seen["auto"]["bounced_buffers"] == seen["off"]["bounced_buffers"], seen
        assert seen["auto"]["zero_copy_buffers"] >= seen["off"]["zero_copy_buffers"] > 0, seen
    finally:
        proc.stdin.close()
        proc.wait(timeout=60)
