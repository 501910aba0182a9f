#!/usr/bin/env python3
"""Benchmarks for the BASELINE.json configs other than the flagship (bench.py).

  wordcount_loopback  uda_standalone wordcount on CPU loopback: provider + R NetMergers in one
                      process through the UdaBridge C ABI (the JNI plumbing path), heap merge.
  wordcount_tcp       the same with the MOFSupplier in another process, over the TCP transport.
  cpu_reference       in-house baseline: the reference algorithm (single-threaded heap k-way merge,
                      write_kv_to_stream packing) on TeraSort runs on this host's CPU.
  secondary_sort      variable-length Text keys with long common prefixes + partition skew: GPU generic
                      merge (F1/F2/F3/F4 kernels) vs the CPU heap merge on the same runs.
  decode              F6 Snappy / LZO1X block decode on the device vs the host decoder; --codec zlib / gzip: the
                      device inflate (one wave per stream, --maps streams) vs the system zlib; --codec zstd: the
                      device zstd decode (one wave per frame) vs libzstd on 16 threads where it loads.
  netmerger           secondary-sort data through provider -> NetMerger -> dataFromUda: CPU heap merge vs
                      GPU backend (online and hybrid LPQ/RPQ).
  aio                 AsyncIO (io_uring / thread pool, O_DIRECT) read bandwidth vs sequential pread.
  spill               TeraSort whose map outputs live in pinned host DRAM (the spill tier used when a
                      job exceeds HBM): rounds are streamed H2D, merged on the GPU, delivered D2H.
  combine             wordcount over HBM-resident MOFs, 16 concurrent reduce tasks, 16 and 64 maps:
                      mapred.uda.merge.combine none vs sum.int (--op: another op; sum.vint runs over
                      VIntWritable counts), and the F4 kernels phase by phase.
                      --vocab N --tasks N --maps N: one low-duplication, few-task shape (several inner
                      rounds per task); --over-budget: the GPU hybrid, skipping against combining.
  key_order           IntWritable keys (non-negative, so both orders deliver the same bytes), 90-byte values: the
                      device merge under mapred.uda.key.order reference vs hadoop (the 8-byte normalized key per
                      record that the numeric path stores and reads), the two alternated.

Each prints one JSON line per result. Data is synthetic (native generators, csrc/engine/datagen.cc).
"""
from __future__ import annotations

import argparse
import json
import sys
import threading
import resource
import time
import os

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def wordcount_loopback(args) -> dict:
    from uda_amd import native
    from uda_amd.bridge import UdaConsumer, UdaProvider
    from uda_amd.utils.datagen import TEXT
    from uda_amd.utils.mof import encode_partitions

    n = native()
    maps, reducers = args.maps, args.reducers
    rows = int(args.gb * 1e9 / maps / 17)  # ~17 B per (word, 1) IFile record
    t0 = time.perf_counter()
    runs = n.generate_runs("wordcount", maps, reducers, rows, 7)
    gen_s = time.perf_counter() - t0
    prov = UdaProvider()
    total = 0
    for m, parts in enumerate(runs):
        data, index = encode_partitions(parts)
        total += len(data) - 2 * len(parts)
        prov.add_mof_memory("job_wc", f"attempt_wc_m_{m:06d}_0", data, index)
    consumers = [UdaConsumer(maps, "job_wc", f"attempt_wc_r_{r:06d}_0", TEXT, keep_records=False)
                 for r in range(reducers)]
    t0 = time.perf_counter()
    for r, c in enumerate(consumers):
        for m in range(maps):
            c.fetch("localhost", "job_wc", f"attempt_wc_m_{m:06d}_0", r)
    for c in consumers:
        c.wait(3600)
    wall = time.perf_counter() - t0
    stats = [c.close() for c in consumers]
    prov.close()
    delivered = sum(s["bytes_delivered"] for s in stats) - 2 * reducers
    assert delivered == total, (delivered, total)
    return {"config": "uda_standalone wordcount CPU loopback", "gb": round(total / 1e9, 3),
            "maps": maps, "reducers": reducers, "wall_s": round(wall, 3),
            "shuffle_merge_gbps": round(total / wall / 1e9, 3), "gen_s": round(gen_s, 1),
            "records": sum(s["records"] for s in stats), "backend": "cpu heap merge, loopback transport"}


TCP_PROVIDER = r"""
import json, sys
sys.path.insert(0, sys.argv[3])
from uda_amd.bridge import UdaProvider
p = UdaProvider(transport="tcp", data_port=int(sys.argv[1]))
for job, mid, path in json.loads(sys.argv[2]):
    p.add_mof_file(job, mid, path)
print("READY", flush=True)
sys.stdin.read()
p.close()
"""


def wordcount_tcp(args) -> dict:
    """wordcount with the MOFSupplier in another process: the socket transport (the reference's
    cross-node RDMA path, here TCP over the host's loopback interface)."""
    import socket
    import subprocess
    import tempfile

    from uda_amd import native
    from uda_amd.bridge import UdaConsumer
    from uda_amd.utils.datagen import TEXT
    from uda_amd.utils.mof import write_mof
    n = native()
    maps, reducers = args.maps, args.reducers
    rows = int(args.gb * 1e9 / maps / 17)
    runs = n.generate_runs("wordcount", maps, reducers, rows, 7)
    tmp = tempfile.mkdtemp(prefix="uda_tcp_", dir=args.dir)
    mofs, total = [], 0
    for m, parts in enumerate(runs):
        mid = f"attempt_tcp_m_{m:06d}_0"
        path, _ = write_mof(tmp, mid, parts)
        mofs.append(("job_tcp", mid, path))
        total += sum(len(p) - 2 for p in parts)
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    prov = subprocess.Popen([sys.executable, "-c", TCP_PROVIDER, str(port), json.dumps(mofs), root],
                            stdin=subprocess.PIPE, stdout=subprocess.PIPE, text=True)
    try:
        assert prov.stdout.readline().strip() == "READY"
        consumers = [UdaConsumer(maps, "job_tcp", f"attempt_tcp_r_{r:06d}_0", TEXT, keep_records=False,
                                 transport="tcp", data_port=port) for r in range(reducers)]
        t0 = time.perf_counter()
        for r, c in enumerate(consumers):
            for _, mid, _ in mofs:
                c.fetch("127.0.0.1", "job_tcp", mid, r)
        for c in consumers:
            c.wait(3600)
        wall = time.perf_counter() - t0
        stats = [c.close() for c in consumers]
    finally:
        prov.stdin.close()
        prov.wait(timeout=60)
    delivered = sum(st["bytes_delivered"] for st in stats) - 2 * reducers
    assert delivered == total, (delivered, total)
    return {"config": "wordcount, MOFSupplier in a separate process, TCP transport", "gb": round(total / 1e9, 3),
            "maps": maps, "reducers": reducers, "wall_s": round(wall, 3),
            "shuffle_merge_gbps": round(total / wall / 1e9, 3)}


def cpu_reference(args) -> dict:
    from uda_amd import native
    n = native()
    rows = int(args.gb * 1e9 / 104 / args.maps)
    runs = [p[0] for p in n.generate_runs("terasort", args.maps, 1, rows, 3)]
    nbytes = sum(len(r) - 2 for r in runs)
    t0 = time.perf_counter()
    out, lens = n.cpu_merge(runs, "org.apache.hadoop.io.Text", 1 << 20)
    dt = time.perf_counter() - t0
    assert len(out) == nbytes + 2
    return {"config": "reference algorithm: 1-thread heap k-way merge (CPU)", "gb": round(nbytes / 1e9, 3),
            "runs": args.maps, "merge_s": round(dt, 3), "merge_gbps": round(nbytes / dt / 1e9, 3),
            "buffers": len(lens)}


def secondary_sort(args) -> dict:
    from uda_amd import native, ops
    n = native()
    rows = int(args.gb * 1e9 / 100 / args.maps)
    gen = n.generate_runs("secondary", args.maps, 2, rows, 5)
    runs = [m[0] for m in gen]  # reducer 0 receives the skewed majority
    nbytes = sum(len(r) - 2 for r in runs)
    # first full-size call: allocates the merger's HBM workspace (cached per process afterwards, as
    # the NetMerger's pooled workspace is across reduce tasks)
    ops.merge_runs(runs, "org.apache.hadoop.io.Text", "gpu")
    cold_ms = ops.last_stats["merge_ms"]
    res = {}
    for dev in ("gpu", "cpu"):
        t0 = time.perf_counter()
        body, cuts = ops.merge_runs(runs, "org.apache.hadoop.io.Text", dev)
        dt = time.perf_counter() - t0
        res[dev] = (dt, body)
        if dev == "gpu":
            dev_ms = ops.last_stats["merge_ms"]
    assert res["gpu"][1] == res["cpu"][1], "GPU and CPU merges differ"
    return {"config": "secondary sort: variable-length Text keys, long common prefixes, 60% skew to reducer 0",
            "gb": round(nbytes / 1e9, 3), "runs": args.maps,
            "gpu_s_incl_h2d_d2h": round(res["gpu"][0], 3), "cpu_heap_s": round(res["cpu"][0], 3),
            "gpu_gbps": round(nbytes / res["gpu"][0] / 1e9, 3), "cpu_gbps": round(nbytes / res["cpu"][0] / 1e9, 3),
            "gpu_device_merge_ms": round(dev_ms, 1), "gpu_device_merge_gbps": round(nbytes / dev_ms / 1e6, 2),
            "gpu_device_merge_first_call_ms": round(cold_ms, 1),
            "byte_identical": True}


def decode(args) -> dict:
    """F6: device block decode of block-compressed IFile runs (secondary-sort data) vs host decode."""
    from uda_amd import native
    n = native()
    if args.codec in ("zlib", "gzip"):
        return decode_zlib(args, n)
    if args.codec == "zstd":
        return decode_zstd(args, n)
    codec = {"snappy": 1, "lzo": 2, "lz4": 3}[args.codec]
    rows = int(args.gb * 1e9 / 100 / args.maps)
    runs = [m[0] for m in n.generate_runs("secondary", args.maps, 1, rows, 5)]
    t0 = time.perf_counter()
    streams = [n.block_compress(codec, r, 256 * 1024) for r in runs]
    comp_s = time.perf_counter() - t0
    raw = sum(len(r) for r in runs)
    comp = sum(len(s) for s in streams)
    n.gpu_block_decode(args.codec, streams[:1])  # warm up
    outs, blocks, ms = n.gpu_block_decode(args.codec, streams)
    assert outs == runs
    t0 = time.perf_counter()
    host = n.block_decompress(codec, streams[0], 1 << 20)
    host_s = (time.perf_counter() - t0) * len(streams)
    assert host == runs[0]
    return {"config": f"F6 device {args.codec} block decode, 256 KiB blocks, secondary-sort IFile data",
            "raw_gb": round(raw / 1e9, 3), "ratio": round(raw / comp, 2), "blocks": blocks,
            "device_decode_ms": round(ms, 1), "device_gbps_raw": round(raw / ms / 1e6, 1),
            "host_1thread_gbps_raw": round(raw / host_s / 1e9, 3), "host_compress_s": round(comp_s, 1)}


def decode_zlib(args, n) -> dict:
    """Device inflate of DefaultCodec partitions, one wave per stream: the launch's raw GB/s for --maps streams
    (64 and 1024 are the recorded shapes) of TeraSort partitions and of wordcount partitions of --gb in all,
    the Adler-32 kernel's rate over the decoded bytes, and the yardstick that is not ours: Python's
    zlib.decompress over the same streams on one core, and that rate x 16.
    --codec gzip: the same partitions as GzipCodec members (gzip.compress, bare header); the launch's time is
    then inflate + the CRC-32 pass over the output, and the yardstick zlib.decompress(s, 31)."""
    import gzip
    import zlib
    gz = args.codec == "gzip"
    wbits = 31 if gz else 15
    out = {"config": f"device {args.codec} inflate, {args.maps} streams, one wave per stream", "streams": args.maps}
    rows = max(1, int(args.gb * 1e9 / 100 / args.maps))
    distinct = min(args.maps, 32)  # (the streams repeat these partitions: the generator is the slow part)
    for kind in ("terasort", "wordcount"):
        parts = [m[0] for m in n.generate_runs(kind, distinct, 1, rows, 5)]
        raws = [parts[i % distinct] for i in range(args.maps)]
        packed = [gzip.compress(p, 6, mtime=0) if gz else zlib.compress(p) for p in parts]
        streams = [packed[i % distinct] for i in range(args.maps)]
        raw = sum(len(r) for r in raws)
        n.gpu_inflate_streams(streams[:1], [len(raws[0])], 0, args.codec)  # warm up
        best = None
        for _ in range(3):
            outs, consumed, ms = n.gpu_inflate_streams(streams, [len(r) for r in raws], 0, args.codec)
            best = ms if best is None else min(best, ms)
        assert outs == raws and consumed == [len(s) for s in streams]
        _, adler_ms = n.gpu_adler32(raws, 0, 0, True)
        _, adler_ms = n.gpu_adler32(raws, 0, 0, True)
        t0 = time.perf_counter()
        for s in packed:
            zlib.decompress(s, wbits)
        host_s = (time.perf_counter() - t0) * args.maps / distinct
        host = raw / host_s / 1e9
        out[kind] = {"raw_gb": round(raw / 1e9, 3), "ratio": round(raw / sum(len(s) for s in streams), 2),
                     ("device_inflate_and_crc_ms" if gz else "device_inflate_and_adler_ms"): round(best, 2), "device_gbps_raw": round(raw / best / 1e6, 2),
                     "adler_ms": round(adler_ms, 2), "adler_gbps": round(raw / adler_ms / 1e6, 1),
                     "system_zlib_1core_gbps_raw": round(host, 3), "system_zlib_x16_gbps_raw": round(host * 16, 2)}
    return out


def decode_zstd(args, n) -> dict:
    """Device zstd decode of ZStandardCodec partitions, one wave per frame: the launch's raw GB/s for --maps frames of
    TeraSort and of wordcount partitions of --gb in all. Where libzstd.so.1 loads, the frames are what it writes at
    level 3 (Hadoop's default: Huffman literals, described tables) and the yardstick is its ZSTD_decompress over
    the same frames on 16 threads (ctypes calls release the GIL); otherwise the frames come from the in-tree
    encoder (Raw literals, Predefined tables) and the yardstick is the in-tree host decoder on one core."""
    import ctypes
    from concurrent.futures import ThreadPoolExecutor
    try:
        lib = ctypes.CDLL("libzstd.so.1")
        for f in ("ZSTD_compressBound", "ZSTD_compress", "ZSTD_decompress"):
            getattr(lib, f).restype = ctypes.c_size_t
    except OSError:
        lib = None

    def lib_compress(raw):
        cap = lib.ZSTD_compressBound(ctypes.c_size_t(len(raw)))
        buf = ctypes.create_string_buffer(cap)
        r = lib.ZSTD_compress(buf, ctypes.c_size_t(cap), raw, ctypes.c_size_t(len(raw)), 3)
        return buf.raw[:r]

    out = {"config": f"device zstd decode, {args.maps} frames, one wave per frame", "streams": args.maps,
           "frames_by": "libzstd level 3" if lib else "in-tree encoder"}
    rows = max(1, int(args.gb * 1e9 / 100 / args.maps))
    distinct = min(args.maps, 32)  # (the frames repeat these partitions: the generator is the slow part)
    for kind in ("terasort", "wordcount"):
        parts = [m[0] for m in n.generate_runs(kind, distinct, 1, rows, 5)]
        raws = [parts[i % distinct] for i in range(args.maps)]
        packed = [lib_compress(p) if lib else n.zstd_compress(p) for p in parts]
        streams = [packed[i % distinct] for i in range(args.maps)]
        raw = sum(len(r) for r in raws)
        n.gpu_zstd_streams(streams[:1], [len(raws[0])])  # warm up
        best = None
        for _ in range(3):
            outs, consumed, _, ms, _ = n.gpu_zstd_streams(streams, [len(r) for r in raws])
            best = ms if best is None else min(best, ms)
        assert outs == raws and consumed == [len(s) for s in streams]
        res = {"raw_gb": round(raw / 1e9, 3), "ratio": round(raw / sum(len(s) for s in streams), 2),
               "device_decode_ms": round(best, 2), "device_gbps_raw": round(raw / best / 1e6, 2)}
        if lib:
            bufs = [ctypes.create_string_buffer(max(len(r), 1)) for r in raws[:16]]

            def one(i):
                for k in range(i, len(streams), 16):
                    lib.ZSTD_decompress(bufs[i], ctypes.c_size_t(len(raws[k])), streams[k], ctypes.c_size_t(len(streams[k])))

            t0 = time.perf_counter()
            with ThreadPoolExecutor(16) as ex:
                list(ex.map(one, range(min(16, len(streams)))))
            res["libzstd_16_threads_gbps_raw"] = round(raw / (time.perf_counter() - t0) / 1e9, 2)
        else:
            t0 = time.perf_counter()
            for s, p in zip(packed, parts):
                n.zstd_decompress(s, len(p))
            res["host_decoder_1core_gbps_raw"] = round(raw / ((time.perf_counter() - t0) * args.maps / distinct) / 1e9, 3)
        out[kind] = res
    return out


def netmerger(args) -> dict:
    """Secondary-sort data through the whole plugin path (provider -> loopback fetch -> NetMerger ->
    dataFromUda): CPU heap merge vs the GPU backend (online, and hybrid LPQ/RPQ with a small device
    budget)."""
    from uda_amd import native
    from uda_amd.bridge import UdaConsumer, UdaProvider
    from uda_amd.utils.datagen import TEXT
    from uda_amd.utils.mof import encode_partitions
    n = native()
    rows = int(args.gb * 1e9 / 100 / args.maps)
    runs = n.generate_runs("secondary", args.maps, 1, rows, 9)
    prov = UdaProvider()
    total = 0
    for m, parts in enumerate(runs):
        data, index = encode_partitions(parts)
        total += len(data) - 2
        prov.add_mof_memory("job_nm", f"attempt_nm_m_{m:06d}_0", data, index)
    out = {"config": "secondary sort through the NetMerger (loopback transport, 1 reducer)",
           "gb": round(total / 1e9, 3), "maps": args.maps}
    variants = [("cpu", {}), ("gpu_cold", {"mapred.uda.merge.backend": "gpu"}),
                ("gpu_second", {"mapred.uda.merge.backend": "gpu"}),
                ("gpu", {"mapred.uda.merge.backend": "gpu"}),
                ("gpu_drains_all", {"mapred.uda.merge.backend": "gpu", "mapred.uda.gpu.fetch.drains": 0}),
                ("gpu_drains8_step8m", {"mapred.uda.merge.backend": "gpu", "mapred.uda.gpu.fetch.drains": 8,
                                        "mapred.uda.gpu.early.h2d.step": 8 << 20}),
                ("gpu_hybrid_first", {"mapred.uda.merge.backend": "gpu",
                                      "mapred.uda.gpu.merge.bytes": max(1 << 20, total // 6),
                                      "mapred.uda.gpu.spill": "host"}),
                ("gpu_hybrid", {"mapred.uda.merge.backend": "gpu",
                                "mapred.uda.gpu.merge.bytes": max(1 << 20, total // 6),
                                "mapred.uda.gpu.spill": "host"}),
                ("gpu_hybrid_lpq", {"mapred.uda.merge.backend": "gpu",
                                    "mapred.uda.gpu.merge.bytes": max(1 << 20, total // 6),
                                    "mapred.uda.gpu.spill": "host", "mapred.uda.gpu.hybrid.direct": 0})]
    for i, (name, conf) in enumerate(variants):
        c = UdaConsumer(args.maps, "job_nm", f"attempt_nm_r_{i:06d}_0", TEXT, conf=conf, keep_records=False)
        r0 = resource.getrusage(resource.RUSAGE_SELF)
        t0 = time.perf_counter()
        for m in range(args.maps):
            c.fetch("localhost", "job_nm", f"attempt_nm_m_{m:06d}_0", 0)
        c.wait(3600)
        wall = time.perf_counter() - t0
        r1 = resource.getrusage(resource.RUSAGE_SELF)
        # CPU seconds the task burned (all threads): the GPU box runs under a 16-CPU CFS quota, and a
        # process that exceeds it inside a 100 ms period is stalled until the next one
        out[name + "_cpu_s"] = round(r1.ru_utime + r1.ru_stime - r0.ru_utime - r0.ru_stime, 3)
        st = c.close()
        print(f"# {name}: {wall * 1e3:.1f} ms, delivered {st['bytes_delivered'] - 2} of {total} "
              f"path={st.get('merge_path')}", file=sys.stderr, flush=True)
        assert st["bytes_delivered"] - 2 == total, (name, st)
        out[name + "_gbps"] = round(total / wall / 1e9, 3)
        out[name + "_merge_ms"] = round(st["merge_ms"], 1)
        out[name + "_fetch_ms"] = round(st["fetch_ms"], 1)
        if name.startswith("gpu"):
            out[name + "_phases_ms"] = {k: round(st["gpu_" + k + "_ms"], 1) for k in ("h2d", "device", "d2h_wait", "sink")}
        if name.startswith("gpu_hybrid"):
            out[name + "_direct"] = st.get("hybrid_direct")
        if name == "gpu_hybrid":
            out["hybrid_lpqs"] = st["lpqs"]
            out["hybrid_rpq_rounds"] = st["rpq_rounds"]
    prov.close()
    out.update(_netmerger_device_mofs(args, runs))
    if args.reducers > 1:
        out.update(_netmerger_concurrent(args, rows))
    return out


def _netmerger_device_mofs(args, runs) -> dict:
    """The same data with HBM-resident MOFs (the provider registers device memory): the reducer fetches
    partition descriptors and merges the partitions where they live, so only the merged output
    crosses PCIe (device fetch, generic-key merge with key-range rounds streamed out)."""
    from uda_amd.bridge import UdaConsumer, UdaProvider
    from uda_amd.utils.datagen import TEXT
    from uda_amd.utils.mof import encode_partitions
    prov = UdaProvider()
    total = 0
    for m, parts in enumerate(runs):
        data, index = encode_partitions(parts)
        total += len(data) - 2
        prov.add_mof_device("job_nmd", f"attempt_nmd_m_{m:06d}_0", data, index)
    out = {}
    conf = {"mapred.uda.merge.backend": "gpu", "mapred.uda.gpu.fetch": "device"}
    for attempt in ("cold", "warm", "warm2"):
        c = UdaConsumer(args.maps, "job_nmd", f"attempt_nmd_r_000000_{attempt}", TEXT, conf=conf, keep_records=False)
        t0 = time.perf_counter()
        for m in range(args.maps):
            c.fetch("localhost", "job_nmd", f"attempt_nmd_m_{m:06d}_0", 0)
        c.wait(3600)
        wall = time.perf_counter() - t0
        st = c.close()
        assert st["bytes_delivered"] - 2 == total, (st["bytes_delivered"], total)
        out[f"gpu_hbm_mofs_{attempt}_gbps"] = round(total / wall / 1e9, 3)
        if attempt != "cold":
            out[f"gpu_hbm_mofs_{attempt}_stats"] = {k: st[k] for k in ("merge_path", "device_descriptors",
                                                                       "host_fetched_bytes", "gpu_device_ms",
                                                                       "gpu_d2h_wait_ms", "merge_ms", "fetch_ms")
                                                   if k in st}
    prov.close()
    return out


def _netmerger_concurrent(args, rows: int) -> dict:
    """The node view of the same path: `reducers` reduce tasks of one job run at once on one GPU (a
    TaskTracker's reduce slots), each its own NetMerger over its partition of every MOF. One task's
    input H2D overlaps another's output D2H, so the node uses both PCIe directions."""
    from uda_amd import native
    from uda_amd.bridge import UdaConsumer, UdaProvider
    from uda_amd.utils.datagen import TEXT
    from uda_amd.utils.mof import encode_partitions
    n, R = native(), args.reducers
    runs = n.generate_runs("secondary", args.maps, R, rows, 11)
    prov = UdaProvider()
    for m, parts in enumerate(runs):
        data, index = encode_partitions(parts)
        prov.add_mof_memory("job_nmc", f"attempt_nmc_m_{m:06d}_0", data, index)
    del runs
    out = {}
    for attempt in ("cold", "warm"):
        cons = [UdaConsumer(args.maps, "job_nmc", f"attempt_nmc_r_{r:06d}_{attempt}", TEXT,
                            conf={"mapred.uda.merge.backend": "gpu"}, keep_records=False) for r in range(R)]
        t0 = time.perf_counter()
        for m in range(args.maps):
            for r, c in enumerate(cons):
                c.fetch("localhost", "job_nmc", f"attempt_nmc_m_{m:06d}_0", r)
        for c in cons:
            c.wait(3600)
        wall = time.perf_counter() - t0
        stats = [c.close() for c in cons]
        total = sum(st["bytes_delivered"] - 2 for st in stats)
        out[f"gpu_{R}tasks_{attempt}_gbps"] = round(total / wall / 1e9, 3)
    out[f"gpu_{R}tasks_gb"] = round(total / 1e9, 3)
    prov.close()
    return out


def hybrid_budget(args) -> dict:
    """BASELINE config #4's mechanism on one GPU: one reduce task whose partition is several times its
    device budget. The map outputs are in host memory (the DRAM tier), mapred.uda.gpu.hbm.budget caps
    the device at --budget-gb and mapred.uda.gpu.merge.bytes at --merge-gb, so the task takes the GPU
    hybrid merge (direct RPQ key-range rounds over the fetched partitions; the reference's LPQ/RPQ,
    src/Merger/MergeManager.cc:202-288). The stream is validated natively (framing, key order, record
    checksum against the generated runs). --ifile-checksum skip | verify: the MOFs carry Hadoop's IFile checksum
    trailer and mapred.uda.ifile.checksum.over.budget is set to that value (none: no trailers, the key absent)."""
    import resource
    from uda_amd import native
    from uda_amd.bridge import UdaConsumer, UdaProvider
    from uda_amd.utils.datagen import TEXT
    from uda_amd.utils.mof import encode_partitions
    n = native()
    rows = int(args.gb * 1e9 / 100 / args.maps)
    trailers = args.ifile_checksum != "none"
    prov = UdaProvider()
    total, want_sum = 0, 0
    for m in range(args.maps):  # one map at a time: the host holds the encoded MOFs, not the runs too
        parts = n.generate_runs("secondary", 1, 1, rows, 1000 + m)[0]
        want_sum = (want_sum + n.ifile_checksum(parts[0])[2]) & 0xFFFFFFFFFFFFFFFF
        data, index = encode_partitions(parts, None, checksum=trailers)
        total += len(data) - 2 - (4 if trailers else 0)
        prov.add_mof_memory("job_hb", f"attempt_hb_m_{m:06d}_0", data, index)
        del parts
        if m % 8 == 7:  # progress (a GPU box takes a silent minute for a hung run)
            print(f"# hybrid_budget: {m + 1}/{args.maps} maps, {total / 1e9:.1f} GB", file=sys.stderr, flush=True)
    budget = int(args.budget_gb * 1e9)
    conf = {"mapred.uda.merge.backend": "gpu", "mapred.uda.gpu.hbm.budget": budget,
            "mapred.uda.gpu.merge.bytes": int(args.merge_gb * 1e9), "mapred.uda.gpu.spill": "host"}
    if trailers:
        conf["mapred.uda.ifile.checksum.over.budget"] = args.ifile_checksum
    c = UdaConsumer(args.maps, "job_hb", "attempt_hb_r_000000_0", TEXT, conf=conf, keep_records=False, validate=True)
    t0 = time.perf_counter()
    for m in range(args.maps):
        c.fetch("localhost", "job_hb", f"attempt_hb_m_{m:06d}_0", 0)
    while not c._done.wait(30):
        print(f"# hybrid_budget: merging, {time.perf_counter() - t0:.0f} s, "
              f"{c.validator.records if c.validator else 0} records delivered", file=sys.stderr, flush=True)
    c.wait(1)
    wall = time.perf_counter() - t0
    st = c.close()
    v = c.validator
    prov.close()
    hs = n.hbm_stats(0)
    out = {"config": "one NetMerger task over host MOFs, partition >> device budget (GPU hybrid)",
           "gb": round(total / 1e9, 3), "maps": args.maps, "budget_gb": args.budget_gb, "merge_gb": args.merge_gb,
           "ratio_partition_to_budget": round(total / budget, 2), "gbps": round(total / wall / 1e9, 3),
           "wall_s": round(wall, 2), "merge_path": st.get("merge_path"), "hybrid_direct": st.get("hybrid_direct"),
           "rpq_rounds": st.get("rpq_rounds"), "lpqs": st.get("lpqs"), "delivered_ok": st["bytes_delivered"] - 2 == total,
           "ledger_peak_gb": round(hs["peak"] / 1e9, 2), "device_peak_gb": round(hs["device_peak"] / 1e9, 2),
           "over_budget_bytes": hs["over"], "max_rss_gb": round(resource.getrusage(resource.RUSAGE_SELF).ru_maxrss / 1e6, 1)}
    if trailers:
        out.update({k: st.get(k) for k in ("ifile_checksum", "checksum_partitions", "gpu_checksum_ms")})
        out["ifile_checksum_over_budget"] = args.ifile_checksum
    out["validation"] = {"records": v.records, "order_errors": v.order_errors, "framing_errors": v.framing_errors,
                         "eof": v.eof, "checksum_ok": v.checksum == want_sum}
    out["validated"] = bool(v.order_errors == 0 and v.framing_errors == 0 and v.eof and v.checksum == want_sum
                            and out["delivered_ok"])
    return out


def aio(args) -> dict:
    """AsyncIO read bandwidth vs a sequential pread loop (the reference's AIOHandler_test)."""
    from uda_amd import native
    path = os.path.join(args.dir, "uda_aio_bench.bin")
    size = int(args.gb * 1e9) // (1 << 20) * (1 << 20)
    out = {"config": "AIO microbenchmark (io_uring, O_DIRECT, 1 MiB blocks)", "gb": round(size / 1e9, 3)}
    for be in ("", "threadpool"):
        r = native().aio_bench(path, size, 1 << 20, 16, True, be)
        out[(r["backend"]) + "_mbps"] = round(r["aio_mbps"], 1)
        out[(r["backend"]) + "_streaming_mbps"] = round(r["aio_streaming_mbps"], 1)
        out["sequential_mbps"] = round(r["sequential_mbps"], 1)
        assert r["ok"]
    # the store loader's pattern: 32 files read round-robin in 16 MiB chunks, 16 in flight
    ib = native().aio_interleave_bench
    out["interleaved_32x16MiB_gbps"] = round(ib(args.dir, 32, size // 32, 16 << 20, 16), 2)
    out["interleaved_32x1MiB_d64_gbps"] = round(ib(args.dir, 32, size // 32, 1 << 20, 64), 2)
    out["interleaved_32x2MiB_d64_gbps"] = round(ib(args.dir, 32, size // 32, 2 << 20, 64), 2)
    out["interleaved_32x4MiB_d32_gbps"] = round(ib(args.dir, 32, size // 32, 4 << 20, 32), 2)
    out["interleaved_32x1MiB_d256_gbps"] = round(ib(args.dir, 32, size // 32, 1 << 20, 256), 2)
    return out


def spill(args) -> dict:
    import torch  # noqa: F401
    from uda_amd.models.terasort import TeraSortConfig, TeraSortShuffle
    from uda_amd.parallel.dist import DistContext
    cfg = TeraSortConfig(rows_per_gpu=int(args.gb * 1e9 / 104), maps_per_rank=args.maps, rounds=args.rounds,
                         store="host", validate=args.validate)
    job = TeraSortShuffle(DistContext(), cfg, device=0)
    job.setup()
    job.step()
    t0 = time.perf_counter()
    st = job.step()
    dt = time.perf_counter() - t0
    job.check(st)
    return {"config": "TeraSort with map outputs in pinned host DRAM (spill tier), 1 GPU",
            "gb": round(st["bytes_in"] / 1e9, 3), "wall_s": round(dt, 3),
            "shuffle_merge_gbps": round(st["bytes_in"] / dt / 1e9, 3),
            "breakdown_ms": {k: round(st[k], 1) for k in ("comm_ms", "merge_ms", "d2h_ms")}}


def radix(args) -> dict:
    """F8 map-side sort: one map output's records (uniform random 10-byte keys) sorted on the device by
    the LSD radix sort + gather (`csrc/gpu/radix.hip`); checked against numpy's stable lexsort."""
    import numpy as np
    from uda_amd import native
    n = int(args.gb * 1e9 / 104)
    rng = np.random.default_rng(11)
    r = np.empty((n, 104), dtype=np.uint8)
    r[:, 0], r[:, 1], r[:, 2], r[:, 13] = 0x0B, 0x5B, 0x0A, 0x5A
    r[:, 3:13] = rng.integers(0, 256, size=(n, 10), dtype=np.uint8)
    r[:, 14:] = ord("A") + (np.arange(90, dtype=np.uint8)[None, :] + r[:, 3:4]) % 26
    out, ms = native().gpu_sort_fixed(r, staged=True)  # the engine's layout: no copy aside
    keys = r[:, 3:13]
    order = np.lexsort(tuple(keys[:, j] for j in range(9, -1, -1)))  # stable, byte 0 most significant
    ok = out == r[order].tobytes()
    # HBM bytes the sort moves: key extract (104 read, 16 write), 10 passes of hist (16) + scatter (32),
    # and the gather (104 + 104 + 16 key read)
    moved = n * (104 + 16 + 10 * 48 + 224)
    return {"config": "F8 device radix sort of one map output (TeraSort records, 10-byte keys)",
            "records": n, "gb": round(n * 104 / 1e9, 3), "sort_ms": round(ms, 2),
            "mrecords_per_s": round(n / ms / 1e3, 1), "gbps_records": round(n * 104 / ms / 1e6, 1),
            "hbm_gbps_est": round(moved / ms / 1e6, 1), "matches_numpy_lexsort": bool(ok)}


def _uniform_wordcount_runs(maps: int, tasks: int, rows: int, vocab: int, seed: int = 7):
    """(word, 1) runs like the native wordcount generator's, but with words drawn uniformly from `vocab`
    (the native one is Zipf over 100 000 words: hundreds of records per key). About vocab * (1 - exp(-R /
    vocab)) distinct keys among the R records of the job: vocab = R / 1.6 leaves about R / 2 groups. Records
    are 17 bytes: Text("w" + 9 digits) -> IntWritable(1), partitioned by word % tasks, sorted."""
    import numpy as np
    out = []
    for m in range(maps):
        w = np.random.default_rng(seed * 1000003 + m).integers(0, vocab, size=rows, dtype=np.int64)
        parts = []
        for r in range(tasks):
            k = np.sort(w[w % tasks == r])
            rec = np.zeros((len(k), 17), dtype=np.uint8)
            rec[:, 0], rec[:, 1], rec[:, 2], rec[:, 3], rec[:, 16] = 0x0B, 0x04, 0x0A, ord("w"), 1
            for j in range(9):
                rec[:, 12 - j] = 48 + (k // 10 ** j) % 10
            parts.append(rec.tobytes() + b"\xff\xff")
        out.append(parts)
    return out


def _vint_count_runs(runs):
    """The wordcount runs above (fixed-size records, IntWritable(1) values) with VIntWritable(1) values
    instead: the same records and order, three bytes shorter each."""
    import numpy as np
    out = []
    for parts in runs:
        conv = []
        for p in parts:
            body = np.frombuffer(p, dtype=np.uint8)[:-2]
            if len(body) == 0:
                conv.append(bytes(p))
                continue
            size = 2 + int(body[0]) + 4  # one-byte key and value lengths, 4 value bytes
            assert body[1] == 4 and len(body) % size == 0
            rec = body.reshape(-1, size)
            assert (rec[:, -4:] == (0, 0, 0, 1)).all()
            v = np.ascontiguousarray(rec[:, :size - 3])
            v[:, 1] = 1
            v[:, -1] = 1
            conv.append(v.tobytes() + b"\xff\xff")
        out.append(conv)
    return out


def _combine_tasks(n, maps: int, tasks: int, rows: int, op: str, steps: int, warmup: int, vocab: int = 0,
                   over_budget: str = "", lpq: bool = False, value: str = "int") -> dict:
    """`tasks` concurrent reduce tasks over HBM-resident wordcount MOFs, `warmup` + `steps` times.
    over_budget ("skip" | "combine"): the MOFs in host memory instead and mapred.uda.gpu.merge.bytes at a
    quarter of a task's input, so every task takes the over-budget GPU hybrid (lpq: with LPQ spills in DRAM
    instead of RPQ rounds straight over the partitions)."""
    from uda_amd.bridge import UdaConsumer, UdaProvider
    from uda_amd.utils.datagen import TEXT
    from uda_amd.utils.mof import encode_partitions
    runs = _uniform_wordcount_runs(maps, tasks, rows, vocab) if vocab else n.generate_runs("wordcount", maps, tasks, rows, 7)
    if value == "vint":
        runs = _vint_count_runs(runs)
    prov = UdaProvider()
    total = 0
    for m, parts in enumerate(runs):
        data, index = encode_partitions(parts)
        total += len(data) - 2 * len(parts)
        if over_budget:
            prov.add_mof_memory("job_cb", f"attempt_cb_m_{m:06d}_0", data, index)
        else:
            prov.add_mof_device("job_cb", f"attempt_cb_m_{m:06d}_0", data, index)
    del runs
    conf = {"mapred.uda.merge.backend": "gpu", "mapred.uda.gpu.fetch": "device", "mapred.uda.merge.combine": op}
    if over_budget:
        conf = {"mapred.uda.merge.backend": "gpu", "mapred.uda.merge.combine": op, "mapred.uda.gpu.spill": "host",
                "mapred.uda.gpu.merge.bytes": total // tasks // 4, "mapred.uda.merge.combine.over.budget": over_budget}
        if lpq:
            conf["mapred.uda.gpu.hybrid.direct"] = 0
    gbps, last = [], None
    for step in range(warmup + steps):
        cons = [UdaConsumer(maps, "job_cb", f"attempt_cb_r_{r:06d}_{step}", TEXT, conf=conf, keep_records=False)
                for r in range(tasks)]
        t0 = time.perf_counter()
        for m in range(maps):
            for r, c in enumerate(cons):
                c.fetch("localhost", "job_cb", f"attempt_cb_m_{m:06d}_0", r)
        for c in cons:
            c.wait(3600)
        wall = time.perf_counter() - t0
        last = [c.close() for c in cons]
        if step >= warmup:
            gbps.append(total / wall / 1e9)
    prov.close()
    mean = lambda k: round(sum(st[k] for st in last) / len(last), 2)  # noqa: E731
    return {"input_gb": round(total / 1e9, 3), "input_gbps": [round(x, 2) for x in sorted(gbps)],
            "input_gbps_min_med_max": [round(min(gbps), 2), round(sorted(gbps)[len(gbps) // 2], 2), round(max(gbps), 2)],
            "bytes_delivered": sum(st["bytes_delivered"] for st in last), "records": sum(st["records"] for st in last),
            "combine": sorted({st.get("combine", "none") for st in last}),
            "merge_path": sorted({st["merge_path"] for st in last}),
            "combine_in_records": sum(st.get("combine_in_records", 0) for st in last),
            "combine_groups": sum(st.get("combine_groups", 0) for st in last),
            "merge_rounds": sum(st.get("merge_rounds", 0) for st in last),
            "rpq_rounds": sum(st.get("rpq_rounds", 0) for st in last), "lpqs": sum(st.get("lpqs", 0) for st in last),
            "spill_bytes": sum(st.get("spill_bytes", 0) for st in last),
            "task_d2h_wait_ms": [round(st["gpu_d2h_wait_ms"], 2) for st in last][:16],
            "task_mean_ms": {k: mean(k) for k in ("gpu_device_ms", "gpu_d2h_wait_ms", "gpu_sink_ms", "merge_ms")}}


def combine_kernels(args) -> dict:
    """One task's runs through ops.merge_runs with UDA_GM_PROFILE set by the caller: prints the merger's
    phase lines on stderr (the whole path: every F4 kernel is a phase of its own)."""
    from uda_amd import native, ops
    from uda_amd.utils.datagen import TEXT
    rows = int(args.gb * 1e9 / args.maps / 17)
    runs = [p[0] for p in native().generate_runs("wordcount", args.maps, args.reducers, rows, 7)]
    out = {}
    for op in ("none", "sum.int"):
        for _ in range(3):
            body, _ = ops.merge_runs(runs, TEXT, "gpu", combine=op)
        out[op] = {"records_in": ops.last_stats["records_in"], "records": ops.last_stats["records"], "bytes": len(body)}
    return out


def combine(args) -> dict:
    """Reduce-side combiner (mapred.uda.merge.combine) on a wordcount-shaped job: 16 concurrent reduce
    tasks over HBM-resident MOFs of 16 and of 64 maps, `none` against `sum.int`, five steps each after two
    warm-ups; then the F4 kernels of one task's merge, phase by phase, from a child process under
    UDA_GM_PROFILE (each phase is synchronized: kernel time plus one launch and sync)."""
    import re
    import subprocess
    from uda_amd import native
    n = native()
    tasks = args.tasks or 16
    cop = args.op
    # the v ops run over the same records with VIntWritable counts (three bytes shorter each)
    value = "vint" if cop in ("sum.vint", "sum.vlong") else "int"
    out = {"config": f"wordcount ({value} counts), {tasks} reduce tasks over HBM-resident MOFs, combine none vs {cop}",
           "tasks": tasks, "op": cop}
    if args.over_budget:
        # one shape, sum.int: the over-budget hybrid delivering the uncombined stream against combining
        rows = int(args.gb * 1e9 / args.maps / 17)
        out["config"] = f"wordcount, {tasks} reduce task(s) over host MOFs, device budget a quarter of the input"
        for mode in ("skip", "combine"):
            out[f"over_budget_{mode}"] = _combine_tasks(n, args.maps, tasks, rows, cop, steps=5, warmup=2,
                                                        vocab=args.vocab, over_budget=mode, lpq=args.lpq, value=value)
            print(f"# over budget, {mode}: {json.dumps(out[f'over_budget_{mode}'])}", file=sys.stderr, flush=True)
        return out
    shaped = bool(args.vocab or args.tasks)  # --vocab / --tasks: that one shape (--maps), task level only
    for maps in ((args.maps,) if shaped else (16, 64)):
        rows = int(args.gb * 1e9 / maps / 17)
        for op in ("none", cop):
            r = _combine_tasks(n, maps, tasks, rows, op, steps=5, warmup=2, vocab=args.vocab, value=value)
            print(f"# maps={maps} {op}: {json.dumps(r)}", file=sys.stderr, flush=True)
            out[f"maps{maps}_{op}"] = r
        a, b = out[f"maps{maps}_none"], out[f"maps{maps}_{cop}"]
        out[f"maps{maps}_records_per_group"] = round(b["combine_in_records"] / max(1, b["combine_groups"]), 1)
        out[f"maps{maps}_delivered_ratio"] = round(a["bytes_delivered"] / max(1, b["bytes_delivered"]), 1)
        if shaped or cop != "sum.int":  # (the kernel phases are sum.int's)
            continue
        # kernel phases of one task's merge (last of three calls per op)
        env = dict(os.environ, UDA_GM_PROFILE="1")
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "combine_kernels", "--gb", str(args.gb),
                            "--maps", str(maps), "--reducers", "16"], env=env, capture_output=True, text=True,
                           timeout=600)
        lines = [ln for ln in p.stderr.splitlines() if ln.startswith("[GM profile]")]
        if p.returncode != 0 or len(lines) != 6:
            raise RuntimeError("combine_kernels failed: " + p.stderr[-2000:])
        ph = {}
        for op, ln in (("none", lines[2]), ("sum.int", lines[5])):
            ph[op] = {k: float(v) for k, v in re.findall(r"(f[34]c?_\w+)=([0-9.]+)ms", ln)}
        out[f"maps{maps}_kernel_phases_ms"] = ph
        base = sum(ph["none"].get(k, 0) for k in ("f4_record_sizes", "f4_scan", "f4_gather_var"))
        new = sum(ph["sum.int"].get(k, 0) for k in ("f4c_heads", "f4c_group_scan", "f4c_sums"))
        out[f"maps{maps}_heads_plus_sums_over_plain_f4"] = round(new / base, 2) if base else None
        out[f"maps{maps}_one_task"] = json.loads(p.stdout.strip().splitlines()[-1])
    return out


def checksum(args) -> dict:
    """IFile checksum trailers (mapred.uda.ifile.checksum). First the CRC32 kernels alone: 16 ranges of equal
    size filling --gb, next to launch_batched_copy of the same bytes in the same process (hipEvents around
    each launch, 3 warm-ups, 10 repetitions). Then 16 concurrent reduce tasks over HBM-resident
    TeraSort-shaped MOFs that carry trailers, `auto` (verified on the device) against `off` (stripped only):
    2 warm-up steps of each, then 5 steps of each, alternating."""
    from uda_amd import native
    from uda_amd.bridge import UdaConsumer, UdaProvider
    from uda_amd.utils.datagen import TEXT
    from uda_amd.utils.mof import encode_partitions
    n = native()
    tasks = args.tasks or 16
    out = {"config": f"IFile checksum: CRC32 kernel vs batched copy; {tasks} TeraSort tasks over HBM MOFs, auto vs off"}
    part = int(args.gb * 1e9 / 16) & ~255
    k = n.gpu_crc32_bench(16, part, 3, 10)
    gbps = lambda ms: k["bytes"] / (ms * 1e-3) / 1e9  # noqa: E731
    crc, cpy = sorted(gbps(ms) for ms in k["crc_ms"]), sorted(gbps(ms) for ms in k["copy_ms"])
    out["kernel"] = {"bytes": k["bytes"], "ranges": 16, "repeatable": k["repeatable"],
                     "crc32_gbps_min_med_max": [round(crc[0], 1), round(crc[len(crc) // 2], 1), round(crc[-1], 1)],
                     "batched_copy_gbps_min_med_max": [round(cpy[0], 1), round(cpy[len(cpy) // 2], 1), round(cpy[-1], 1)],
                     "crc32_over_copy": round(crc[len(crc) // 2] / cpy[len(cpy) // 2], 2)}
    print(f"# kernel: {json.dumps(out['kernel'])}", file=sys.stderr, flush=True)
    rows = int(args.gb * 1e9 / args.maps / 104)  # per map, spread over the tasks' partitions
    runs = n.generate_runs("terasort", args.maps, tasks, rows, 7)
    prov = UdaProvider()
    total = 0
    for m, parts in enumerate(runs):
        data, index = encode_partitions(parts, checksum=True)
        total += len(data) - 6 * len(parts)
        prov.add_mof_device("job_ck", f"attempt_ck_m_{m:06d}_0", data, index)
    del runs
    base = {"mapred.uda.merge.backend": "gpu", "mapred.uda.gpu.fetch": "device"}
    res = {"auto": [], "off": []}
    last = {}
    for step in range(2 + 5):
        for mode in ("auto", "off"):
            conf = dict(base, **{"mapred.uda.ifile.checksum": mode})
            cons = [UdaConsumer(args.maps, "job_ck", f"attempt_ck_r_{r:06d}_{step}{mode}", TEXT, conf=conf, keep_records=False)
                    for r in range(tasks)]
            t0 = time.perf_counter()
            for m in range(args.maps):
                for r, c in enumerate(cons):
                    c.fetch("localhost", "job_ck", f"attempt_ck_m_{m:06d}_0", r)
            for c in cons:
                c.wait(3600)
            wall = time.perf_counter() - t0
            last[mode] = [c.close() for c in cons]
            if step >= 2:
                res[mode].append(total / wall / 1e9)
    prov.close()
    out["input_gb"] = round(total / 1e9, 3)
    for mode in ("auto", "off"):
        st = last[mode]
        out[mode] = {"input_gbps": [round(x, 2) for x in sorted(res[mode])],
                     "input_gbps_min_max": [round(min(res[mode]), 2), round(max(res[mode]), 2)],
                     "ifile_checksum": sorted({s["ifile_checksum"] for s in st}),
                     "merge_path": sorted({s["merge_path"] for s in st}),
                     "checksum_partitions": sum(s["checksum_partitions"] for s in st),
                     "checksum_bytes": sum(s["checksum_bytes"] for s in st),
                     "task_gpu_checksum_ms_mean": round(sum(s["gpu_checksum_ms"] for s in st) / len(st), 3),
                     "task_merge_ms_mean": round(sum(s["merge_ms"] for s in st) / len(st), 2)}
    return out


def key_order(args) -> dict:
    """The generic device merge of IntWritable-keyed runs under both key orders. Keys are non-negative, where
    memcmp and the signed order agree, so the two merges must deliver the same bytes."""
    import numpy as np

    from uda_amd import ops
    INT = "org.apache.hadoop.io.IntWritable"
    rows = int(args.gb * 1e9 / 96 / args.maps)  # record: 2 header bytes, 4 key bytes, 90 value bytes
    rng = np.random.default_rng(17)
    runs = []
    for _ in range(args.maps):
        keys = np.sort(rng.integers(0, 1 << 31, size=rows, dtype=np.uint32))
        rec = rng.integers(0, 256, size=(rows, 96), dtype=np.uint8)
        rec[:, 0], rec[:, 1] = 4, 90
        rec[:, 2:6] = keys.astype(">u4").view(np.uint8).reshape(rows, 4)
        runs.append(rec.tobytes() + b"\xff\xff")
    nbytes = sum(len(r) - 2 for r in runs)
    orders = ("reference", "hadoop")
    body = {}
    for o in orders:  # first full-size calls: the merger's workspace, and the normalized-key buffer
        body[o], _ = ops.merge_runs(runs, INT, "gpu", key_order=o)
    assert body["reference"] == body["hadoop"], "the two orders differ on non-negative keys"
    reps = max(3, args.rounds)
    dev = {o: [] for o in orders}
    wall = {o: [] for o in orders}
    for _ in range(reps):
        for o in orders:
            t0 = time.perf_counter()
            ops.merge_runs(runs, INT, "gpu", key_order=o)
            wall[o].append(time.perf_counter() - t0)
            dev[o].append(ops.last_stats["merge_ms"])
    med = lambda v: sorted(v)[len(v) // 2]
    out = {"config": "IntWritable keys >= 0, 90-byte values: device merge under mapred.uda.key.order reference vs hadoop",
           "gb": round(nbytes / 1e9, 3), "runs": args.maps, "records": rows * args.maps, "reps": reps, "byte_identical": True}
    for o in orders:
        out[o] = {"device_merge_ms_median": round(med(dev[o]), 2), "device_merge_ms_min": round(min(dev[o]), 2),
                  "device_merge_ms_max": round(max(dev[o]), 2), "device_merge_gbps": round(nbytes / med(dev[o]) / 1e6, 2),
                  "s_incl_h2d_d2h_median": round(med(wall[o]), 3)}
    out["hadoop_over_reference_device_ms"] = round(med(dev["hadoop"]) / med(dev["reference"]), 3)
    return out


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("config", choices=["wordcount_loopback", "wordcount_tcp", "cpu_reference", "secondary_sort", "spill", "decode", "aio",
                                       "netmerger", "radix", "hybrid_budget", "combine", "combine_kernels", "checksum", "key_order"])
    ap.add_argument("--dir", default="/tmp")
    ap.add_argument("--codec", default="snappy", choices=["snappy", "lzo", "lz4", "zlib", "gzip", "zstd"])
    ap.add_argument("--gb", type=float, default=1.0)
    ap.add_argument("--maps", type=int, default=16)
    ap.add_argument("--reducers", type=int, default=4)
    ap.add_argument("--rounds", type=int, default=8)
    ap.add_argument("--validate", action="store_true")
    ap.add_argument("--budget-gb", type=float, default=10.0, help="hybrid_budget: mapred.uda.gpu.hbm.budget")
    ap.add_argument("--merge-gb", type=float, default=8.0, help="hybrid_budget: mapred.uda.gpu.merge.bytes")
    ap.add_argument("--ifile-checksum", default="none", choices=["none", "skip", "verify"],
                    help="hybrid_budget: MOFs with IFile checksum trailers under "
                         "mapred.uda.ifile.checksum.over.budget=skip | verify (none: no trailers)")
    ap.add_argument("--vocab", type=int, default=0,
                    help="combine: words drawn uniformly from this many (default: the Zipf generator's 100 000)")
    ap.add_argument("--tasks", type=int, default=0, help="combine: concurrent reduce tasks (default 16)")
    ap.add_argument("--op", default="sum.int",
                    help="combine: the mapred.uda.merge.combine op measured against none (default sum.int); "
                         "sum.vint / sum.vlong run over the same wordcount with VIntWritable counts")
    ap.add_argument("--lpq", action="store_true", help="combine --over-budget: mapred.uda.gpu.hybrid.direct=0 (LPQ spills)")
    ap.add_argument("--over-budget", action="store_true",
                    help="combine: host MOFs under a device budget of a quarter of a task's input, "
                         "mapred.uda.merge.combine.over.budget skip vs combine")
    a = ap.parse_args()
    fn = globals()[a.config]
    out = fn(a)
    print(json.dumps(out), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
