"""bench.py --full / --dump-outputs and the stream sampler behind the dump.

CPU tier: the sampler keeps exactly the stream bytes of its windows however the stream is cut into
buffers; --full alone turns the validated step on. GPU tier: the sample of a step equals the same
records of the stream a Python sink receives, and two benchmark runs with the same arguments write
the same files."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_stream_sampler_keeps_its_windows_across_buffer_cuts(native):
    rng = np.random.RandomState(7)
    window = 104
    streams = [rng.randint(0, 256, size=n, dtype=np.uint8) for n in (104 * 300 + 2, 104 * 5 + 2, 2)]
    starts = [np.unique(np.concatenate([rng.randint(0, 300, 40), [0, 299]])) * window,
              np.arange(5) * window,           # every record: adjacent windows
              np.zeros(0, np.int64)]           # an empty reducer: the EOF marker only
    s = native.StreamSampler([[int(x) for x in st] for st in starts], window)
    for attempt in range(3):  # the same windows whatever the buffer boundaries
        s.reset()
        for r, stream in enumerate(streams):
            p = 0
            while p < len(stream):
                n = int(rng.randint(1, 1000))
                s.observe(r, stream[p:p + n])
                p += n
        for r, stream in enumerate(streams):
            got = np.asarray(s.data(r))
            assert got.shape == (len(starts[r]), window)
            want = np.stack([stream[a:a + window] for a in starts[r]]) if len(starts[r]) else got
            assert np.array_equal(got, want)
            assert s.stream_bytes(r) == len(stream) and s.captured_bytes(r) == got.size
    with pytest.raises(ValueError):
        native.StreamSampler([[0, 50]], window)  # overlapping windows


def test_validated_step_only_with_full():
    sys.path.insert(0, ROOT)
    try:
        import bench
    finally:
        sys.path.remove(ROOT)
    plain = bench.parse_args(["--gpus", "1", "--steps", "2", "--warmup", "1"])
    assert plain.full is False and plain.validate is False and plain.dump_outputs == ""
    assert bench.parse_args(["--full"]).validate is True
    assert bench.parse_args(["--full", "--no-validate"]).validate is False
    assert bench.parse_args(["--dump-outputs", "d"]).dump_outputs == "d"
    assert bench.main(["--api", "--dump-outputs", "d"]) == 2  # flagship path only, said before any work


@pytest.mark.gpu
def test_sampled_records_are_the_delivered_stream(require_gpu):
    from uda_amd.models.terasort import RECORD_BYTES, TeraSortConfig, TeraSortShuffle
    from uda_amd.parallel.dist import DistContext
    reducers = 4
    cfg = TeraSortConfig(rows_per_gpu=100000, maps_per_rank=5, rounds=3, reducers=reducers, sample_every=64,
                         map_sort=True, kv_buf_bytes=64 << 10, d2h_piece_bytes=256 << 10)
    j = TeraSortShuffle(DistContext(), cfg, device=0)
    j.setup()
    j.sample_outputs(64, seed=cfg.seed)
    counts = list(j.job.reducer_records())
    for r, idx in enumerate(j.sample_index):
        assert idx[0] == 0 and idx[-1] == counts[r] - 1 and len(idx) <= 64 and np.all(np.diff(idx) > 0)
    j.check(j.step())
    first = j.sampled_outputs()
    j.check(j.step())
    second = j.sampled_outputs()
    index = j.sample_index
    streams = [bytearray() for _ in range(reducers)]
    j.use_python_sink(lambda r, b: streams[r].extend(b), with_reducer=True)
    j.check(j.step())
    for r in range(reducers):
        stream = np.frombuffer(bytes(streams[r]), np.uint8)
        assert len(stream) == counts[r] * RECORD_BYTES + 2  # the records and the EOF marker
        want = np.stack([stream[i * RECORD_BYTES:(i + 1) * RECORD_BYTES] for i in index[r]])
        assert np.array_equal(first[r], want) and np.array_equal(second[r], want)


def _bench(out_dir, *extra):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--warmup", "1", "--rows-per-gpu", "200000",
           "--maps-per-gpu", "4", "--reducers", "3", "--rounds", "2", "--d2h-piece-mb", "8", "--pinned-slots", "4",
           "--dump-outputs", str(out_dir), *extra]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-3000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


@pytest.mark.gpu
def test_bench_dumps_the_same_outputs_for_the_same_arguments(require_gpu, tmp_path):
    """A plain run and a --full run with another step count: the same inputs, so the same files; the
    plain run does not run the validated step, and `steps` timed steps make ms_per_step."""
    a = _bench(tmp_path / "a", "--steps", "2")
    b = _bench(tmp_path / "b", "--steps", "1", "--full")
    assert a["steps"] == 2 and a["ms_per_step"] > 0 and a["validated"] is None and a["exchange_errors"] is None
    assert b["steps"] == 1 and b["ms_per_step"] > 0 and b["validated"] is True
    assert a["unit"] == "GB/s" and a["higher_is_better"] is True and a["dtype"] == "bytes"
    names = sorted(os.listdir(tmp_path / "a"))
    assert names == sorted(os.listdir(tmp_path / "b")) == ["record_index.npy", "records.npy", "reducer_records.npy"]
    total = 0
    for n in names:
        x, y = np.load(tmp_path / "a" / n), np.load(tmp_path / "b" / n)
        assert x.dtype in (np.float32, np.float64) and x.dtype == y.dtype
        assert np.array_equal(x, y), n
        total += x.nbytes
    assert total <= 64 << 20
    rec = np.load(tmp_path / "a" / "records.npy")
    idx = np.load(tmp_path / "a" / "record_index.npy")
    assert rec.shape == (len(idx), 104) and rec.max() <= 255 and np.any(rec[:, 2:12] != rec[0, 2:12])
    assert np.load(tmp_path / "a" / "reducer_records.npy").sum() == 200000 // 4 * 4
