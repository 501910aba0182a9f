"""The combiner's further ops on the host (mapred.uda.merge.combine = min.int, max.int, min.long, max.long,
sum.vint, sum.vlong; csrc/engine/combine.cc): the conf parser, the CPU merge against the pure-Python
oracle of tests/combine_ops_cases.py, the values a v op refuses, a loopback reduce task of the CPU backend
over VIntWritable counts, and the streaming reference under ASan + UBSan in a program of its own."""
import os
import shutil
import subprocess

import pytest

import uda_amd
from tests.combine_ops_cases import BAD_VALUES, NEW_OPS, bad_value_runs, expected_task, ops_cases, oracle
from uda_amd import ops
from uda_amd.bridge import UdaConsumer, UdaFallback, UdaProvider, run_reduce
from uda_amd.utils import datagen
from uda_amd.utils.ifile import J2CQueueReader, encode_stream, text, vint_encode
from uda_amd.utils.mof import encode_partitions

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPU = {"mapred.uda.merge.backend": "cpu"}
CASES = list(ops_cases(uda_amd.native().combine_tile()))


def test_combine_ops_native_selftest_under_sanitizers(tmp_path):
    """tests/native/combine_ops_selftest.cc with csrc/engine/combine.cc (and the IFile engine it sits in)
    under ASan + UBSan; never loaded into Python."""
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "combine_ops_selftest")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I" + os.path.join(ROOT, "csrc", "include"),
                    os.path.join(ROOT, "tests", "native", "combine_ops_selftest.cc"),
                    os.path.join(ROOT, "csrc", "engine", "combine.cc"),
                    os.path.join(ROOT, "csrc", "engine", "ifile.cc"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert " 0 failures" in r.stdout


def test_conf_parser_takes_the_six_names_and_rejects_the_rest():
    one = [encode_stream([(text(b"k"), b"\0\0\0\1")])]
    for op in NEW_OPS:
        val = vint_encode(1) if op.startswith("sum.v") else (1).to_bytes(8 if op.endswith("long") else 4, "big")
        body, _ = ops.merge_runs([encode_stream([(text(b"k"), val)])], datagen.TEXT, "cpu", combine=op)
        assert body == encode_stream([(text(b"k"), val)], eof=False)
    for bad in ("sum", "SUM.INT", "sum.float", "min", "max.vint", "sum.vint "):
        with pytest.raises(ValueError, match="none, sum.int or sum.long") as e:
            ops.merge_runs(one, datagen.TEXT, "cpu", combine=bad)
        assert all(op in str(e.value) for op in NEW_OPS)
    for bad in ("sum.float", "SUM.INT", "sum"):  # a task fails INIT
        with pytest.raises(RuntimeError, match="none, sum.int or sum.long"):
            UdaConsumer(1, "job_10_0001", "attempt_job_10_0001_r_000000_0", datagen.TEXT,
                        conf=dict(CPU, **{"mapred.uda.merge.combine": bad}))
    c = UdaConsumer(1, "job_10_0002", "attempt_job_10_0002_r_000000_0", datagen.TEXT,
                    conf=dict(CPU, **{"mapred.uda.merge.combine": "max.long"}))
    c.close()


@pytest.mark.parametrize("name,key_class,op,runs", CASES, ids=[c[0] for c in CASES])
def test_cpu_merge_folds_like_the_oracle(native, name, key_class, op, runs):
    want = oracle(runs, key_class, op)
    body, cuts = ops.merge_runs(runs, key_class, "cpu", kv_buf=256, combine=op)
    assert body == want
    r = J2CQueueReader(max_len=256)
    for b in ops.buffers(body, cuts):
        r.feed(b)
    assert r.eof and encode_stream(r.records, eof=False) == want
    # the binding over the streaming reference, fed the uncombined merge
    plain, _ = ops.merge_runs(runs, key_class, "cpu", kv_buf=256)
    assert native.combine_stream(plain, key_class, op) == want
    assert native.combine_stream(plain + b"\xff\xff", key_class, op) == want + b"\xff\xff"
    if name == "all-distinct-sum.vint":
        assert want == plain
    if name.startswith("non-canonical"):
        assert (text(b"only"), b"\x05") in r.records and (text(b"a"), b"\x06") in r.records


@pytest.mark.parametrize("name", list(BAD_VALUES))
def test_cpu_merge_refuses_the_value(name):
    op, bad, says = BAD_VALUES[name]
    with pytest.raises(RuntimeError, match=says):
        ops.merge_runs(bad_value_runs(op, bad), datagen.TEXT, "cpu", combine=op)


@pytest.fixture
def provider():
    p = UdaProvider()
    yield p
    p.close()


def _publish(provider, job, maps):
    ids = []
    for i, parts in enumerate(datagen.streams(maps)):
        mid = f"attempt_{job}_m_{i:06d}_0"
        data, index = encode_partitions(parts)
        provider.add_mof_memory(job, mid, data, index)
        ids.append(mid)
    return ids


def test_wordcount_value_kinds_draw_the_same_counts():
    a = datagen.wordcount(3, 2, 800, seed=5)
    assert a == datagen.wordcount(3, 2, 800, seed=5, value="int")
    for kind in ("vint", "vlong"):
        b = datagen.wordcount(3, 2, 800, seed=5, value=kind)
        assert [[[(k, vint_encode(int.from_bytes(v, "big"))) for k, v in p] for p in m] for m in a] == b
    with pytest.raises(ValueError):
        datagen.wordcount(1, 1, 1, value="float")


@pytest.mark.parametrize("mode", ["online", "hybrid"])
def test_cpu_task_sums_vint_counts(provider, tmp_path, mode):
    maps = datagen.wordcount(num_maps=23, reducers=2, words_per_map=1500, seed=31, value="vint")
    job = "job_10_010" + str(len(mode))
    ids = _publish(provider, job, maps)
    kw = dict(approach=2, lpq_size=5, local_dirs=(str(tmp_path),)) if mode == "hybrid" else {}
    conf = dict(CPU, **{"mapred.uda.merge.combine": "sum.vint"})
    recs, st, c = run_reduce("h", job, ids, 1, datagen.TEXT, conf=conf, kv_buf_size=4096, **kw)
    want = expected_task(maps, 1, datagen.TEXT, "sum.vint")
    assert recs == want
    assert st["combine"] == "sum.vint" and st["combine_groups"] == len(recs) == st["records"]
    assert st["combine_in_records"] == sum(len(m[1]) for m in maps) > len(recs)
    assert st["bytes_delivered"] == len(encode_stream(want)) == c.bytes and st["buffers"] == c.buffers
    assert any(len(v) > 1 for _, v in recs)  # some sums left one byte
    # the same counts as IntWritable sum to the same numbers
    ints = expected_task(datagen.wordcount(num_maps=23, reducers=2, words_per_map=1500, seed=31), 1, datagen.TEXT, "sum.int")
    assert [(k, vint_encode(int.from_bytes(v, "big"))) for k, v in ints] == want


def test_cpu_task_bad_vint_falls_back_once(provider):
    maps = datagen.terasort(num_maps=3, reducers=1, rows_per_map=200)
    ids = _publish(provider, "job_10_0200", maps)
    conf = dict(CPU, **{"mapred.uda.merge.combine": "sum.vint"})
    c = UdaConsumer(len(ids), "job_10_0200", "attempt_job_10_0200_r_000000_0", datagen.TEXT, conf=conf)
    for m in ids:
        c.fetch("h", "job_10_0200", m, 0)
    with pytest.raises(UdaFallback, match=r"value of 91 bytes \(one VInt expected\)"):
        c.wait(30)
    c.close()
    assert c.failure_calls == 1 and c.bytes == 0
