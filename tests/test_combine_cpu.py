"""The reduce-side combiner on the host (mapred.uda.merge.combine = sum.int / sum.long): the streaming
reference (csrc/engine/combine.cc) under ASan + UBSan in a program of its own, the CPU merge against
a pure-Python oracle (tests/combine_cases.py), and reduce tasks of the CPU backend, online and hybrid."""
import os
import shutil
import subprocess

import pytest

import uda_amd
from tests.combine_cases import combine_records, expected_task, huge_key_runs, merged_records, ops_cases, oracle
from uda_amd import ops
from uda_amd.bridge import UdaConsumer, UdaFallback, UdaProvider, run_reduce
from uda_amd.utils import datagen
from uda_amd.utils.ifile import J2CQueueReader, encode_stream, text
from uda_amd.utils.mof import encode_partitions

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPU = {"mapred.uda.merge.backend": "cpu"}


def test_combine_native_selftest_under_sanitizers(tmp_path):
    """tests/native/combine_selftest.cc with csrc/engine/combine.cc (and the IFile engine it sits in)
    under ASan + UBSan; never loaded into Python."""
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "combine_selftest")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I" + os.path.join(ROOT, "csrc", "include"),
                    os.path.join(ROOT, "tests", "native", "combine_selftest.cc"),
                    os.path.join(ROOT, "csrc", "engine", "combine.cc"),
                    os.path.join(ROOT, "csrc", "engine", "ifile.cc"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert " 0 failures" in r.stdout


CASES = list(ops_cases(uda_amd.native().combine_tile()))


@pytest.mark.parametrize("name,key_class,op,runs", CASES, ids=[c[0] for c in CASES])
def test_cpu_merge_combines_like_the_oracle(native, name, key_class, op, runs):
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


def test_cpu_merge_huge_keys_stay_three_groups():
    runs = huge_key_runs()
    body, _ = ops.merge_runs(runs, datagen.TEXT, "cpu", kv_buf=1 << 20, combine="sum.int")
    assert body == oracle(runs, datagen.TEXT, "sum.int")
    assert [int.from_bytes(v, "big") for _, v in merged_records([body], datagen.TEXT)] == [3, 3, 3]


def test_none_and_unset_are_the_plain_merge():
    runs = [s[0] for s in datagen.streams(datagen.wordcount(5, 1, 1500))]
    plain = ops.merge_runs(runs, datagen.TEXT, "cpu", kv_buf=4096)
    assert ops.merge_runs(runs, datagen.TEXT, "cpu", kv_buf=4096, combine="none") == plain
    assert plain[0] != ops.merge_runs(runs, datagen.TEXT, "cpu", kv_buf=4096, combine="sum.int")[0]


def test_wrong_value_length_and_unknown_op_raise():
    runs = [encode_stream([(text(b"a"), b"\0\0\0\1"), (text(b"bad-key"), b"12345")]), encode_stream([(text(b"a"), b"\0\0\0\2")])]
    with pytest.raises(RuntimeError, match=r"value of 5 bytes.*bad-key"):
        ops.merge_runs(runs, datagen.TEXT, "cpu", combine="sum.int")
    with pytest.raises(RuntimeError, match=r"value of 4 bytes \(8 expected\)"):
        ops.merge_runs(runs[1:], datagen.TEXT, "cpu", combine="sum.long")
    with pytest.raises(ValueError, match="none, sum.int or sum.long"):
        ops.merge_runs(runs, datagen.TEXT, "cpu", combine="sum")


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


@pytest.mark.parametrize("mode", ["online", "hybrid"])
def test_cpu_task_delivers_one_record_per_key(provider, tmp_path, mode):
    maps = datagen.wordcount(num_maps=23, reducers=2, words_per_map=1500, seed=31)
    job = "job_7_000" + str(len(mode))
    ids = _publish(provider, job, maps)
    kw = dict(approach=2, lpq_size=5, local_dirs=(str(tmp_path),)) if mode == "hybrid" else {}
    conf = dict(CPU, **{"mapred.uda.merge.combine": "sum.int"})
    recs, st, c = run_reduce("h", job, ids, 1, datagen.TEXT, conf=conf, kv_buf_size=4096, **kw)
    want = expected_task(maps, 1, datagen.TEXT, "sum.int")
    assert recs == want
    assert st["combine"] == "sum.int" and st["combine_groups"] == len(recs) == st["records"]
    assert st["combine_in_records"] == sum(len(m[1]) for m in maps) > len(recs)
    assert st["bytes_delivered"] == len(encode_stream(want)) == c.bytes and st["buffers"] == c.buffers
    if mode == "hybrid":
        assert st["lpqs"] == 5
    # none and an unset key: the same stream, which is the uncombined merge (a task breaks ties between
    # maps by their arrival, so equal keys compare as multisets)
    r_none, st_none, _ = run_reduce("h", job, ids, 1, datagen.TEXT,
                                    conf=dict(CPU, **{"mapred.uda.merge.combine": "none"}), kv_buf_size=4096, **kw)
    r_unset, st_unset, _ = run_reduce("h", job, ids, 1, datagen.TEXT, conf=CPU, kv_buf_size=4096, **kw)
    assert [k for k, _ in r_none] == [k for k, _ in r_unset] and sorted(r_none) == sorted(r_unset)
    assert len(r_none) == st["combine_in_records"] and st_none["bytes_delivered"] == st_unset["bytes_delivered"]
    assert st_none["combine"] == st_unset["combine"] == "none" and st_none["combine_groups"] == 0
    assert combine_records(r_none, datagen.TEXT, "sum.int") == want


def test_cpu_task_wrong_value_length_falls_back_once(provider):
    maps = datagen.terasort(num_maps=3, reducers=1, rows_per_map=200)
    ids = _publish(provider, "job_7_0010", maps)
    conf = dict(CPU, **{"mapred.uda.merge.combine": "sum.int"})
    c = UdaConsumer(len(ids), "job_7_0010", "attempt_job_7_0010_r_000000_0", datagen.TEXT, conf=conf)
    for m in ids:
        c.fetch("h", "job_7_0010", m, 0)
    with pytest.raises(UdaFallback, match="value of 91 bytes"):
        c.wait(30)
    c.close()
    assert c.failure_calls == 1 and c.bytes == 0


def test_unknown_combine_value_fails_init():
    with pytest.raises(RuntimeError, match="none, sum.int or sum.long"):
        UdaConsumer(1, "job_7_0011", "attempt_job_7_0011_r_000000_0", datagen.TEXT,
                    conf=dict(CPU, **{"mapred.uda.merge.combine": "sum.float"}))
