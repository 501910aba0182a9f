"""mapred.uda.key.order=hadoop on the host (csrc/include/uda/compare.h): the sortable word and the comparator
against the pure-Python oracle of tests/key_order_cases.py, loopback reduce tasks of the CPU backend per
numeric key class, the group a memcmp merge splits, the combiner over negative keys, keys of the wrong
length, the conf parser, and the comparator under ASan + UBSan in a program of its own."""
import os
import shutil
import subprocess

import pytest

from tests import key_order_cases as ko
from tests.generic_cases import record, write_vlong
from uda_amd import ops
from uda_amd.bridge import UdaConsumer, UdaFallback, UdaProvider, run_reduce
from uda_amd.utils.mof import encode_partitions

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPU = {"mapred.uda.merge.backend": "cpu"}
CPU_HADOOP = dict(CPU, **ko.HADOOP)


def sign(x):
    return (x > 0) - (x < 0)


# ------------------------------------------------------------------------------------------------ comparator
def test_kind_lookup_takes_the_order(native):
    for cls in ko.CLASSES:
        assert native.key_kind_ordered(cls, "hadoop") == ko.KIND[cls]
    # the default order: nothing changes
    for cls in (ko.BYTE, ko.SHORT, ko.INT, ko.LONG):
        assert native.key_kind_ordered(cls, "reference") == native.key_kind(cls) == 1
    for cls in (ko.VINT, ko.VLONG, ko.FLOAT, ko.DOUBLE):
        assert native.key_kind_ordered(cls, "reference") == native.key_kind(cls) == -1
    # byte-compared classes keep their kinds under either order
    for cls, kind in ((ko.P + "Text", 0), (ko.P + "BooleanWritable", 1), (ko.P + "BytesWritable", 2),
                      ("org.apache.hadoop.hbase.io.ImmutableBytesWritable", 2), ("com.example.Custom", -1)):
        assert native.key_kind_ordered(cls, "hadoop") == native.key_kind_ordered(cls, "reference") == kind
    with pytest.raises(ValueError, match="reference or hadoop"):
        native.key_kind_ordered(ko.INT, "bogus")


@pytest.mark.parametrize("cls", ko.CLASSES, ids=[c.rsplit(".", 1)[1] for c in ko.CLASSES])
def test_sortable_and_compare_match_the_oracle(native, cls):
    kind = ko.KIND[cls]
    edges = ko.edge_keys(cls)
    words = {k: ko.sortable(cls, k) for k in edges + ko.random_keys(cls)}
    for k, w in words.items():
        assert native.key_sortable(kind, k) == w, k.hex()
    for a in edges:  # pairwise over the edge values
        for b in edges:
            assert sign(native.key_compare(kind, a, b)) == sign(words[a] - words[b]), (a.hex(), b.hex())
    rnd = ko.random_keys(cls)
    for a, b in zip(rnd, rnd[1:] + edges[:1]):
        assert sign(native.key_compare(kind, a, b)) == sign(words[a] - words[b]), (a.hex(), b.hex())
        assert sign(native.key_compare(kind, b, a)) == sign(words[b] - words[a])


def test_the_order_is_javas(native):
    """Spot checks written out, so a mistake shared by the oracle and the table it copies would show."""
    def lt(cls, a, b):
        return native.key_compare(ko.KIND[cls], a, b) < 0 and native.key_compare(ko.KIND[cls], b, a) > 0

    def eq(cls, a, b):
        return native.key_compare(ko.KIND[cls], a, b) == 0 == native.key_compare(ko.KIND[cls], b, a)

    assert lt(ko.INT, ko.int_key(ko.INT, -1), ko.int_key(ko.INT, 3))
    assert native.key_compare(1, ko.int_key(ko.INT, -1), ko.int_key(ko.INT, 3)) > 0  # the reference kind: memcmp
    assert lt(ko.BYTE, b"\x80", b"\x7f") and lt(ko.SHORT, b"\xff\xff", b"\x00\x00")
    assert lt(ko.LONG, ko.int_key(ko.LONG, -(1 << 63)), ko.int_key(ko.LONG, (1 << 63) - 1))
    assert lt(ko.VLONG, write_vlong(-1000), write_vlong(-113)) and lt(ko.VLONG, write_vlong(127), write_vlong(128))
    assert eq(ko.VLONG, write_vlong(300), ko.noncanonical_vlong(300, 4))
    assert eq(ko.VINT, write_vlong(-1), ko.noncanonical_vlong(-1, 2))
    assert lt(ko.FLOAT, ko.f32(0x80000000), ko.f32(0))  # -0.0 < +0.0
    assert lt(ko.FLOAT, ko.f32(0x7f800000), ko.f32(0xffc00001))  # +inf < a negative-signed NaN
    assert eq(ko.FLOAT, ko.f32(0x7fc00000), ko.f32(0xffffffff))
    assert lt(ko.DOUBLE, ko.f64(0xfff0000000000000), ko.f64(0xffefffffffffffff))  # -inf < -max
    assert eq(ko.DOUBLE, ko.f64(0x7ff0000000000001), ko.f64(0xfff8000000000001))
    assert lt(ko.DOUBLE, ko.f64(0x8000000000000001), ko.f64(0x8000000000000000))  # -denormal < -0.0


def test_sortable_refuses_a_wrong_length(native):
    bad = [(ko.INT, b"\0\0\0"), (ko.INT, b"\0" * 5), (ko.BYTE, b""), (ko.LONG, b"\0" * 4), (ko.FLOAT, b"\0" * 8),
           (ko.DOUBLE, b"\0" * 4), (ko.VINT, b""), (ko.VINT, b"\x8f\x01\x02"), (ko.VLONG, b"\x05\x00"),
           (ko.VINT, write_vlong(1 << 31)), (ko.VINT, write_vlong(-(1 << 31) - 1))]
    for cls, key in bad:
        with pytest.raises(ko.BadKey):
            ko.sortable(cls, key)
        with pytest.raises(ValueError, match=cls.rsplit(".", 1)[1] + " key of %d bytes" % len(key)):
            native.key_sortable(ko.KIND[cls], key)
    assert native.key_sortable(ko.KIND[ko.VLONG], write_vlong(1 << 31)) == ko.sortable(ko.VLONG, write_vlong(1 << 31))


def test_comparator_under_sanitizers(tmp_path):
    """tests/native/key_order_selftest.cc (key_sortable, key_compare, key_normalize over the edge values, and the
    CPU merge through csrc/engine/ifile.cc) under ASan + UBSan; never loaded into Python."""
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "key_order_selftest")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I" + os.path.join(ROOT, "csrc", "include"),
                    os.path.join(ROOT, "tests", "native", "key_order_selftest.cc"),
                    os.path.join(ROOT, "csrc", "engine", "combine.cc"),
                    os.path.join(ROOT, "csrc", "engine", "ifile.cc"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert " 0 failures" in r.stdout


# ------------------------------------------------------------------------------------------------ CPU merge
@pytest.mark.parametrize("cls", ko.CLASSES, ids=[c.rsplit(".", 1)[1] for c in ko.CLASSES])
def test_cpu_merge_matches_the_oracle(cls):
    runs = ko.make_runs(cls, (150, 0, 200, 1, 90), seed=1)
    body, cuts = ops.merge_runs([ko.stream(r) for r in runs], cls, "cpu", kv_buf=512, key_order="hadoop")
    assert body == ko.oracle_merge(runs, cls)
    assert cuts[0] == 0 and cuts[-1] == len(body)


# ------------------------------------------------------------------------------------------------ reduce tasks
@pytest.fixture
def provider():
    p = UdaProvider()
    yield p
    p.close()


def _publish(provider, job, runs):
    """One map output per run, a single partition each."""
    ids = []
    for i, run in enumerate(runs):
        mid = f"attempt_{job}_m_{i:06d}_0"
        data, index = encode_partitions([ko.stream(run)])
        provider.add_mof_memory(job, mid, data, index)
        ids.append(mid)
    return ids


def _bytes(recs):
    return b"".join(record(k, v) for k, v in recs)


@pytest.mark.parametrize("cls", ko.CLASSES, ids=[c.rsplit(".", 1)[1] for c in ko.CLASSES])
def test_cpu_task_delivers_hadoops_order(provider, cls):
    """Fails without the feature: IntWritable comes out in memcmp order, DoubleWritable fails INIT. (A task
    numbers its map outputs as they arrive, so the runs share no key here; ties between runs are checked on
    the merge above, whose run order is given.)"""
    runs = ko.make_runs(cls, (200, 210, 190), seed=2, disjoint=True)
    assert all(runs)
    assert any(ko.sortable(cls, k) < ko.SIGN for r in runs for k, _ in r)  # negative keys present
    job = "job_21_%04d" % ko.KIND[cls]
    ids = _publish(provider, job, runs)
    recs, st, c = run_reduce("h", job, ids, 0, cls, conf=CPU_HADOOP, kv_buf_size=4096)
    assert _bytes(recs) == ko.oracle_merge(runs, cls)
    assert st["key_order"] == "hadoop" and st["records"] == sum(len(r) for r in runs)
    assert c.failure_calls == 0


def test_cpu_task_hybrid_merge_delivers_hadoops_order(provider, tmp_path):
    runs = ko.make_runs(ko.INT, (40,) * 23, seed=3)
    ids = _publish(provider, "job_21_0100", runs)
    recs, st, c = run_reduce("h", "job_21_0100", ids, 0, ko.INT, conf=CPU_HADOOP, kv_buf_size=4096, approach=2,
                             lpq_size=5, local_dirs=(str(tmp_path),))
    # LPQ files merge map outputs in the order they arrive: equal keys tie by that, so compare as sorted groups
    want = ko.merged_records(runs, ko.INT)
    assert [ko.sortable(ko.INT, k) for k, _ in recs] == [ko.sortable(ko.INT, k) for k, _ in want]
    assert sorted(recs) == sorted(want)


def test_the_validator_follows_the_order(provider):
    """The consumer's native stream validator checks the delivered order under the job's key order."""
    runs = ko.make_runs(ko.LONG, (120, 130), seed=6, disjoint=True)
    ids = _publish(provider, "job_21_0150", runs)
    _, st, c = run_reduce("h", "job_21_0150", ids, 0, ko.LONG, conf=CPU_HADOOP, validate=True)
    assert c.validator.records == 250 and c.validator.order_errors == 0 and c.validator.framing_errors == 0
    _, st, c = run_reduce("h", "job_21_0150", ids, 0, ko.LONG, conf=CPU, validate=True)  # runs unsorted to memcmp
    assert c.validator.records == 250 and c.validator.order_errors > 0


def test_the_group_of_key_3_is_not_split(provider):
    k = lambda v: ko.int_key(ko.INT, v)
    runs = [[(k(-1), b"a"), (k(3), b"b")], [(k(3), b"c")]]
    ids = _publish(provider, "job_21_0200", runs)
    recs, st, _ = run_reduce("h", "job_21_0200", ids, 0, ko.INT, conf=CPU_HADOOP)
    # (the two records of key 3 tie by the order in which their map outputs arrived)
    assert [key for key, _ in recs] == [k(-1), k(3), k(3)] and sorted(v for _, v in recs) == [b"a", b"b", b"c"]
    # the default order is the reference's memcmp: the group of key 3 is split around -1 or ends before it
    recs, st, _ = run_reduce("h", "job_21_0200", ids, 0, ko.INT, conf=CPU)
    assert [key for key, _ in recs] in ([k(3), k(-1), k(3)], [k(3), k(3), k(-1)]) and st["key_order"] == "reference"


def test_sum_int_over_negative_keys_yields_one_record_per_key(provider):
    keys = [ko.int_key(ko.INT, v) for v in (-70000, -300, -2, -1, 0, 1, 2, 255, 256, 70000)]
    runs = ko.make_runs(ko.INT, (120, 130, 110), seed=4, keys=keys)
    runs = [[(key, (7 * r + i).to_bytes(4, "big")) for i, (key, _) in enumerate(run)] for r, run in enumerate(runs)]
    ids = _publish(provider, "job_21_0300", runs)
    conf = dict(CPU_HADOOP, **{"mapred.uda.merge.combine": "sum.int"})
    recs, st, _ = run_reduce("h", "job_21_0300", ids, 0, ko.INT, conf=conf)
    assert recs == ko.fold_sum(ko.merged_records(runs, ko.INT), ko.INT, "sum.int")
    assert [k for k, _ in recs] == keys and st["combine_groups"] == len(keys)


@pytest.mark.parametrize("cls,bad,length", [(ko.INT, b"\x00\x00\x07", 3), (ko.VINT, b"\x8e\x01", 2)],
                         ids=["int-of-3-bytes", "vint-shorter-than-announced"])
def test_a_key_of_the_wrong_length_fails_the_task_once(provider, cls, bad, length):
    runs = ko.make_runs(cls, (30, 30, 30), seed=5)
    runs[1].insert(15, (bad, b"v"))
    job = "job_21_04%02d" % ko.KIND[cls]
    ids = _publish(provider, job, runs)
    c = UdaConsumer(len(ids), job, f"attempt_{job}_r_000000_0", cls, conf=CPU_HADOOP)
    for m in ids:
        c.fetch("h", job, m, 0)
    name = cls.rsplit(".", 1)[1]
    with pytest.raises(UdaFallback, match=rf"{name} key of {length} bytes .* in map output {ids[1]}"):
        c.wait(30)
    c.close()
    assert c.failure_calls == 1


def test_an_unknown_order_fails_init():
    with pytest.raises(RuntimeError, match=r'mapred.uda.key.order "bogus" \(reference or hadoop\)'):
        UdaConsumer(1, "job_21_0500", "attempt_job_21_0500_r_000000_0", ko.INT,
                    conf=dict(CPU, **{"mapred.uda.key.order": "bogus"}))
    with pytest.raises(RuntimeError, match="unsupported type"):  # the default order still has no DoubleWritable
        UdaConsumer(1, "job_21_0501", "attempt_job_21_0501_r_000000_0", ko.DOUBLE, conf=CPU)
    c = UdaConsumer(1, "job_21_0502", "attempt_job_21_0502_r_000000_0", ko.DOUBLE, conf=CPU_HADOOP)
    c.close()
