"""The combiner in streamed key-range rounds (csrc/gpu/generic_merger.cc, combine.hip): a device merge of
more than round_bytes under mapred.uda.merge.combine hands its output over in rounds that end on group
boundaries, carrying an open last group into the next round. Byte for byte what the CPU backend and the
Python oracle deliver (tests/combine_cases.py).

A cell of the K-way merge holds about 512 elements (generic_kway.hip: cap 1024, T = cap / 2) and the
rounds are whole cells, so a few thousand records under round_bytes = 8 KiB make tens of rounds. An
input of at most round_bytes takes the whole path (one hand-over, nothing held): every test asserts that
its input was streamed."""
import functools
import random

import pytest

import uda_amd
from tests.combine_cases import _val, boundary_lengths, expected_task, huge_key_runs, ops_cases, oracle
from uda_amd import ops
from uda_amd.bridge import UdaProvider, run_reduce
from uda_amd.utils import datagen
from uda_amd.utils.ifile import J2CQueueReader, decode_stream, encode_stream, text
from uda_amd.utils.mof import encode_partitions

pytestmark = pytest.mark.gpu
TILE = uda_amd.native().combine_tile()
CASES = {c[0]: c for c in ops_cases(TILE)}
CELL = 512  # elements per K-way cell; fewer than two cells cannot make two rounds
SMALL, LARGE = 8 << 10, 64 << 10


def long_group_runs():
    """12 groups of 1 500 records dealt over 5 runs: no cell holds a whole group, every round ends in one."""
    rng = random.Random(3)
    parts = [[] for _ in range(5)]
    for g in range(12):
        for j in range(1500):
            parts[(g * 1500 + j) % 5].append((text(b"long-%04d" % g), _val(rng, 4)))
    return [encode_stream(p) for p in parts]


CASES["long-groups"] = ("long-groups", datagen.TEXT, "sum.int", long_group_runs())


@functools.lru_cache(maxsize=None)
def want_of(name):
    _, key_class, op, runs = CASES[name]
    return oracle(runs, key_class, op)


@functools.lru_cache(maxsize=None)
def records_in(name):
    return sum(len(decode_stream(r, require_eof=False)) for r in CASES[name][3])


def streamed(name, round_bytes, kv_buf, combine=None):
    """One streamed merge of a case, with every check that holds for all of them."""
    _, key_class, op, runs = CASES[name]
    body, cuts, st = ops.merge_runs_streamed(runs, key_class, kv_buf=kv_buf, round_bytes=round_bytes,
                                             combine=op if combine is None else combine)
    rounds = st["rounds"]
    assert st["records"] == sum(r for r, _ in rounds)
    assert st["records_in"] == records_in(name)
    # the rounds' cuts are the call's cuts, in order, each round starting where the one before ended
    joined = [0]
    for _, rc in rounds:
        assert rc[0] == joined[-1] and rc == sorted(rc)
        joined += rc[1:]
    assert joined == cuts and cuts[-1] == len(body)
    assert all(b - a <= kv_buf - 2 for a, b in zip(cuts[:-1], cuts[1:]))  # (2: the EOF marker's room)
    r = J2CQueueReader(max_len=kv_buf)
    for b in ops.buffers(body, cuts):
        r.feed(b)
    assert r.eof and encode_stream(r.records, eof=False) == body and len(r.records) == st["records"]
    return body, st


def was_streamed(st):
    return len(st["rounds"]) > 1 or st["held_records"] > 0


@pytest.mark.parametrize("name", list(CASES))
def test_streamed_rounds_match_the_oracle(require_gpu, name):
    _, key_class, op, runs = CASES[name]
    if name == "wordcount":  # the references agree with each other (once: the oracle serves every other case)
        assert ops.merge_runs(runs, key_class, "cpu", kv_buf=4096, combine=op)[0] == want_of(name)
    nbytes = sum(len(r) for r in runs)
    for round_bytes in (SMALL, LARGE):
        for kv_buf in (4096, 256):
            body, st = streamed(name, round_bytes, kv_buf)
            assert body == want_of(name)
            if nbytes > 2 * round_bytes and records_in(name) > 2 * CELL and len(runs) >= 2:
                assert was_streamed(st), (name, round_bytes, len(st["rounds"]))


def test_one_key_is_carried_to_the_final_round(require_gpu):
    body, st = streamed("one-key", SMALL, 4096)
    assert body == want_of("one-key")
    assert len(st["rounds"]) == 1 and st["rounds"][0][0] == 1  # only the final call
    assert st["held_records"] > 0 and st["records"] == 1 and st["records_in"] == 30000


def test_groups_longer_than_a_round(require_gpu):
    body, st = streamed("long-groups", SMALL, 4096)
    assert body == want_of("long-groups")
    assert len(st["rounds"]) >= 4 and st["held_records"] > 0 and st["records"] == 12
    # a group spans several rounds: fewer hand-overs than a plain streamed merge of the same input makes
    _, plain = streamed("long-groups", SMALL, 4096, combine="none")
    assert len(st["rounds"]) <= 12 < len(plain["rounds"])


def test_all_distinct_is_the_plain_streamed_merge(require_gpu):
    body, st = streamed("all-distinct", SMALL, 4096)
    plain, pst = streamed("all-distinct", SMALL, 4096, combine="none")
    assert len(st["rounds"]) >= 4 and len(pst["rounds"]) >= 4
    assert body == plain == want_of("all-distinct") and st["records"] == pst["records"] == 6000


def test_group_lengths_around_every_boundary(require_gpu):
    body, st = streamed("group-lengths", SMALL, 4096)
    assert body == want_of("group-lengths")
    assert len(st["rounds"]) >= 4 and st["records"] == len(boundary_lengths(TILE))


def test_huge_keys_stay_three_groups(require_gpu):
    runs = huge_key_runs()
    body, _, st = ops.merge_runs_streamed(runs, datagen.TEXT, kv_buf=1 << 20, round_bytes=SMALL, combine="sum.int")
    assert body == oracle(runs, datagen.TEXT, "sum.int")
    assert st["records"] == 3 and st["records_in"] == 6 and sum(r for r, _ in st["rounds"]) == 3


def test_wrong_value_length_in_the_last_round_delivers_nothing(require_gpu):
    good = [encode_stream([(text(b"k%d-%05d" % (r, i)), b"\0\0\0\1") for i in range(2500)]) for r in range(3)]
    bad = encode_stream([(text(b"k0-00007"), b"\0\0\0\2"), (text(b"zzz-bad-key"), b"12345")])
    n = uda_amd.native()
    with pytest.raises(RuntimeError, match=r"value of 5 bytes.*zzz-bad-key"):
        ops.merge_runs_streamed(good + [bad], datagen.TEXT, kv_buf=4096, round_bytes=SMALL, combine="sum.int")
    assert n.gpu_merge_streamed_last_rounds() == 0  # no on_round call was made
    # the same runs without the bad record stream, and the counter does count
    ok = good + [encode_stream([(text(b"k0-00007"), b"\0\0\0\2")])]
    body, _, st = ops.merge_runs_streamed(ok, datagen.TEXT, kv_buf=4096, round_bytes=SMALL, combine="sum.int")
    assert body == oracle(ok, datagen.TEXT, "sum.int") and st["records"] == 7500
    assert n.gpu_merge_streamed_last_rounds() == len(st["rounds"]) >= 4


# ---------------------------------------------------------------------------------------- reduce tasks
SUM = {"mapred.uda.merge.backend": "gpu", "mapred.uda.merge.combine": "sum.int",
       "mapred.uda.gpu.merge.round.bytes": 16 << 10}


@pytest.fixture(scope="module")
def maps():
    return datagen.wordcount(num_maps=9, reducers=1, words_per_map=6000, seed=43)


@pytest.fixture(scope="module")
def want(maps):
    return expected_task(maps, 0, datagen.TEXT, "sum.int")


@pytest.fixture
def provider():
    p = UdaProvider()
    yield p
    p.close()


def _publish(provider, job, maps, where):
    ids = []
    for i, parts in enumerate(datagen.streams(maps)):
        mid = f"attempt_{job}_m_{i:06d}_0"
        data, index = encode_partitions(parts, None, block_size=64 << 10)
        if where == "device":
            provider.add_mof_device(job, mid, data, index, device=0)
        else:
            provider.add_mof_memory(job, mid, data, index)
        ids.append(mid)
    return ids


@pytest.mark.parametrize("path", ["device-generic", "staged", "staged-progressive"])
def test_task_combines_in_inner_rounds(require_gpu, provider, maps, want, path):
    job = "job_9_01%02d" % len(path)
    ids = _publish(provider, job, maps, "device" if path == "device-generic" else "host")
    conf = dict(SUM)
    kw = {}
    if path == "device-generic":
        conf["mapred.uda.gpu.fetch"] = "device"
    else:
        conf["mapred.uda.gpu.progressive.phases"] = 3 if path == "staged-progressive" else 0
        kw = dict(max_buf_kb=16, min_buf_kb=16)
    recs, st, c = run_reduce("h", job, ids, 0, datagen.TEXT, conf=conf, kv_buf_size=8192, **kw)
    # (without SDMA staging the progressive phases are not taken: the task is then the staged one)
    assert st["merge_path"] == path or (path == "staged-progressive" and st["merge_path"] == "staged"), st
    assert st["merge_rounds"] >= 4, st  # the inner rounds were driven, not one hand-over per merge
    assert recs == want
    assert st["combine"] == "sum.int" and st["combine_groups"] == len(want) == st["records"]
    assert st["combine_in_records"] == sum(len(m[0]) for m in maps)
    assert st["bytes_delivered"] == len(encode_stream(want)) == c.bytes
    if path == "device-generic":  # the CPU backend over the same MOFs delivers the same records
        cpu, st_cpu, _ = run_reduce("h", job, ids, 0, datagen.TEXT, kv_buf_size=8192,
                                    conf={"mapred.uda.merge.backend": "cpu", "mapred.uda.merge.combine": "sum.int"})
        assert cpu == recs and st_cpu["bytes_delivered"] == st["bytes_delivered"]
