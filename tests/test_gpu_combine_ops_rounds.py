"""The combiner's further ops in streamed key-range rounds and in reduce tasks (csrc/gpu/generic_merger.cc,
combine.hip, gpu_merge_staged.cc): sum.vint, whose delivered records change length, and min.int / max.long.
A round's cuts are sized from its input bytes, so a carried group whose record grows at a round's end is
the case the sizing has to cover. Byte for byte what the Python oracle delivers
(tests/combine_ops_cases.py); the over-budget hybrid combines its spills' re-encoded records again.

Follows tests/test_gpu_combine_rounds.py: a K-way cell holds about 512 elements and rounds are whole cells,
so a few thousand records under round_bytes = 8 KiB make tens of rounds."""
import functools
import random

import pytest

from tests.combine_ops_cases import OPS, encode_value, expected_task, oracle
from uda_amd import ops
from uda_amd.bridge import UdaProvider, run_reduce
from uda_amd.utils import datagen
from uda_amd.utils.ifile import J2CQueueReader, decode_stream, encode_stream, text, vint_encode
from uda_amd.utils.mof import encode_partitions

pytestmark = pytest.mark.gpu
SMALL, LARGE = 8 << 10, 64 << 10


def _value(rng, op):
    bits = 31 if OPS[op][1] is None else 8 * OPS[op][1] - 1
    return encode_value(op, rng.randint(-(1 << bits), (1 << bits) - 1) >> rng.choice((0, 8, 16, 24)))


def long_group_runs(op):
    """12 groups of 1 500 records dealt over 5 runs: no cell holds a whole group, every round ends in one."""
    rng = random.Random(3)
    parts = [[] for _ in range(5)]
    for g in range(12):
        for j in range(1500):
            parts[(g * 1500 + j) % 5].append((text(b"long-%04d" % g), _value(rng, op)))
    return [encode_stream(p) for p in parts]


def one_key_runs(op):
    rng = random.Random(4)
    return [encode_stream([(text(b"the-only-key"), _value(rng, op)) for _ in range(1500)]) for _ in range(6)]


def growing_carry_runs():
    """Groups of 700 records of VInt 127 (one byte) over 4 runs, so that most rounds end inside a group: the
    carried group's record is 3 bytes longer than its head when it is delivered (88 900 takes 4 bytes).
    Between them single records with 1-byte values, which stay as they are."""
    parts = [[] for _ in range(4)]
    for g in range(16):
        for j in range(700):
            parts[j % 4].append((text(b"grow-%04d" % g), vint_encode(127)))
        parts[g % 4].append((text(b"grow-%04d-single" % g), vint_encode(g)))
    return [encode_stream(p) for p in parts]


def wordcount_runs(value):
    return [s[0] for s in datagen.streams(datagen.wordcount(9, 1, 4000, value=value))]


CASES = {}
for _op in ("sum.vint", "min.int"):
    CASES[f"wordcount-{_op}"] = (datagen.TEXT, _op, wordcount_runs("vint" if _op == "sum.vint" else "int"))
    CASES[f"long-groups-{_op}"] = (datagen.TEXT, _op, long_group_runs(_op))
    CASES[f"one-key-{_op}"] = (datagen.TEXT, _op, one_key_runs(_op))
CASES["growing-carry-sum.vint"] = (datagen.TEXT, "sum.vint", growing_carry_runs())
CASES["growing-carry-sum.vlong"] = (datagen.TEXT, "sum.vlong", growing_carry_runs())


@functools.lru_cache(maxsize=None)
def want_of(name):
    key_class, op, runs = CASES[name]
    return oracle(runs, key_class, op)


def streamed(name, round_bytes, kv_buf):
    """One streamed merge of a case, with every check that holds for all of them."""
    key_class, op, runs = CASES[name]
    body, cuts, st = ops.merge_runs_streamed(runs, key_class, kv_buf=kv_buf, round_bytes=round_bytes, combine=op)
    rounds = st["rounds"]
    assert st["records"] == sum(r for r, _ in rounds)
    assert st["records_in"] == sum(len(decode_stream(r, require_eof=False)) for r in runs)
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
    key_class, op, runs = CASES[name]
    if name.startswith("wordcount"):  # the references agree with each other (the oracle serves every other case)
        assert ops.merge_runs(runs, key_class, "cpu", kv_buf=4096, combine=op)[0] == want_of(name)
    nbytes = sum(len(r) for r in runs)
    for round_bytes in (SMALL, LARGE):
        for kv_buf in (4096, 256):
            body, st = streamed(name, round_bytes, kv_buf)
            assert body == want_of(name)
            if nbytes > 2 * round_bytes:
                assert was_streamed(st), (name, round_bytes, len(st["rounds"]))
    assert nbytes > 2 * SMALL  # every case is streamed at the small round size


def test_a_carried_group_grows_at_a_rounds_end(require_gpu):
    body, st = streamed("growing-carry-sum.vint", SMALL, 256)
    assert body == want_of("growing-carry-sum.vint")
    assert len(st["rounds"]) >= 4 and st["held_records"] > 0 and st["records"] == 32
    recs = decode_stream(body, require_eof=False)
    assert recs[0] == (text(b"grow-0000"), vint_encode(88900)) and len(recs[0][1]) == 4


def test_one_key_is_carried_to_the_final_round(require_gpu):
    for name in ("one-key-sum.vint", "one-key-min.int"):
        body, st = streamed(name, SMALL, 4096)
        assert body == want_of(name)
        assert len(st["rounds"]) == 1 and st["rounds"][0][0] == 1  # only the final call
        assert st["held_records"] > 0 and st["records"] == 1 and st["records_in"] == 9000


def test_groups_longer_than_a_round(require_gpu):
    for name in ("long-groups-sum.vint", "long-groups-min.int"):
        body, st = streamed(name, SMALL, 4096)
        assert body == want_of(name)
        assert len(st["rounds"]) >= 4 and st["held_records"] > 0 and st["records"] == 12


# ---------------------------------------------------------------------------------------- reduce tasks
BUDGET = 340_000


def conf_of(op, **more):
    return dict({"mapred.uda.merge.backend": "gpu", "mapred.uda.merge.combine": op}, **more)


@pytest.fixture(scope="module")
def vint_maps():
    return datagen.wordcount(num_maps=9, reducers=1, words_per_map=6000, seed=43, value="vint")


@pytest.fixture(scope="module")
def big_vint_maps():  # 12 maps of about 35 KB each in VInt counts: over BUDGET
    return datagen.wordcount(num_maps=12, reducers=1, words_per_map=14000, seed=37, value="vint")


@pytest.fixture(scope="module")
def long_maps():
    """The wordcount's keys with 8-byte values of either sign, for max.long."""
    rng = random.Random(47)
    maps = datagen.wordcount(num_maps=9, reducers=1, words_per_map=6000, seed=43)
    return [[[(k, rng.randint(-(1 << 63), (1 << 63) - 1).to_bytes(8, "big", signed=True)) for k, _ in p] for p in m]
            for m in maps]


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


def _task_ok(recs, st, c, maps, op, job, ids):
    want = expected_task(maps, 0, datagen.TEXT, op)
    assert recs == want
    assert st["combine"] == op and st["combine_groups"] == len(want) == st["records"]
    assert st["combine_in_records"] == sum(len(m[0]) for m in maps)
    assert st["bytes_delivered"] == len(encode_stream(want)) == c.bytes
    # the CPU backend's task over the same MOFs delivers the same records
    cpu, st_cpu, _ = run_reduce("h", job, ids, 0, datagen.TEXT, kv_buf_size=8192,
                                conf={"mapred.uda.merge.backend": "cpu", "mapred.uda.merge.combine": op})
    assert cpu == recs and st_cpu["bytes_delivered"] == st["bytes_delivered"]


@pytest.mark.parametrize("op", ["sum.vint", "max.long"])
def test_task_device_mofs_in_key_range_rounds(require_gpu, provider, vint_maps, long_maps, op):
    maps = vint_maps if op == "sum.vint" else long_maps
    job = "job_11_01%02d" % len(op)
    ids = _publish(provider, job, maps, "device")
    conf = conf_of(op, **{"mapred.uda.gpu.fetch": "device", "mapred.uda.gpu.round.bytes": 64 << 10})
    recs, st, c = run_reduce("h", job, ids, 0, datagen.TEXT, conf=conf, kv_buf_size=8192)
    assert st["merge_path"] == "device-generic" and st["rpq_rounds"] > 1, st
    _task_ok(recs, st, c, maps, op, job, ids)


def test_task_host_mofs_within_budget(require_gpu, provider, vint_maps):
    ids = _publish(provider, "job_11_0200", vint_maps, "host")
    conf = conf_of("sum.vint", **{"mapred.uda.gpu.merge.round.bytes": 16 << 10})
    recs, st, c = run_reduce("h", "job_11_0200", ids, 0, datagen.TEXT, conf=conf, max_buf_kb=16, min_buf_kb=16,
                             kv_buf_size=8192)
    assert st["merge_path"] in ("staged", "staged-progressive") and st["merge_rounds"] >= 4, st
    _task_ok(recs, st, c, vint_maps, "sum.vint", "job_11_0200", ids)


@pytest.mark.parametrize("name", ["direct", "lpq-host"])
def test_task_over_budget_combines_re_encoded_spills(require_gpu, provider, big_vint_maps, name):
    job = "job_11_03%02d" % len(name)
    ids = _publish(provider, job, big_vint_maps, "host")
    conf = conf_of("sum.vint", **{"mapred.uda.merge.combine.over.budget": "combine", "mapred.uda.gpu.merge.bytes": BUDGET,
                                  "mapred.uda.gpu.spill": "host"})
    conf.update({"mapred.uda.gpu.hybrid.progressive": 0} if name == "direct" else {"mapred.uda.gpu.hybrid.direct": 0})
    recs, st, c = run_reduce("h", job, ids, 0, datagen.TEXT, conf=conf, kv_buf_size=8192)
    assert st["bytes_fetched"] > BUDGET and st["rpq_rounds"] > 1, st
    if name == "direct":
        assert st["hybrid_direct"] == 1 and st["lpqs"] == 0, st
    else:
        assert st["lpqs"] >= 2 and st["hybrid_direct"] == 0, st
    _task_ok(recs, st, c, big_vint_maps, "sum.vint", job, ids)
