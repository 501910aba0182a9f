"""CPU: the oracle of the device validators and of the TeraGen kernel (validate_cases.py) against what the host
already has: `record_hash` (uda/hash.h) and the `StreamValidator` (csrc/engine/validate.cc). The GPU tests
compare the kernels with the same oracle on the same cases (test_gpu_validate.py)."""
import numpy as np
import pytest

from tests import fixed10_cases as fc
from tests import validate_cases as vc
from uda_amd.utils import datagen


@pytest.mark.parametrize("n", list(range(25)) + [104])
def test_record_hash_is_the_native_one(native, n):
    data = bytes(np.random.RandomState(n).randint(0, 256, size=n, dtype=np.uint8))
    assert vc.record_hash(data) == native.record_hash(data)
    if n:  # the padding is zeros, and the length is part of the seed
        assert vc.record_hash(data) != vc.record_hash(data + b"\x00")


def host_validate(native, stream):
    v = native.StreamValidator(datagen.TEXT)
    v.feed(stream + fc.EOF)
    assert v.framing_errors == 0 and v.eof and v.records == len(stream) // vc.L
    return v.order_errors, v.checksum


@pytest.mark.parametrize("name", sorted(vc.order_cases()))
def test_order_cases_oracle_is_the_host_validator(native, name):
    stream, closed_form = vc.order_cases()[name]
    errors, ck, last = vc.validate([stream])
    assert errors == closed_form
    assert (errors, ck) == host_validate(native, stream)
    assert ck == vc.stream_checksum(stream)
    assert last == stream[-vc.L:][vc.KEY]


def test_order_cases_cover_the_edges():
    names = set(vc.order_cases())
    for n in vc.ORDER_N:
        want = {p for p in (0, 62, 63, 64, 254, 255, 256, n - 2) if 0 <= p <= n - 2}
        assert {f"swap_n{n}_p{p}" for p in want} <= names
    assert {"swap_n1000_p998", "swap_n257_p255", "swap_n65_p63", "swap_n2_p0"} <= names
    # the byte cases differ where they say, and nowhere else in the key
    for name, byte in (("byte9_only", 9), ("byte8_only", 8), ("byte0_only", 0)):
        r = fc.records(vc.order_cases()[name][0])
        p = 100 if byte == 0 else 63
        a, b = r[p][vc.KEY], r[p + 1][vc.KEY]
        assert a > b and [i for i in range(10) if a[i] != b[i]] == [byte]
    assert vc.order_cases()["descending"][1] == 999 and vc.order_cases()["all_equal"][1] == 0


def test_chunking_does_not_change_the_oracle(native):
    s, n = vc.chunk_stream(), vc.CHUNK_N
    whole = vc.validate([s])
    assert whole[0] == len(vc.CHUNK_INVERSIONS) == 6
    assert whole[:2] == host_validate(native, s)
    for c in vc.CHUNK_CUTS:
        assert vc.validate(vc.cut(s, [c])) == whole
    many = vc.cut(s, vc.MANY_CUTS)
    assert vc.validate(many) == whole
    lens = [len(c) // vc.L for c in many]
    assert lens.count(0) >= 5 and lens[0] == 0 and lens[-1] == 0 and lens.count(1) == 3
    # inversions on a cut: the chunk's last key is above the next chunk's first
    on_cut = [c for c in vc.CHUNK_CUTS if s[(c - 1) * vc.L:c * vc.L][vc.KEY] > s[c * vc.L:(c + 1) * vc.L][vc.KEY]]
    assert on_cut == [1, 64, 256, n - 1]
    t = vc.tail_stream()
    a, b = fc.records(t)[63][vc.KEY], fc.records(t)[64][vc.KEY]
    assert a > b and a[:8] == b[:8]
    assert vc.validate(vc.cut(t, [64])) == vc.validate([t]) and vc.validate([t])[0] == 1


def test_checksum_cases():
    base = vc.stream_checksum(vc.checksum_base())
    flips = vc.bit_flips()
    assert len(flips) == vc.L == 104
    sums = {vc.stream_checksum(f) for f in flips}
    assert len(sums) == 104 and base not in sums
    assert vc.permuted() != vc.checksum_base() and vc.stream_checksum(vc.permuted()) == base
    x = vc.values_exchanged()
    assert sorted(x) == sorted(vc.checksum_base()) and vc.stream_checksum(x) != base
    assert vc.validate([vc.permuted()])[1] == base


def test_layout_cases():
    cases = vc.layout_cases()
    assert sum(1 for _, good in cases.values() if not good) == 2 * 3 * 4 + 1
    for name, (slices, good) in cases.items():
        assert vc.slices_ok(slices) == good, name
    slices, _ = cases["only_last_slice_bad"]
    assert len(slices) == 40 and vc.slices_ok(slices[:-1]) and not vc.slices_ok(slices[-1:])
    assert vc.LAYOUT_RECORDS == (0, vc.LAYOUT_N - 1, 300) and 256 < 300


def test_mismatch_cases():
    cases = vc.mismatch_cases()
    for n in vc.MISMATCH_N:
        assert vc.count_mismatch(*cases[f"n{n}_equal"]) == 0
        assert vc.count_mismatch(*cases[f"n{n}_all_differ"], start=3) == n + 3
        assert vc.count_mismatch(*cases[f"n{n}_edges"]) == len({i for i in (0, 255, 256, n - 1) if i < n})
        for bit in (0, 63):
            a, b = cases[f"n{n}_bit{bit}_at{n - 1}"]
            assert vc.count_mismatch(a, b) == 1 and a[n - 1] ^ b[n - 1] == 1 << bit
    assert all(0 <= x < 1 << 64 for a, b in cases.values() for x in a + b)


@pytest.mark.parametrize("unsorted", [False, True])
def test_teragen_runs(native, unsorted):
    runs = vc.TERAGEN_UNSORTED if unsorted else vc.TERAGEN_SORTED
    assert sorted(r[0] for r in runs) == [1, 2, 255, 256, 257, 1000]
    for n, lo, span, seed in runs:
        run = vc.teragen_run(n, lo, span, seed, unsorted)
        assert len(run) == vc.L * n + 2 and run.endswith(fc.EOF)
        a = np.frombuffer(run[:-2], np.uint8).reshape(n, vc.L)
        assert all(vc.layout_ok(bytes(rec)) for rec in a)
        assert ((a[:, 14:] >= ord("A")) & (a[:, 14:] <= ord("Z"))).all()
        hi = [int.from_bytes(bytes(rec[3:11]), "big") for rec in a]
        assert all(lo <= h <= lo + span - (0 if unsorted and span == vc.M64 else 1) for h in hi)
        errors, ck, _ = vc.validate([run[:-2]])
        v = native.StreamValidator(datagen.TEXT)
        v.feed(run)
        assert (v.order_errors, v.checksum, v.records, v.eof, v.framing_errors) == (errors, ck, n, True, 0)
        if not unsorted:
            assert span >= n
            assert all(x < y for x, y in zip(hi, hi[1:])), "sorted mode ascends strictly in the first 8 key bytes"
            assert errors == 0
            if span == n:  # stride 1, jitter 0
                assert hi == [lo + i for i in range(n)]
    if not unsorted:
        assert any(lo + span == 1 << 64 for _, lo, span, _ in runs)
        assert vc.teragen_run(257, vc.TOP - 257, 257, 3)[-2 - vc.L:][3:11] == b"\xff" * 8
    else:
        assert any(span == vc.M64 for _, _, span, _ in runs) and any(span < 10 for _, _, span, _ in runs)


def test_teragen_span_below_the_record_count_is_no_sorted_run():
    """Why sorted generation needs key_span >= nrec: the stride is 0 and only the random last two bytes differ."""
    run = vc.teragen_run(50, 1000, 49, 1)
    keys = [rec[vc.KEY] for rec in fc.records(run[:-2])]
    assert {k[:8] for k in keys} == {(1000).to_bytes(8, "big")}
    assert vc.validate([run[:-2]])[0] > 0


def test_teragen_contract_is_refused_on_the_host(native):
    native.teragen_require_spans([1, 1000, 0], [1, 1000, 0])
    native.teragen_require_spans([], [])
    with pytest.raises(ValueError, match="run 1 has 1000 records in a key span of 999"):
        native.teragen_require_spans([5, 1000], [5, 999])
    with pytest.raises(ValueError):
        native.teragen_require_spans([1], [0])
    with pytest.raises(ValueError):
        native.teragen_require_spans([1, 2], [1])


def test_cases_stay_small():
    longest = max(len(s) // vc.L for s in vc.all_streams())
    assert 1000 <= longest < vc.MAX_RECORDS == 1200
    assert all(n < 1200 for n, *_ in vc.TERAGEN_SORTED + vc.TERAGEN_UNSORTED)
    assert all(len(a) < 1200 for a, _ in vc.mismatch_cases().values())
