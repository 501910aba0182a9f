"""GPU: the device validators (`validate_fixed_kernel`, `slice_checksum_kernel`, `check_fixed_kernel`,
`count_mismatch_kernel`, csrc/gpu/merge.hip) and the TeraGen kernel (csrc/gpu/datagen.hip) on streams that are
wrong in one known way, and a shuffle step whose merged output is made wrong on purpose.

Oracle: the pure-Python validators and generator of validate_cases.py (checked against the host's `record_hash`
and `StreamValidator` in test_validate_cases_cpu.py). Everything is an integer or bytes and compared for equality;
there are no tolerances. The cases sit on the kernels' edges: a 64-lane wave, a 256-thread block, record n - 1."""
import pytest

from tests import fixed10_cases as fc
from tests import validate_cases as vc
from uda_amd.parallel.dist import DistContext

pytestmark = pytest.mark.gpu


def device_validate(native, chunks):
    d = native.gpu_validate_fixed([bytes(c) for c in chunks])
    assert d["group_ck"] == d["checksum"]  # both sums take every wave's hashes
    return d["order_errors"], d["checksum"], d["last_key"]


# ------------------------------------------------------------------ validate_fixed_kernel: order


@pytest.mark.parametrize("name", sorted(vc.order_cases()))
def test_order_errors(require_gpu, native, name):
    stream, closed_form = vc.order_cases()[name]
    want = vc.validate([stream])
    assert want[0] == closed_form
    assert device_validate(native, [stream]) == want


def test_no_records(require_gpu, native):
    assert device_validate(native, []) == (0, 0, b"") == vc.validate([])
    assert device_validate(native, [b"", b""]) == (0, 0, b"")


# ------------------------------------------------------------------ validate_fixed_kernel: chained launches


@pytest.mark.parametrize("at", vc.CHUNK_CUTS)
def test_two_chunks(require_gpu, native, at):
    """An inversion on the cut (1, 64, 256, n - 1) is the second launch's to count, once; one beside it is not."""
    s = vc.chunk_stream()
    want = vc.validate([s])
    assert want[0] == len(vc.CHUNK_INVERSIONS)
    assert device_validate(native, vc.cut(s, [at])) == want


def test_many_chunks_and_empty_ones(require_gpu, native):
    """One-record chunks with a predecessor take the has_prev and the last_key branch in one thread."""
    s = vc.chunk_stream()
    assert device_validate(native, vc.cut(s, vc.MANY_CUTS)) == vc.validate([s])
    every = list(range(1, 70))  # 69 one-record chunks, then the rest
    assert device_validate(native, vc.cut(s, every)) == vc.validate([s])


def test_boundary_inversion_in_the_last_two_key_bytes(require_gpu, native):
    t = vc.tail_stream()
    want = vc.validate([t])
    assert want[0] == 1
    assert device_validate(native, [t]) == want
    assert device_validate(native, vc.cut(t, [64])) == want       # across launches: prev_key->lo >> 48
    assert device_validate(native, vc.cut(t, [63, 64, 65])) == want
    # the same records in order: nothing to report on the cut
    good = vc.swap(t, 63)
    assert device_validate(native, vc.cut(good, [64])) == vc.validate([good]) and vc.validate([good])[0] == 0


# ------------------------------------------------------------------ checksums


def test_checksum_sees_every_byte(require_gpu, native):
    flips = vc.bit_flips()
    base = vc.stream_checksum(vc.checksum_base())
    want = [vc.stream_checksum(f) for f in flips]
    assert base not in want and len(set(want)) == len(flips) == 104
    assert native.gpu_slice_checksums(list(flips) + [vc.checksum_base()]) == want + [base]
    for f in flips:  # a flipped key byte may also invert a pair: the oracle says
        assert device_validate(native, [f]) == vc.validate([f])


def test_checksum_keeps_permutations_only(require_gpu, native):
    base = vc.stream_checksum(vc.checksum_base())
    p, x = vc.permuted(), vc.values_exchanged()
    assert vc.stream_checksum(p) == base != vc.stream_checksum(x)
    assert native.gpu_slice_checksums([vc.checksum_base(), p, x]) == [base, base, vc.stream_checksum(x)]
    assert device_validate(native, [p]) == vc.validate([p])
    assert device_validate(native, [x]) == vc.validate([x])


@pytest.mark.parametrize("max_nrec", [None, 1, 1 << 20])
def test_slice_checksums(require_gpu, native, max_nrec):
    """Slices of 0 to 1000 records in one launch; max_nrec 1 is one block per slice (grid-stride loop), 2^20 the
    widest grid the launcher makes (most blocks find nothing to do)."""
    slices = list(vc.slice_mix())
    assert [len(s) // vc.L for s in slices] == list(vc.SLICE_SIZES)
    want = [vc.stream_checksum(s) for s in slices]
    assert want[0] == 0
    assert native.gpu_slice_checksums(slices, max_nrec=max_nrec) == want


def test_slice_checksums_many_slices(require_gpu, native):
    singles = list(vc.slice_singles())
    assert len(singles) == 300
    assert native.gpu_slice_checksums(singles) == [vc.record_hash(r) for r in singles]
    assert native.gpu_slice_checksums([]) == []


# ------------------------------------------------------------------ check_fixed_kernel


@pytest.mark.parametrize("max_nrec", [None, 1])
def test_layout_check(require_gpu, native, max_nrec):
    for name, (slices, good) in vc.layout_cases().items():
        assert vc.slices_ok(slices) == good
        assert native.gpu_check_fixed(list(slices), max_nrec=max_nrec) == good, name


# ------------------------------------------------------------------ count_mismatch_kernel


def test_count_mismatch(require_gpu, native):
    for name, (a, b) in vc.mismatch_cases().items():
        assert native.gpu_count_mismatch(a, b) == vc.count_mismatch(a, b), name
        assert native.gpu_count_mismatch(a, b, start=1 << 40) == vc.count_mismatch(a, b, 1 << 40), name
    assert native.gpu_count_mismatch([], [], start=7) == 7


# ------------------------------------------------------------------ teragen_kernel


@pytest.mark.parametrize("unsorted", [False, True])
def test_teragen_is_the_python_generator(require_gpu, native, unsorted):
    plan = vc.TERAGEN_UNSORTED if unsorted else vc.TERAGEN_SORTED
    nrec, lo, span, seeds = (list(c) for c in zip(*plan))
    bufs, cks = native.gpu_teragen(nrec, lo, span, seeds, unsorted=unsorted)
    assert len(bufs) == len(cks) == len(plan)
    for (n, klo, kspan, seed), buf, ck in zip(plan, bufs, cks):
        want = vc.teragen_run(n, klo, kspan, seed, unsorted)
        assert len(buf) == vc.L * n + 2 + 16
        assert buf[:-16] == want, (n, klo, kspan)
        assert buf[-16:] == b"\xa5" * 16, "written past the EOF marker"
        assert ck == vc.stream_checksum(want[:-2])
    # the generated runs through the validators: their verdicts agree with the generator's checksum
    records = [bytes(b[:-18]) for b in bufs]
    assert native.gpu_check_fixed(records)
    assert native.gpu_slice_checksums(records) == list(cks)
    for rec, ck in zip(records, cks):
        errors, got, last = device_validate(native, [rec])
        assert (errors, got, last) == vc.validate([rec]) and got == ck
        if not unsorted:
            assert errors == 0


def test_teragen_refuses_a_span_below_the_record_count(require_gpu, native):
    with pytest.raises(ValueError, match="key_span >= nrec"):
        native.gpu_teragen([10, 50], [0, 1000], [10, 49], [1, 1])
    # unsorted generation has no such contract: the keys are drawn, not strided
    bufs, cks = native.gpu_teragen([50], [1000], [49], [1], unsorted=True)
    assert bufs[0][:-16] == vc.teragen_run(50, 1000, 49, 1, True)


# ------------------------------------------------------------------ a wrong merge reaches the caller


@pytest.fixture(scope="module")
def shuffle(require_gpu):
    from uda_amd.models.terasort import TeraSortConfig, TeraSortShuffle
    cfg = TeraSortConfig(rows_per_gpu=60_000, maps_per_rank=4, rounds=3, reducers=2, validate=True,
                         sample_every=64, kv_buf_bytes=64 << 10, d2h_piece_bytes=256 << 10)
    j = TeraSortShuffle(DistContext(), cfg, device=0)
    j.setup()
    return j


def clean_step(j):
    st = j.step()
    j.check(st)
    assert st["order_errors"] == 0 and st["merge_errors"] == 0 and st["checksum"] == j.expected_checksum
    assert st["records"] == 60_000


def test_clean_step(shuffle):
    clean_step(shuffle)


def test_swapped_records_are_an_order_error(shuffle, monkeypatch):
    """MERGE_SWAP at round 2: two neighbours of a sorted group exchanged invert exactly one pair; the records are
    the same, so every checksum still holds."""
    monkeypatch.setenv("UDA_FAULT_MERGE_SWAP", "2")
    st = shuffle.step()
    assert st["order_errors"] == 1
    assert st["checksum"] == shuffle.expected_checksum
    assert st["merge_errors"] == 0
    with pytest.raises(AssertionError, match="out-of-order"):
        shuffle.check(st)
    monkeypatch.delenv("UDA_FAULT_MERGE_SWAP")
    clean_step(shuffle)


def test_flipped_value_bit_is_a_checksum_error(shuffle, monkeypatch):
    """MERGE_FLIP at round 2: the order holds, one (round, reducer) output no longer sums to its inputs."""
    monkeypatch.setenv("UDA_FAULT_MERGE_FLIP", "2")
    st = shuffle.step()
    assert st["order_errors"] == 0
    assert st["checksum"] != shuffle.expected_checksum
    assert st["merge_errors"] == 1
    assert "round 1 reducer 0" in st["diag"]
    with pytest.raises(AssertionError):
        shuffle.check(st)
    monkeypatch.delenv("UDA_FAULT_MERGE_FLIP")
    clean_step(shuffle)


def test_unvalidated_steps_do_not_poll_the_fault_sites(shuffle, monkeypatch):
    """The sites count validate steps' rounds only: two unvalidated steps (6 rounds) leave the count at zero."""
    monkeypatch.setenv("UDA_FAULT_MERGE_SWAP", "4")
    for _ in range(2):
        st = shuffle.step(validate=False)
        assert st["records"] == 60_000
    st = shuffle.step()  # rounds 1..3 of the count
    assert st["order_errors"] == 0
    st = shuffle.step()  # round 4: this step's first
    assert st["order_errors"] == 1
    monkeypatch.delenv("UDA_FAULT_MERGE_SWAP")
    clean_step(shuffle)
