"""delivery_schedule (csrc/gpu/delivery_schedule.h): the D2H pieces of a round and their issue order.
Per reducer the pieces tile its bytes in ascending order; pack_index numbers the reducer-major list the
device piece descriptors keep; "wave" order never issues a reducer's piece w+1 before any reducer's
piece w; "reducer" order is the list the copy thread walked before the order became a choice."""
import pytest

L = 104
PIECE_RECS = 20
PIECE = PIECE_RECS * L

CASES = {
    "mixed": [0, 1, 5 * PIECE_RECS, PIECE_RECS, PIECE_RECS + 1],
    "all_zero": [0, 0, 0, 0],
    "one_reducer": [3 * PIECE_RECS + 7],
    "one_record_each": [1, 1, 1],
    "none": [],
}


def reducer_major(group_recs, piece=PIECE):
    """The enumeration ShuffleJob::round_pieces() and copy_loop wrote out twice before: reducers back to
    back in the output slot, each cut into pieces of at most `piece` bytes."""
    out, goff = [], 0
    for i, n in enumerate(group_recs):
        nbytes, off = n * L, 0
        while off < nbytes:
            ln = min(piece, nbytes - off)
            out.append(dict(reducer=i, src_off=goff + off, len=ln, pack_index=len(out),
                            last_of_reducer=off + ln >= nbytes))
            off += ln
        goff += nbytes
    return out


@pytest.mark.parametrize("order", ["wave", "reducer"])
@pytest.mark.parametrize("case", sorted(CASES))
def test_pieces_tile_every_reducer_in_ascending_order(native, case, order):
    recs = CASES[case]
    sched = native.delivery_schedule(recs, PIECE, order, L)
    starts, goff = [], 0
    for n in recs:
        starts.append(goff)
        goff += n * L
    for i, n in enumerate(recs):
        mine = [p for p in sched if p["reducer"] == i]
        pos = starts[i]
        for p in mine:  # contiguous and ascending in issue order
            assert p["src_off"] == pos
            assert 0 < p["len"] <= PIECE and p["len"] % L == 0
            pos += p["len"]
        assert pos == starts[i] + n * L  # covers exactly its bytes
        assert [p["last_of_reducer"] for p in mine] == [False] * (len(mine) - 1) + [True] * (1 if n else 0)
        assert len(mine) == -(-n * L // PIECE)
    assert all(0 <= p["reducer"] < len(recs) for p in sched)
    assert sum(p["last_of_reducer"] for p in sched) == sum(1 for n in recs if n > 0)


@pytest.mark.parametrize("order", ["wave", "reducer"])
@pytest.mark.parametrize("case", sorted(CASES))
def test_pack_index_is_the_reducer_major_position(native, case, order):
    recs = CASES[case]
    want = reducer_major(recs)
    sched = native.delivery_schedule(recs, PIECE, order, L)
    assert sorted(p["pack_index"] for p in sched) == list(range(len(want)))
    for p in sched:
        assert p == want[p["pack_index"]]


@pytest.mark.parametrize("case", sorted(CASES))
def test_reducer_order_is_the_former_list(native, case):
    assert native.delivery_schedule(CASES[case], PIECE, "reducer", L) == reducer_major(CASES[case])


@pytest.mark.parametrize("case", sorted(CASES))
def test_wave_order_goes_wave_by_wave(native, case):
    recs = CASES[case]
    sched = native.delivery_schedule(recs, PIECE, "wave", L)
    seen = [0] * len(recs)
    waves = []  # (wave, reducer) in issue order
    for p in sched:
        waves.append((seen[p["reducer"]], p["reducer"]))
        seen[p["reducer"]] += 1
    # no reducer's piece w+1 before piece w of any reducer that has one; reducer order inside a wave
    assert waves == sorted(waves)
    if case == "mixed":
        assert [p["reducer"] for p in sched] == [1, 2, 3, 4, 2, 4, 2, 2, 2]
        assert sched[5]["len"] == L  # reducer 4's remainder: one record


def test_piece_size_is_cut_to_whole_records(native):
    sched = native.delivery_schedule([50], PIECE + 57, "wave", L)
    assert [p["len"] for p in sched] == [PIECE, PIECE, 10 * L]
    tiny = native.delivery_schedule([3], 1, "wave", L)  # smaller than a record: one record per piece
    assert [p["len"] for p in tiny] == [L, L, L]


def test_default_order_is_wave_and_unknown_orders_are_refused(native):
    recs = CASES["mixed"]
    assert native.delivery_schedule(recs, PIECE) == native.delivery_schedule(recs, PIECE, "wave", L)
    for bad in ("", "Wave", "round"):
        with pytest.raises(ValueError):
            native.delivery_schedule(recs, PIECE, bad, L)
