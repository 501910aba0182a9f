"""Shared by the tests of ShuffleJob on lopsided key-range cells (tests/test_gpu_shuffle_bounds.py and its CPU
companion): a pure-Python oracle of what every reducer must receive under given cell bounds, and builders of
bounds that leave cells empty, holding one record, or holding everything.

Nothing here touches the native module. The oracle works on the partitions as ShuffleJob.read_partition
returns them: 104-byte IFile records (VInt(11) VInt(91) Text(10) Text(90)) followed by the EOF marker ff ff.
The key is bytes 3..12 of a record; `hi` is its first 8 bytes big-endian, `lo16` its last 2. Keys and bounds
travel as (n, 2) uint64 rows (hi, lo16 << 48), the layout of the job's samples and of set_bounds. Byte order
of the 10-byte key is the order of (hi, lo16).

Destination d with bounds B[d] (C - 1 rows, C = R * Q) has C cells: a record belongs to cell c iff
B[d][c-1] <= key < B[d][c], the ends open. Cell c = i * Q + q is reducer i, round q. Reducer i must receive
its records in key order followed by ff ff, whatever the cells hold."""
import numpy as np

RECORD = 104
KEY_OFF = 3
KEY_LEN = 10
EOF = b"\xff\xff"
U64_MAX = 0xFFFFFFFFFFFFFFFF
LOW = (0, 0)                       # no key is below it
HIGH = (U64_MAX, 0xFFFF << 48)     # only the all-ones key is not below it

CASES = ("quantile", "all_low", "all_high", "key_hit", "collapsed")  # at any world; "mixed" needs world > 1


# ------------------------------------------------------------------------------------------------ oracle
def partition_records(part):
    """(n, 104) uint8 records of one partition; the EOF marker is checked and dropped."""
    part = bytes(part)
    assert len(part) >= len(EOF) and part[-2:] == EOF, "partition without its EOF marker"
    assert (len(part) - 2) % RECORD == 0, "partition does not hold whole records"
    return np.frombuffer(part, np.uint8, len(part) - 2).reshape(-1, RECORD)


def record_keys(recs):
    """(n, 2) uint64 (hi, lo16 << 48) of (n, 104) records."""
    k = recs[:, KEY_OFF:KEY_OFF + KEY_LEN].astype(np.uint64)
    hi = np.zeros(len(recs), np.uint64)
    for b in range(8):
        hi = (hi << np.uint64(8)) | k[:, b]
    lo16 = (k[:, 8] << np.uint64(8)) | k[:, 9]
    return np.stack([hi, lo16 << np.uint64(48)], axis=1)


def sorted_records(parts):
    """All records of a destination's partitions in byte order of their keys, and those keys. The keys must
    be distinct (TeraGen draws them: a precondition of the byte-for-byte comparison, not a property under
    test)."""
    recs = np.concatenate([partition_records(p) for p in parts]) if parts else np.zeros((0, RECORD), np.uint8)
    keys = record_keys(recs)
    order = np.lexsort((keys[:, 1], keys[:, 0]))
    recs, keys = recs[order], keys[order]
    same = (keys[1:] == keys[:-1]).all(axis=1)
    assert not same.any(), "two records of one destination share a key"
    return recs, keys


def cell_of(keys, bounds):
    """Cell index of every key: the number of bounds that are <= the key."""
    bounds = np.asarray(bounds, np.uint64).reshape(-1, 2)
    assert not (bounds[:, 1] & np.uint64((1 << 48) - 1)).any(), "a bound's low word is lo16 << 48"
    cell = np.zeros(len(keys), np.int64)
    for bh, bl in bounds:
        cell += (bh < keys[:, 0]) | ((bh == keys[:, 0]) & (bl <= keys[:, 1]))
    return cell


def is_ascending(bounds):
    b = [(int(h), int(l)) for h, l in np.asarray(bounds, np.uint64).reshape(-1, 2)]
    return all(x <= y for x, y in zip(b, b[1:]))


def expected_dest(recs, keys, bounds, R, Q):
    """One destination: ([R] expected streams, [R][Q] record counts) from its sorted records."""
    C = R * Q
    bounds = np.asarray(bounds, np.uint64).reshape(-1, 2)
    assert bounds.shape == (C - 1, 2) and is_ascending(bounds)
    cell = cell_of(keys, bounds)
    assert (np.diff(cell) >= 0).all()  # ascending bounds over ascending keys
    counts = np.bincount(cell, minlength=C).reshape(R, Q)
    streams, pos = [], 0
    for i in range(R):
        n = int(counts[i].sum())
        streams.append(recs[pos:pos + n].tobytes() + EOF)
        pos += n
    assert pos == len(recs)
    return streams, [[int(x) for x in row] for row in counts]


def oracle(parts_by_dest, bounds, R, Q):
    """parts_by_dest[d]: every partition for destination d, from every rank and map. bounds: (world, C-1, 2).
    Returns (streams[d][i], counts[d][i][q])."""
    bounds = np.asarray(bounds, np.uint64)
    assert bounds.shape == (len(parts_by_dest), R * Q - 1, 2)
    out = [expected_dest(*sorted_records(parts), bounds[d], R, Q) for d, parts in enumerate(parts_by_dest)]
    return [s for s, _ in out], [c for _, c in out]


def pieces_needed(counts_d, piece_records):
    """D2H pieces of one destination's step: every non-empty (reducer, round) cell in pieces of piece_records."""
    return sum(-(-n // piece_records) for row in counts_d for n in row if n > 0)


def piece_records(kv_buf_bytes, d2h_piece_bytes):
    """Records per D2H piece: whole delivery buffers of whole records."""
    buf = max(1, kv_buf_bytes // RECORD)
    return max(1, d2h_piece_bytes // (buf * RECORD)) * buf


# ------------------------------------------------------------------------------------------------ builders
# Each takes the per-destination sorted keys ((n_d, 2) uint64) and (R, Q); returns (world, C-1, 2) uint64.
def _quantile_one(keys, C):
    n = len(keys)
    assert n >= C, "fewer keys than cells"
    return np.asarray([keys[min(n - 1, n * c // C)] for c in range(1, C)], np.uint64).reshape(C - 1, 2)


def _const_one(bound, C):
    return np.asarray([bound] * (C - 1), np.uint64).reshape(C - 1, 2)


def quantile(sorted_keys, R, Q):
    return np.stack([_quantile_one(k, R * Q) for k in sorted_keys])


def all_low(sorted_keys, R, Q):
    """Everything in the last cell."""
    return np.stack([_const_one(LOW, R * Q) for _ in sorted_keys])


def all_high(sorted_keys, R, Q):
    """Everything in cell 0."""
    return np.stack([_const_one(HIGH, R * Q) for _ in sorted_keys])


def key_hit_triple_at(C):
    """First bound index of key_hit's (h, 0), (h, l), (h, l + 1) triple, or None where C - 1 < 3."""
    return None if C - 1 < 3 else max(0, (C - 1) // 2 - 1)


def _key_hit_one(keys, C):
    b = _quantile_one(keys, C)
    j = key_hit_triple_at(C)
    if j is None:
        return b
    n = len(keys)
    # an existing key strictly between the keys of bounds j - 1 and j + 3, so that the triple stays in order
    lo = min(n - 1, n * j // C) + 1 if j > 0 else 0
    hi = min(n - 1, n * (j + 4) // C) if j + 3 < C - 1 else n
    prev = (int(b[j - 1, 0]), int(b[j - 1, 1])) if j > 0 else LOW
    nxt = (int(b[j + 3, 0]), int(b[j + 3, 1])) if j + 3 < C - 1 else HIGH
    for x in sorted(range(lo, hi), key=lambda x: abs(x - (lo + hi) // 2)):
        h, l = int(keys[x, 0]), int(keys[x, 1]) >> 48
        if l < 0xFFFF and prev <= (h, 0) and (h, (l + 1) << 48) <= nxt:
            b[j:j + 3] = [(h, 0), (h, l << 48), (h, (l + 1) << 48)]
            return b
    raise AssertionError("key_hit: no key leaves room for the triple")


def key_hit(sorted_keys, R, Q):
    """Every bound is the key of a record (that record opens the upper cell), but for one triple (h, 0), (h, l),
    (h, l + 1) around an existing key (h, l): a cell that ends just below the key, then a cell of exactly that
    record, both decided by the low 16 bits alone."""
    return np.stack([_key_hit_one(k, R * Q) for k in sorted_keys])


def collapsed_properties(R, Q):
    """What `collapsed` holds at (R, Q): reducer 0's first round is empty; some reducer has an empty last round
    after data; some reducer has an empty round between two rounds with data."""
    return dict(first=R * Q >= 2,
                last_after_data=(R >= 2 and Q >= 2) or Q >= 3,
                middle=Q >= 3 and (R >= 3 or Q >= 5 or (R == 2 and Q >= 4)))


def collapsed_cells(R, Q):
    """The cells `collapsed` empties (sorted)."""
    C = R * Q
    want = collapsed_properties(R, Q)
    empty = set()

    def data(i, qs):
        return any(i * Q + q not in empty for q in qs)

    if want["first"]:
        empty.add(0)
    if want["last_after_data"]:
        i = R - 1
        empty.add(i * Q + Q - 1)
        assert data(i, range(Q - 1))
    if want["middle"]:
        for i, q in [(i, q) for i in sorted(range(R), key=lambda i: abs(i - R // 2)) for q in range(1, Q - 1)]:
            c = i * Q + q
            if c in empty or c + 1 in empty and c + 1 == C - 1:
                continue
            trial = empty | {c}
            if any(i * Q + a not in trial for a in range(q)) and any(i * Q + a not in trial for a in range(q + 1, Q)):
                empty.add(c)
                break
        else:
            raise AssertionError("collapsed: no room for an empty middle round")
    if Q == 1 and C >= 4:
        empty.add(C // 2)  # one more reducer without records, by a pair of equal bounds
    assert not (C - 1 in empty and C - 2 in empty)
    return sorted(empty)


def _collapsed_one(keys, R, Q):
    C = R * Q
    b = _quantile_one(keys, C)
    for c in collapsed_cells(R, Q):  # ascending: a run of empty cells chains
        if c == 0:
            b[0] = LOW
        elif c == C - 1:
            b[C - 2] = HIGH
        else:
            b[c] = b[c - 1]
    return b


def collapsed(sorted_keys, R, Q):
    """Quantile bounds with pairs of adjacent bounds made equal (and the first pulled to the bottom, the last
    to the top where the last cell is emptied): see collapsed_properties."""
    return np.stack([_collapsed_one(k, R, Q) for k in sorted_keys])


def mixed(sorted_keys, R, Q):
    """world > 1: destination 0 all_low, the last destination all_high, the ones between quantile: the ranks
    disagree about which rounds are empty."""
    W, C = len(sorted_keys), R * Q
    assert W > 1
    out = []
    for d, k in enumerate(sorted_keys):
        out.append(_const_one(LOW, C) if d == 0 else _const_one(HIGH, C) if d == W - 1 else _quantile_one(k, C))
    return np.stack(out)


BUILDERS = dict(quantile=quantile, all_low=all_low, all_high=all_high, key_hit=key_hit, collapsed=collapsed,
                mixed=mixed)


# ------------------------------------------------------------------------------------------------ non-vacuity
def _only_cell(counts_d, i, q):
    total = sum(map(sum, counts_d))
    assert total > 0 and counts_d[i][q] == total, counts_d


def _all_full(counts_d):
    assert all(n > 0 for row in counts_d for n in row), counts_d


def check_case(name, counts, R, Q):
    """The named case really holds what its name says, by the oracle's cell counts [d][i][q]."""
    C, W = R * Q, len(counts)
    for d, cd in enumerate(counts):
        assert len(cd) == R and all(len(row) == Q for row in cd)
        flat = [n for row in cd for n in row]
        kind = name if name != "mixed" else "all_low" if d == 0 else "all_high" if d == W - 1 else "quantile"
        if kind == "quantile":
            _all_full(cd)
        elif kind == "all_low":
            _only_cell(cd, R - 1, Q - 1)  # every other reducer without a record, rounds 0 .. Q-2 wholly empty
        elif kind == "all_high":
            _only_cell(cd, 0, 0)          # every later round wholly empty: every EOF of the last round alone
        elif kind == "key_hit":
            j = key_hit_triple_at(C)
            if j is None:
                _all_full(cd)
            else:  # cells j+1 (ends just below the key) and j+2 (the key alone); everything else has data
                assert flat[j + 1] == 0 and flat[j + 2] == 1, flat
                assert all(n > 0 for c, n in enumerate(flat) if c != j + 1), flat
        elif kind == "collapsed":
            empty = collapsed_cells(R, Q)
            assert [c for c, n in enumerate(flat) if n == 0] == empty, (flat, empty)
            want = collapsed_properties(R, Q)
            got = dict(first=cd[0][0] == 0,
                       last_after_data=any(row[-1] == 0 and any(row[:-1]) for row in cd),
                       middle=any(row[q] == 0 and any(row[:q]) and any(row[q + 1:])
                                  for row in cd for q in range(1, Q - 1)))
            assert got == want, (got, want, cd)
            if Q == 1:
                assert sum(1 for row in cd if not any(row)) >= min(2, R - 1), cd
        else:
            raise AssertionError(f"unknown case {name}")
    if name == "mixed":
        assert W > 1
