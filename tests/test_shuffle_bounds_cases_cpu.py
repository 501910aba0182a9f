"""The bounds cases of tests/shuffle_bounds_cases.py on the host, over synthetic sorted random 10-byte keys:
every builder returns ascending bounds of the right shape, the oracle's cells partition the records against a
brute-force walk, and every named case holds what its name says (cells of 0 records, a cell of 1 record, a
reducer with 0 records, a wholly empty round). tests/test_gpu_shuffle_bounds.py repeats the non-vacuity
checks on the real store."""
import random

import numpy as np
import pytest

from tests import shuffle_bounds_cases as sb

GEOMETRIES = [(1, 5), (3, 4), (4, 1), (2, 2), (2, 3), (2, 5), (2, 4), (1, 3), (1, 2), (1, 1)]


def _record(key, tag):
    return bytes([0x0B, 0x5B, 0x0A]) + key + b"\x5a" + bytes([65 + tag % 26]) * 90


def _parts(rng, n, runs):
    """n distinct random 10-byte keys dealt over `runs` sorted partitions (one may be empty)."""
    keys = set()
    while len(keys) < n:
        keys.add(bytes(rng.getrandbits(8) for _ in range(sb.KEY_LEN)))
    dealt = [[] for _ in range(runs)]
    for x, k in enumerate(sorted(keys)):
        dealt[rng.randrange(runs - 1)].append(_record(k, x))
    return [b"".join(run) + sb.EOF for run in dealt]


@pytest.fixture(scope="module")
def parts_by_dest():
    rng = random.Random(20261021)
    return [_parts(rng, n, 4) for n in (700, 701, 350)]


@pytest.fixture(scope="module")
def sorted_keys(parts_by_dest):
    return [sb.sorted_records(p)[1] for p in parts_by_dest]


def _key_bytes(rec):
    return bytes(rec[sb.KEY_OFF:sb.KEY_OFF + sb.KEY_LEN])


def _bound_bytes(b):
    return int(b[0]).to_bytes(8, "big") + (int(b[1]) >> 48).to_bytes(2, "big")


def test_keys_sort_in_byte_order(parts_by_dest):
    for parts in parts_by_dest:
        recs, keys = sb.sorted_records(parts)
        plain = sorted((r for p in parts for r in (p[o:o + sb.RECORD] for o in range(0, len(p) - 2, sb.RECORD))),
                       key=_key_bytes)
        assert [bytes(r) for r in recs] == plain
        assert [_bound_bytes(k) for k in keys] == [_key_bytes(r) for r in plain]
        assert any(len(p) == 2 for p in parts)  # an empty partition parses


def test_oracle_rejects_duplicate_keys_and_bad_framing():
    rec = _record(b"\x01" * 10, 0)
    with pytest.raises(AssertionError):
        sb.sorted_records([rec + sb.EOF, rec + sb.EOF])
    with pytest.raises(AssertionError):
        sb.partition_records(rec)
    with pytest.raises(AssertionError):
        sb.partition_records(rec[:-1] + sb.EOF)


@pytest.mark.parametrize("R,Q", GEOMETRIES)
@pytest.mark.parametrize("name", sb.CASES + ("mixed",))
def test_case_holds_what_its_name_says(parts_by_dest, sorted_keys, name, R, Q):
    C = R * Q
    bounds = sb.BUILDERS[name](sorted_keys, R, Q)
    assert bounds.dtype == np.uint64 and bounds.shape == (len(sorted_keys), C - 1, 2)
    assert all(sb.is_ascending(b) for b in bounds)
    streams, counts = sb.oracle(parts_by_dest, bounds, R, Q)
    sb.check_case(name, counts, R, Q)
    for d, parts in enumerate(parts_by_dest):
        recs, _ = sb.sorted_records(parts)
        # brute force: every record into the cell whose ends bracket its key bytes
        edges = [_bound_bytes(b) for b in bounds[d]]
        want = [[] for _ in range(C)]
        for r in recs:
            k = _key_bytes(r)
            c = [c for c in range(C) if (c == 0 or edges[c - 1] <= k) and (c == C - 1 or k < edges[c])]
            assert len(c) == 1
            want[c[0]].append(bytes(r))
        assert [[len(want[i * Q + q]) for q in range(Q)] for i in range(R)] == counts[d]
        for i in range(R):
            assert streams[d][i] == b"".join(b"".join(want[i * Q + q]) for q in range(Q)) + sb.EOF
        assert sum(len(s) - 2 for s in streams[d]) == len(recs) * sb.RECORD


@pytest.mark.parametrize("R,Q", [g for g in GEOMETRIES if g[0] * g[1] >= 4])
def test_key_hit_bounds_are_keys_and_the_triple_turns_on_the_low_bits(sorted_keys, R, Q):
    C = R * Q
    j = sb.key_hit_triple_at(C)
    for d, b in enumerate(sb.key_hit(sorted_keys, R, Q)):
        have = {(int(h), int(l)) for h, l in sorted_keys[d]}
        h, l = int(b[j + 1, 0]), int(b[j + 1, 1])
        assert (h, l) in have and (l >> 48) < 0xFFFF
        assert [(int(x), int(y)) for x, y in b[j:j + 3]] == [(h, 0), (h, l), (h, l + (1 << 48))]
        assert all((int(x), int(y)) in have for c, (x, y) in enumerate(b) if not j <= c < j + 3)
        # a split that ignored the low 16 bits, or took `<=` for `<`, would move the key out of its cell
        cells = sb.cell_of(sorted_keys[d], b)
        at = [x for x, k in enumerate(sorted_keys[d]) if (int(k[0]), int(k[1])) == (h, l)]
        assert len(at) == 1 and cells[at[0]] == j + 2 and list(cells).count(j + 2) == 1


def test_quantile_bound_opens_the_upper_cell(sorted_keys):
    b = sb.quantile(sorted_keys, 3, 4)
    for d, keys in enumerate(sorted_keys):
        cells = sb.cell_of(keys, b[d])
        for c, (h, l) in enumerate(b[d]):
            x = [x for x, k in enumerate(keys) if k[0] == h and k[1] == l]
            assert len(x) == 1 and cells[x[0]] == c + 1 and cells[x[0] - 1] == c


def test_pieces_needed():
    assert sb.piece_records(8192, 32 << 10) == 312 and sb.piece_records(100, 50) == 1
    assert sb.pieces_needed([[0, 1, 312], [313, 0, 1000]], 312) == 0 + 1 + 1 + 2 + 0 + 4
