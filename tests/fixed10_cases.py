"""Shared by the FIXED10 (TeraSort-shaped) merge tests: sorted runs whose keys are duplicated, tied on
their first 8 bytes, all-ones or skewed, and a pure-Python oracle of their merge.

A record is 104 bytes: 0b 5b 0a, the 10 key bytes, 5a, 90 value bytes 'A'..'Z'. The first six value
bytes spell the record's run (2 letters) and position (4 letters) in base 26, so all records of a case
differ and any change in the order of equal keys changes the merged bytes. The oracle is Python's stable
sort of a group's runs concatenated in run order: key, then run, then position, which is what both GPU
merges and the CPU heap merge promise."""
import functools

import numpy as np

L = 104
KEY = slice(3, 13)
EOF = b"\xff\xff"
K_SWEEP = (1, 2, 6, 65, 130, 256, 257)
CASES = ("all_equal", "few_distinct", "hi_tie", "extremes", "heavy_key", "identical_runs", "disjoint_runs",
         "ragged", "uniform")
ZERO_KEY = bytes(10)
ONES_KEY = b"\xff" * 10
HEAVY_KEY = bytes.fromhex("8000c3a55a3c0ff0117e")  # mid-range


def _letters(x, digits):
    """x (array) in base 26 as `digits` columns of 'A'..'Z', most significant first."""
    x = np.asarray(x, np.int64)
    return np.stack([(x // 26 ** (digits - 1 - d)) % 26 + 65 for d in range(digits)], axis=1).astype(np.uint8)


def sort_keys(keys):
    """(n, 10) uint8 key rows in ascending byte order."""
    keys = np.asarray(keys, np.uint8).reshape(-1, 10)
    return keys[np.lexsort(keys.T[::-1])]


def make_run(keys, run, rng):
    """A sorted run (record bytes, no EOF marker) of the given key rows, sorted here."""
    keys = sort_keys(keys)
    n = len(keys)
    assert run < 26 ** 2 and n < 26 ** 4
    a = np.empty((n, L), np.uint8)
    a[:, 0:3] = (0x0B, 0x5B, 0x0A)
    a[:, KEY] = keys
    a[:, 13] = 0x5A
    a[:, 14:] = rng.randint(65, 91, size=(n, 90))
    a[:, 14:16] = _letters(np.full(n, run), 2)
    a[:, 16:20] = _letters(np.arange(n), 4)
    return a.tobytes()


def records(run):
    return [run[i:i + L] for i in range(0, len(run), L)]


def oracle(runs, group_first=None):
    """The merge of every group's runs: stable sort by the 10 key bytes, groups in order."""
    gf = [0, len(runs)] if group_first is None else group_first
    out = []
    for g0, g1 in zip(gf[:-1], gf[1:]):
        recs = [rec for r in runs[g0:g1] for rec in records(r)]
        out += sorted(recs, key=lambda rec: rec[KEY])
    return b"".join(out)


def max_copies(runs, group_first=None):
    """The most records that share one key within one group."""
    gf = [0, len(runs)] if group_first is None else group_first
    best = 0
    for g0, g1 in zip(gf[:-1], gf[1:]):
        count = {}
        for r in runs[g0:g1]:
            for rec in records(r):
                count[rec[KEY]] = count.get(rec[KEY], 0) + 1
        best = max(best, max(count.values(), default=0))
    return best


def distinct_keys(rng, n):
    """n distinct random keys (none of them one of the special keys), unsorted."""
    keys = rng.randint(0, 256, size=(n + n // 8 + 8, 10)).astype(np.uint8)
    keys[:, 0] = np.clip(keys[:, 0], 1, 254)  # never 00*10 or ff*10
    keys = keys[keys[:, 0] != HEAVY_KEY[0]]
    keys = np.unique(keys, axis=0)
    assert len(keys) >= n
    return keys[rng.permutation(len(keys))[:n]]


def _row(key, n):
    return np.tile(np.frombuffer(key, np.uint8), (n, 1))


def _deal(keys, K):
    """Key rows dealt round-robin over K runs."""
    return [keys[r::K] for r in range(K)]


def _build(name, K, n, rng):
    """Per-run key rows of case `name`: K runs of about n records."""
    total = K * n
    if name == "all_equal":
        return [_row(HEAVY_KEY, n) for _ in range(K)]
    if name == "few_distinct":  # 60 % / 30 % / 10 %
        three = (bytes.fromhex("00112233445566778899"), HEAVY_KEY, bytes.fromhex("fffefdfcfbfaf9f8f7f6"))
        return [np.concatenate([_row(three[0], n * 6 // 10), _row(three[1], n * 3 // 10),
                                _row(three[2], n - n * 6 // 10 - n * 3 // 10)]) for _ in range(K)]
    if name == "hi_tie":  # 8 constant bytes; the 2 tail bytes vary, 0000 and ffff a few times per run
        out = []
        for _ in range(K):
            keys = _row(bytes.fromhex("5aa5c33c0ff06996") + bytes(2), n)
            tail = rng.randint(0, 65536, size=n)
            edge = min(4, n // 2)
            tail[:edge] = 0
            tail[n - edge:] = 0xFFFF
            keys[:, 8] = tail >> 8
            keys[:, 9] = tail & 0xFF
            out.append(keys)
        return out
    if name == "extremes":  # > 2048 of 00*10 and of ff*10 around random keys
        e = max(2100 // K + 1, 1)
        assert n > 2 * e
        mid = _deal(distinct_keys(rng, K * (n - 2 * e)), K)
        return [np.concatenate([_row(ZERO_KEY, e), mid[r], _row(ONES_KEY, e)]) for r in range(K)]
    if name == "heavy_key":  # 40 % one mid-range key, the rest distinct
        h = n * 4 // 10
        rest = _deal(distinct_keys(rng, K * (n - h)), K)
        return [np.concatenate([_row(HEAVY_KEY, h), rest[r]]) for r in range(K)]
    if name == "identical_runs":
        keys = distinct_keys(rng, n)
        return [keys for _ in range(K)]
    if name == "disjoint_runs":
        keys = sort_keys(distinct_keys(rng, total))
        return [keys[r * n:(r + 1) * n] for r in range(K)]
    if name == "uniform":
        return _deal(distinct_keys(rng, total), K)
    raise KeyError(name)


# ragged: one run with 90 % of the records; empty runs, runs of 1 record, and runs shorter than half the
# sample step of every cell capacity the tests use (step / 2 is 25 at 2048, 11 at 1024, 5 at 512)
RAGGED = (13500, 0, 1, 3, 0, 700, 1, 7, 12, 0, 20, 750, 2, 1)


@functools.lru_cache(maxsize=None)
def case(name, K=6, n=2500):
    """(runs, group_first or None) of a named case; K runs of n records each (ragged: its own shape)."""
    rng = np.random.RandomState(1000 + 17 * CASES.index(name) + K)
    if name == "ragged":
        keys = distinct_keys(rng, sum(RAGGED))
        cuts = np.cumsum((0,) + RAGGED)
        rows = [keys[a:b] for a, b in zip(cuts[:-1], cuts[1:])]
    else:
        rows = _build(name, K, n, rng)
    return tuple(make_run(k, r, rng) for r, k in enumerate(rows)), None


@functools.lru_cache(maxsize=None)
def grouped(name):
    """G = 3: a group of one run, a group whose three runs are all empty, and the named case's 6 runs."""
    rng = np.random.RandomState(77)
    runs, _ = case(name)
    single = make_run(distinct_keys(rng, 900), 0, rng)
    # run numbers in the values follow the position in the whole list
    body = tuple(_renumber(r, 4 + i) for i, r in enumerate(runs))
    return (single, b"", b"", b"") + body, (0, 1, 4, 4 + len(runs))


def _renumber(run, number):
    a = np.frombuffer(run, np.uint8).reshape(-1, L).copy()
    a[:, 14:16] = _letters(np.full(len(a), number), 2)
    return a.tobytes()


def sweep_case(name, K):
    """`name` at K runs with at most 40 000 records in all (at least 6 per run)."""
    n = 2500 if K <= 6 else max(6, min(2500, 36000 // K))
    return case(name, K, n)


@functools.lru_cache(maxsize=None)
def expected(name, K=6, n=2500):
    return oracle(*case(name, K, n))
