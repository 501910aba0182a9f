"""Shared by the tests of the key-range round planner (csrc/gpu/generic_rounds.hip: plan_generic_rounds and
plan_progressive_split, with the partial mode of the F1 index they run on): a pure-Python oracle of both
planners and inputs placed on the kernels' edges.

Nothing here touches the native module. Record framing, the VInt codec and the key order of the byte kinds
come from tests/generic_cases.py, the sortable word of the numeric classes from tests/key_order_cases.py.

The planner chooses its bound strings from a sample of chunk-leading keys; which ones it takes is a matter of
balance, not of correctness, so the oracle does not predict them. It states what every plan must satisfy: the
bounds are chunk-leading keys (cut to sample_key bytes) in strictly ascending order, and every position is
exactly the start of the run's first record that is not below its bound. The progressive split has no such
freedom: expected_split gives the one right answer, the bound included.

`geo` is native.gpu_generic_geometry() joined with native.gpu_rounds_geometry(): the cases compute their
offsets from it and move when the kernels do. A case is built once per (name, geo) and never changed."""
import functools
import random

from tests import generic_cases as gc
from tests import key_order_cases as ko
from tests.generic_cases import BYTES, EOF, LONG, TEXT, read_vlong, record, stream, text, walk


class Hadoop(str):
    """A numeric key class under mapred.uda.key.order=hadoop (a plain str: the class under the default order)."""


def key_order(cls):
    return "hadoop" if isinstance(cls, Hadoop) else "reference"


# ------------------------------------------------------------------------------------------------ oracle
def sort_content(cls, key):
    """The bytes the planner orders a key by: the content of a Text / BytesWritable / raw key, the 8-byte
    big-endian sortable word of a numeric key under Hadoop's order."""
    if isinstance(cls, Hadoop):
        return ko.sortable(str(cls), key).to_bytes(8, "big")
    return gc.content(cls, key)


def records_below(buf, limit):
    """[(start, end, key)] of the records of buf that start below `limit` (a record boundary)."""
    out, pos = [], 0
    while pos < limit:
        kl, a = read_vlong(buf, pos)
        vl, b = read_vlong(buf, pos + a)
        assert kl >= 0 and vl >= 0, (pos, kl, vl)
        out.append((pos, pos + a + b + kl + vl, bytes(buf[pos + a + b:pos + a + b + kl])))
        pos = out[-1][1]
    assert pos == limit, (pos, limit)
    return out


def record_bytes(buf):
    """Where the records of a whole run end: at the EOF marker, or at the stream's end."""
    return walk(buf, require_eof=False)[1]


def first_not_below(buf, limit, cls, bound):
    """The start of the first record below `limit` whose sort_content is >= bound (bytes compare as the key
    order does: unsigned, a prefix first); `limit` if there is none."""
    for start, _, key in records_below(buf, limit):
        if sort_content(cls, key) >= bound:
            return start
    return limit


def complete_prefix(window, avail):
    """The end of the last whole record inside window[:avail]. The EOF marker ends the walk; a header or a body
    cut by `avail` is not counted."""
    buf, pos = window[:avail], 0
    while True:
        try:
            kl, a = read_vlong(buf, pos)
            vl, b = read_vlong(buf, pos + a)
        except gc.CorruptStream:
            return pos
        if kl == -1 and vl == -1:
            return pos
        assert kl >= 0 and vl >= 0, (pos, kl, vl)
        if pos + a + b + kl + vl > avail:
            return pos
        pos += a + b + kl + vl


def chunk_leading_keys(streams, cls, geo):
    """For every f1_chunk-sized chunk of every run: sort_content, cut to sample_key bytes, of the first record
    that starts at or after the chunk's first byte (and below the run's record bytes). A set."""
    chunk, cut = geo["f1_chunk"], geo["sample_key"]
    out = set()
    for s in streams:
        recs = records_below(s, record_bytes(s))
        i = 0
        for c0 in range(0, len(s), chunk):
            while i < len(recs) and recs[i][0] < c0:
                i += 1
            if i < len(recs):
                out.add(sort_content(cls, recs[i][2])[:cut])
    return out


def _merged(runs, cls):
    """Records of the runs (lists of (key, value)) in merged order: sort_content, then run, then position."""
    tagged = [(sort_content(cls, k), r, i, k, v) for r, run in enumerate(runs) for i, (k, v) in enumerate(run)]
    tagged.sort(key=lambda t: t[:3])
    return [record(k, v) for _, _, _, k, v in tagged]


def _header(buf, pos):
    a = read_vlong(buf, pos)[1]
    return a + read_vlong(buf, pos + a)[1]


def _slice_records(buf, a, b):
    """(key, value) of the records of buf[a:b], both record boundaries."""
    return [(key, bytes(buf[a + s + _header(buf, a + s) + len(key):a + e])) for s, e, key in records_below(buf[a:b], b - a)]


def want_rounds(streams, round_bytes):
    return max(1, -(-sum(len(s) for s in streams) // round_bytes))


def check_plan(streams, cls, round_bytes, plan, geo):
    """Assert everything a round plan owes (see the module docstring); `plan` as gpu_plan_generic_rounds
    returns it."""
    rounds, pos, bounds = plan["rounds"], plan["pos"], list(plan["bounds"])
    K = len(streams)
    want = want_rounds(streams, round_bytes)
    # 1. shape (the number of rounds against `want` comes last, so a plan with too many rounds still has
    # its bounds and positions checked)
    assert rounds == len(bounds) + 1 and rounds >= 1, (rounds, len(bounds))
    assert len(pos) == K and all(len(p) == rounds + 1 for p in pos)
    if not bounds:
        assert [list(p) for p in pos] == [[0, len(s)] for s in streams]
    # 2. the bounds
    assert all(a < b for a, b in zip(bounds, bounds[1:])), bounds
    leading = chunk_leading_keys(streams, cls, geo)
    for b in bounds:
        assert b in leading, b
    # 3. the positions, exactly
    ends = [record_bytes(s) for s in streams]
    for k, s in enumerate(streams):
        assert pos[k][0] == 0 and pos[k][rounds] == len(s), (k, pos[k])
        for q in range(1, rounds):
            assert pos[k][q] == first_not_below(s, ends[k], cls, bounds[q - 1]), (k, q, bounds[q - 1])
    # 4. the largest round
    assert plan["max_round_bytes"] == max(sum(pos[k][q + 1] - pos[k][q] for k in range(K)) for q in range(rounds))
    # 5. whatever the bounds are: the rounds merged one after the other are the merge of the whole runs
    whole = _merged([_slice_records(s, 0, ends[k]) for k, s in enumerate(streams)], cls)
    by_round, seen = [], set()
    for q in range(rounds):
        parts = []
        for k, s in enumerate(streams):
            a, b = min(pos[k][q], ends[k]), min(pos[k][q + 1], ends[k])
            assert a <= b
            parts.append(_slice_records(s, a, b))
        keys = {sort_content(cls, key) for part in parts for key, _ in part}
        assert not (keys & seen), (q, sorted(keys & seen)[:3])
        seen |= keys
        by_round += _merged(parts, cls)
    assert by_round == whole
    # 1. again: no more rounds than round_bytes asks for
    assert rounds <= want, f"{rounds} rounds planned, want = ceil(total / round_bytes) = {want}"


def make_plan(streams, cls, bounds):
    """The plan that splits the runs by `bounds`, as the planner would report it (for the oracle's own tests)."""
    ends = [record_bytes(s) for s in streams]
    pos = [[0] + [first_not_below(s, ends[k], cls, b) for b in bounds] + [len(s)] for k, s in enumerate(streams)]
    rounds = len(bounds) + 1
    return {"rounds": rounds, "pos": pos, "bounds": list(bounds),
            "max_round_bytes": max(sum(p[q + 1] - p[q] for p in pos) for q in range(rounds))}


def expected_split(windows, avail, final, cls, geo):
    """What plan_progressive_split must return, exactly."""
    cut = geo["sample_key"]
    complete = [complete_prefix(w, a) for w, a in zip(windows, avail)]
    out = {"complete": complete, "split": [0] * len(windows), "bounded": False, "bound": b""}
    if all(final):
        out["split"] = list(complete)
        return out
    if any(c == 0 for c, f in zip(complete, final) if not f):
        return out
    bound = min(sort_content(cls, records_below(w, c)[-1][2])[:cut]
                for w, c, f in zip(windows, complete, final) if not f)
    out["bounded"], out["bound"] = True, bound
    out["split"] = [first_not_below(w, c, cls, bound) for w, c in zip(windows, complete)]
    return out


# ------------------------------------------------------------------------------------------------ plan cases
class PlanCase:
    def __init__(self, name, cls, streams, round_bytes, **meta):
        self.name, self.cls, self.streams, self.round_bytes, self.meta = name, cls, tuple(streams), round_bytes, meta
        for s in self.streams:  # every run is sorted under the case's order
            cs = [sort_content(cls, k) for _, _, k in records_below(s, record_bytes(s))]
            assert cs == sorted(cs), name
        self.want = want_rounds(self.streams, round_bytes)


ROUND_BYTES = 16 << 10


def _by(cls, recs):
    return sorted(recs, key=lambda kv: sort_content(cls, kv[0]))


def _distinct_text(rng, n, lo=22, hi=62):
    keys = set()
    while len(keys) < n:
        keys.add(bytes(rng.choice(b"abcdefghijklmnopqrstuvwxyz") for _ in range(rng.randint(lo, hi))))
    return sorted(keys)


def _uniform_text(rng):
    """5 runs of 10..26 KiB: distinct keys of 22..62 bytes (no two records of the case share a key)."""
    sizes = [10 << 10, 14 << 10, 18 << 10, 22 << 10, 26 << 10]
    keys = _distinct_text(rng, sum(sizes) // 60)
    rng.shuffle(keys)
    runs, at = [], 0
    for size in sizes:
        recs, total = [], 0
        while total < size:
            recs.append((text(keys[at]), rng.randbytes(rng.randint(20, 60))))
            total += len(record(*recs[-1]))
            at += 1
        runs.append(stream(_by(TEXT, recs)))
    return runs


def _short_text(rng, n, prefix=b""):
    return [(text(prefix + b"%06d" % rng.randrange(10 ** 6) + bytes(rng.choice(b"xyz") for _ in range(rng.randint(0, 30)))),
             rng.randbytes(rng.randint(10, 70))) for _ in range(n)]


def _long_records(geo, rng):
    """Short records (about 60 bytes) with records of 5..13 KB among them, so chunks without a record start.
    Run 0 opens with a long record that ends 100 bytes into a chunk (the parallel index takes the run), run 1
    ends with one, run 2 has two in a row (the second a long *key*), run 3 has one of just over three chunks
    in its middle, run 4 has none. The record after a long one is the first to start in its chunk."""
    chunk = geo["f1_chunk"]

    def enlarge(recs, i, size, long_key=False):
        k, v = recs[i]
        c = gc.content(TEXT, k)
        if long_key:  # the content keeps its place in the order: it only grows
            recs[i] = (text(c + bytes(rng.choice(b"ab") for _ in range(size))), v)
        else:
            recs[i] = (k, rng.randbytes(size))

    runs = []
    recs = _by(TEXT, _short_text(rng, 300))
    recs[0] = (recs[0][0], rng.randbytes(2 * chunk + 100 - len(record(recs[0][0], b"")) - 2))  # a 3-byte VInt(v)
    assert len(record(*recs[0])) == 2 * chunk + 100
    runs.append(recs)
    recs = _by(TEXT, _short_text(rng, 300))
    enlarge(recs, len(recs) - 1, 5000)
    runs.append(recs)
    recs = _by(TEXT, _short_text(rng, 350))
    enlarge(recs, 120, 7000)
    enlarge(recs, 121, 6000, long_key=True)
    runs.append(recs)
    recs = _by(TEXT, _short_text(rng, 400))
    enlarge(recs, 200, 3 * chunk + 100)
    runs.append(recs)
    runs.append(_by(TEXT, _short_text(rng, 350)))
    return [stream(r) for r in runs]


def shared_prefix_body(geo):
    rng = random.Random("rounds-cases/shared-prefix/body")
    return bytes(rng.choice(b"pqrs") for _ in range(300))


def _shared_prefix(geo, rng):
    """Contents that are prefixes of one body P, of sample_key - 1, sample_key and sample_key + 1 bytes, and
    P[:sample_key] followed by other tails up to 127, 128 (a 2-byte Text VInt) and 300 bytes. Every key of
    sample_key bytes or more truncates to P[:sample_key]; the one shorter key is below it, the equal one is
    not. Only run 0 holds the shorter key (at its front, where it is the one other chunk-leading key)."""
    n, body = geo["sample_key"], shared_prefix_body(geo)
    contents = [body[:n], body[:n + 1], body[:127], body[:128], body[:300]]
    contents += [body[:n] + t for t in (b"\x00", b"\x00\x00", b"\xff", b"a")]
    for ln in (127, 128, 300):
        contents += [body[:n] + bytes(rng.choice(b"\x00pq\xff") for _ in range(ln - n)) for _ in range(6)]
    runs = []
    for r in range(4):
        recs = [(text(rng.choice(contents)), b"%d.%d" % (r, i) + rng.randbytes(rng.randint(0, 40))) for i in range(110)]
        if r == 0:
            recs += [(text(body[:n - 1]), b"short.%d" % i) for i in range(5)]
        runs.append(stream(_by(TEXT, recs)))
    return runs


HEAVY = b"m-the-heavy-key"


def _heavy_key(rng):
    """4 runs of about 20 KiB; 70 % of all records have the key HEAVY, the others distinct keys around it."""
    runs = []
    for r in range(4):
        light = [(text(k), rng.randbytes(rng.randint(20, 50))) for k in _distinct_text(rng, 150, 8, 30)]
        heavy = [(text(HEAVY), rng.randbytes(rng.randint(20, 50))) for _ in range(350)]
        runs.append(stream(_by(TEXT, light + heavy)))
    return runs


def _tiny_runs(rng):
    """7 runs: no bytes; the EOF marker alone; one record with and without the marker; one run below all
    others' keys (but the empty one); one above them; a normal run of about 30 KiB that opens with empty contents."""
    below = _by(TEXT, _short_text(rng, 20, prefix=b"a"))
    above = _by(TEXT, _short_text(rng, 20, prefix=b"z"))
    one = [(text(b"m5"), b"one")]
    runs = [b"", EOF, stream(one), stream(one, eof=False), stream(below), stream(above)]
    # the normal run makes the case a little more than two rounds: the first of three rounds is then the
    # smallest the planner makes, cut at its least samples
    normal = [(text(b""), b"e%d" % i) for i in range(3)]
    while sum(map(len, runs)) + len(stream(normal)) < 2 * ROUND_BYTES + 100:
        normal += _short_text(rng, 1, prefix=b"m")
    return runs + [stream(_by(TEXT, normal))]


def _eof_edges(geo, rng):
    """Record bytes of 0, 1, chunk - 1 and chunk - 2 modulo the chunk size, each with and without the EOF
    marker: the marker starts a chunk, follows a record that reaches one byte into a chunk, straddles two
    chunks, or ends one; without it the run ends on those offsets."""
    chunk = geo["f1_chunk"]
    runs = []
    for rb in (2 * chunk, 3 * chunk + 1, 3 * chunk - 1, 2 * chunk - 2):
        for eof in (True, False):
            recs = gc._run_of_length(rb + len(EOF), rng)
            s = stream(recs, eof=eof)
            assert record_bytes(s) == rb and len(s) == rb + (2 if eof else 0)
            runs.append(s)
    return runs


def _numeric(cls):
    return [ko.stream(r) for r in ko.make_runs(cls, (900, 1500, 2500), seed="rounds")]


def _bytes_runs(rng):
    runs = []
    for r in range(4):
        recs = [(gc.bytes_writable(rng.randbytes(rng.choice((0, 1, 3, 8, 20, 70, 100)))), rng.randbytes(rng.randint(0, 60)))
                for _ in range(250)]
        runs.append(stream(_by(BYTES, recs)))
    return runs


def _raw_runs(rng):
    """LongWritable under the default order: 8 raw bytes, the negatives after the positives."""
    runs = []
    for r in range(4):
        recs = [(rng.randint(-2 ** 63, 2 ** 63 - 1).to_bytes(8, "big", signed=True), rng.randbytes(rng.randint(0, 40)))
                for _ in range(600)]
        runs.append(stream(_by(LONG, recs)))
    return runs


def _fan_in(rng):
    """130 runs of 0..40 short records (every seventh run empty, one with the marker alone)."""
    runs = []
    for r in range(130):
        n = 0 if r % 7 == 3 else rng.randint(5, 40)
        runs.append(stream(_by(TEXT, _short_text(rng, n)), eof=r != 10))
    runs[3] = EOF
    return runs


def strided_round_bytes(geo):
    """A round of more chunks than the planner samples for it: with a little less than two rounds of input it
    samples every other chunk or so, not each one."""
    return (geo["samples_per_round"] + geo["samples_per_round"] // 2) * geo["f1_chunk"]


def _strided_sample(geo, rng):
    """3 runs, together just under two rounds of strided_round_bytes: records of 300..700 bytes with distinct
    keys, and in every run one record of two chunks and a half (its chunks hold no record start)."""
    chunk = geo["f1_chunk"]
    size = (2 * strided_round_bytes(geo) - 3 * chunk) // 3
    runs = []
    for r in range(3):
        recs, total = [], 0
        while total < size - 3 * chunk:
            recs.append((text(b"%d-%012d" % (r, rng.randrange(10 ** 12))), rng.randbytes(rng.randint(300, 700))))
            total += len(record(*recs[-1]))
        recs = _by(TEXT, recs)
        recs[len(recs) // 3] = (recs[len(recs) // 3][0], rng.randbytes(2 * chunk + chunk // 2))
        runs.append(stream(recs))
    return runs


REUSED = ("hdr-straddle", "entry-edge", "len-edges-text", "len-edges-bytes")
NUMERIC = {"int": ko.INT, "long": ko.LONG, "vlong": ko.VLONG, "float": ko.FLOAT}
PLAN_NAMES = (["uniform-text", "long-records", "shared-prefix", "heavy-key", "tiny-runs", "eof-at-chunk-edge"] +
              ["reused-" + n for n in REUSED] + ["numeric-" + n for n in NUMERIC] + ["bytes", "raw", "fan-in", "strided-sample"])
MISALIGNED = ("uniform-text", "long-records", "eof-at-chunk-edge")
MISALIGN = (1, 2, 7, 15)


def plan_case(name, geo):
    return _plan_case(name, tuple(sorted(geo.items())))


@functools.lru_cache(maxsize=None)
def _plan_case(name, geo_items):
    geo = dict(geo_items)
    rng = random.Random("rounds-cases/" + name)
    if name == "uniform-text":
        return PlanCase(name, TEXT, _uniform_text(rng), ROUND_BYTES)
    if name == "long-records":
        return PlanCase(name, TEXT, _long_records(geo, rng), ROUND_BYTES)
    if name == "shared-prefix":
        return PlanCase(name, TEXT, _shared_prefix(geo, rng), ROUND_BYTES)
    if name == "heavy-key":
        return PlanCase(name, TEXT, _heavy_key(rng), ROUND_BYTES)
    if name == "tiny-runs":
        return PlanCase(name, TEXT, _tiny_runs(rng), ROUND_BYTES, below=4, above=5)
    if name == "eof-at-chunk-edge":
        return PlanCase(name, TEXT, _eof_edges(geo, rng), ROUND_BYTES)
    if name.startswith("reused-"):
        c = gc.case(name[len("reused-"):], {k: v for k, v in geo.items() if k not in ("sample_key", "samples_per_round")})
        return PlanCase(name, c.key_class, c.streams, ROUND_BYTES)
    if name.startswith("numeric-"):
        cls = Hadoop(NUMERIC[name[len("numeric-"):]])
        return PlanCase(name, cls, _numeric(str(cls)), ROUND_BYTES // 2)
    if name == "bytes":
        return PlanCase(name, BYTES, _bytes_runs(rng), ROUND_BYTES)
    if name == "raw":
        return PlanCase(name, LONG, _raw_runs(rng), ROUND_BYTES)
    if name == "fan-in":
        return PlanCase(name, TEXT, _fan_in(rng), ROUND_BYTES)
    if name == "strided-sample":
        return PlanCase(name, TEXT, _strided_sample(geo, rng), strided_round_bytes(geo))
    raise KeyError(name)


# ------------------------------------------------------------------------------------------------ split cases
class SplitCall:
    """One call of plan_progressive_split: windows (each the true rest of its run from a record start that is
    not 0), how much of each has landed, and which windows reach their run's end."""

    def __init__(self, name, cls, windows, avail, final, geo):
        assert len(windows) == len(avail) == len(final) <= 64, (name, len(windows))
        assert all(0 <= a <= len(w) for w, a in zip(windows, avail))
        # a final window has landed whole (but for its marker): the planner may assume nothing follows it
        assert all(a >= len(w) - 2 for w, a, f in zip(windows, avail, final) if f)
        self.name, self.cls, self.geo = name, cls, geo
        self.windows, self.avail, self.final = tuple(windows), tuple(avail), tuple(final)

    @functools.cached_property
    def expected(self):
        """expected_split of the call, computed once for all the tests that compare with it."""
        return expected_split(self.windows, self.avail, self.final, self.cls, self.geo)

    def with_tail(self, fill):
        """The windows with the bytes that have not landed replaced: None (the true continuation), or a byte."""
        if fill is None:
            return list(self.windows)
        return [w[:a] + bytes([fill]) * (len(w) - a) for w, a in zip(self.windows, self.avail)]


TAILS = (None, 0xFF, 0x00)
SPLIT_FAMILIES = ("long-records", "shared-prefix", "eof-at-chunk-edge", "hdr-straddle", "entry-edge", "len-edges-text",
                  "numeric-int", "numeric-vlong", "numeric-float")


def _window(s, first):
    """The rest of run s from its record `first` (> 0), and the records of that window."""
    starts, _ = walk(s, require_eof=False)
    w = s[starts[first]:]
    return w, records_below(w, record_bytes(w))


def record_cuts(w, recs, j):
    """Values of avail around record j (>= 1) of a window: every byte from one before its start through two
    past its header, the middle of its key and of its value, and one before, at and after its end."""
    s, e, key = recs[j]
    h = _header(w, s)
    cuts = set(range(s - 1, s + h + 3)) | {s + h + len(key) // 2, (s + h + len(key) + e) // 2, e - 1, e, e + 1}
    return sorted(c for c in cuts if recs[1][0] <= c <= len(w))  # at least one whole record has landed


def end_cuts(w):
    """The whole window, and one and two bytes less: the EOF marker halved or missing."""
    return [len(w) - 2, len(w) - 1, len(w)]


def _spread(cuts, n, rng):
    cuts = sorted(set(cuts))
    return cuts if len(cuts) <= n else sorted(rng.sample(cuts, n))


FIRST = (1, 2, 3)  # the record a run's window starts at, by run % 3


def _around(streams, r, t, rng, n=20):
    """Windows of run r cut around the record at quantile t of the window, and at the window's end."""
    w, recs = _window(streams[r], FIRST[r % 3])
    j = max(1, min(len(recs) - 1, int(t * len(recs))))
    return [(w, c) for c in _spread(record_cuts(w, recs, j) + end_cuts(w), n, rng)]


def _flag_sets(name, cls, cut_windows, geo, short):
    """The calls over one list of (window, avail): all windows arriving; the first run's windows final and
    whole (with, with half of and without their marker); and, if asked for, three calls in which one arriving
    window holds no whole record (0 bytes, 1 byte, the first record's header alone)."""
    windows, avail = [w for w, _ in cut_windows], [a for _, a in cut_windows]
    n = len(windows)
    calls = [SplitCall(name + "-arriving", cls, windows, avail, [False] * n, geo)]
    first = [i for i in range(n) if windows[i] is windows[0]]
    mixed = list(avail)
    for i in first:
        mixed[i] = end_cuts(windows[i])[i % 3]
    calls.append(SplitCall(name + "-mixed", cls, windows, mixed, [i in first for i in range(n)], geo))
    if short:
        for k, a in ((0, 0), (n // 2, 1), (n - 1, _header(windows[n - 1], 0))):
            cut = list(avail)
            cut[k] = a
            calls.append(SplitCall(f"{name}-short{a}", cls, windows, cut, [False] * n, geo))
    return calls


def _calls_of(name, cls, streams, rng, quantiles, geo, runs=None, short=False):
    """Per quantile a call over three runs (taken in turn) in the flag sets of _flag_sets, and one call of
    whole final windows of every run."""
    runs = list(range(len(streams))) if runs is None else runs
    calls = []
    for i, t in enumerate(quantiles):
        three = [runs[(3 * i + d) % len(runs)] for d in range(min(3, len(runs)))]
        cut_windows = [wc for r in three for wc in _around(streams, r, t, rng)]
        calls += _flag_sets(f"{name}@{t}", cls, cut_windows, geo, short and i == 0)
    windows = [_window(streams[r], FIRST[r % 3])[0] for r in runs[:21] for _ in range(3)]
    calls.append(SplitCall(name + "-final", cls, windows, [end_cuts(w)[i % 3] for i, w in enumerate(windows)],
                           [True] * len(windows), geo))
    return calls


def _span_call(streams, r, j, others, geo, rng):
    """Record j of run r is longer than two chunks: its window cut at every chunk edge inside the record (the
    window's chunks and the record's own), one byte before and after each, and around the record's ends;
    windows of the runs `others` cut near the same place in the key order couple the bound."""
    chunk = geo["f1_chunk"]
    w, recs = _window(streams[r], FIRST[r % 3])
    jw = j - FIRST[r % 3]
    s, e, _ = recs[jw]
    assert e - s > 2 * chunk
    edges = [c for c in range(0, len(w), chunk) if s < c < e] + [s + chunk, s + 2 * chunk]
    cuts = sorted(set(edges + [c + d for c in edges for d in (-1, 1)] + record_cuts(w, recs, jw)))
    cut_windows = [(w, c) for c in cuts]
    for o in others:
        cut_windows += _around(streams, o, jw / len(recs), rng, n=(64 - len(cuts)) // len(others))
    return SplitCall("long-records-span", TEXT, [w for w, _ in cut_windows], [a for _, a in cut_windows],
                     [False] * len(cut_windows), geo)


@functools.lru_cache(maxsize=None)
def _split_calls(geo_items):
    geo = dict(geo_items)
    rng = random.Random("rounds-cases/split")
    calls = []
    lr = plan_case("long-records", geo).streams
    calls += _calls_of("long-records", TEXT, lr, rng, (0.3, 0.5, 0.98), geo, short=True)
    calls.append(_span_call(lr, 3, 200, (2, 4), geo, rng))
    calls += _calls_of("shared-prefix", TEXT, plan_case("shared-prefix", geo).streams, rng, (0.04, 0.6), geo)
    calls += _calls_of("eof-at-chunk-edge", TEXT, plan_case("eof-at-chunk-edge", geo).streams, rng, (0.5, 0.9, 0.999),
                       geo, short=True)
    calls += _calls_of("hdr-straddle", TEXT, plan_case("reused-hdr-straddle", geo).streams, rng, (0.34, 0.67), geo)
    calls += _calls_of("entry-edge", TEXT, plan_case("reused-entry-edge", geo).streams, rng, (0.3,), geo)
    calls += _calls_of("len-edges-text", TEXT, plan_case("reused-len-edges-text", geo).streams, rng, (0.9,), geo,
                       runs=[0, 4])
    for n, qs in (("int", (0.2, 0.7)), ("vlong", (0.5,)), ("float", (0.5,))):
        c = plan_case("numeric-" + n, geo)
        calls += _calls_of("numeric-" + n, c.cls, c.streams, rng, qs, geo, short=n == "int")
    assert len({c.name for c in calls}) == len(calls) and all(c.name.startswith(SPLIT_FAMILIES) for c in calls)
    return tuple(calls)


def split_calls(geo):
    return _split_calls(tuple(sorted(geo.items())))


