"""Shared by the tests of the generic merge (F1 record index, F2 normalize, F3 K-way cells and pairwise tree,
F4 scan / gather / cuts): a pure-Python oracle of the merge, and inputs placed on the kernels' boundaries.

Nothing here touches the native module or the package's own IFile codec, so a wrong VInt size or content
offset in the shared headers cannot be wrong on both sides of a comparison. The VInt codec follows Hadoop's
WritableUtils.writeVLong / readVLong; the key order is the reference's CompareFunc.cc:29-113 (Hadoop's raw
comparators): content bytes as unsigned bytes, the shorter content first on a common prefix, and equal keys
in run order, then position. Python's ordering of `bytes` is exactly that, so the oracle is one sort.

The kernels' constants come in as `geo`, the dict of native.gpu_generic_geometry(): the cases compute their
offsets from it and move when the kernels do. A case is built once per (name, geo) and never changed."""
import functools
import random

TEXT = "org.apache.hadoop.io.Text"
INT = "org.apache.hadoop.io.IntWritable"
LONG = "org.apache.hadoop.io.LongWritable"
BYTES = "org.apache.hadoop.io.BytesWritable"
EOF = b"\xff\xff"


class CorruptStream(ValueError):
    pass


# ------------------------------------------------------------------------------------------------ format
def write_vlong(v):
    """WritableUtils.writeVLong: one byte for -112..127, else a length byte (-113..-120 positive, -121..-128
    negative, the value then stored as its one's complement) and 1..8 big-endian bytes."""
    if -112 <= v <= 127:
        return bytes([v & 0xFF])
    first = -112
    if v < 0:
        v = ~v
        first = -120
    n = (v.bit_length() + 7) // 8
    return bytes([(first - n) & 0xFF]) + v.to_bytes(n, "big")


def read_vlong(buf, pos):
    """(value, bytes used) of the VLong at buf[pos]; CorruptStream if the buffer ends inside it."""
    if pos >= len(buf):
        raise CorruptStream("stream ends where a VInt begins")
    first = buf[pos] - 256 if buf[pos] > 127 else buf[pos]
    if first >= -112:
        return first, 1
    n = -(first + 120) if first < -120 else -(first + 112)
    if pos + 1 + n > len(buf):
        raise CorruptStream("stream ends inside a VInt")
    v = int.from_bytes(buf[pos + 1:pos + 1 + n], "big")
    return (~v if first < -120 else v), 1 + n


def record(key, val):
    return write_vlong(len(key)) + write_vlong(len(val)) + key + val


def stream(records, eof=True):
    return b"".join(record(k, v) for k, v in records) + (EOF if eof else b"")


def walk(buf, require_eof=True):
    """Offsets of the records of a stream and the offset where they end (the EOF marker's, or the stream's end
    when require_eof is False and it ends on a record boundary): ([starts], end). CorruptStream otherwise."""
    starts, pos = [], 0
    while True:
        if pos == len(buf) and not require_eof:
            return starts, pos
        kl, a = read_vlong(buf, pos)
        vl, b = read_vlong(buf, pos + a)
        if kl == -1 and vl == -1:
            return starts, pos
        if kl < 0 or vl < 0:
            raise CorruptStream("negative length")
        if pos + a + b + kl + vl > len(buf):
            raise CorruptStream("record longer than the rest of the stream")
        starts.append(pos)
        pos += a + b + kl + vl


def parse(buf, require_eof=True):
    """[(key, value)] of a stream."""
    starts, end = walk(buf, require_eof)
    out = []
    for s, e in zip(starts, starts[1:] + [end]):
        kl, a = read_vlong(buf, s)
        _, b = read_vlong(buf, s + a)
        out.append((buf[s + a + b:s + a + b + kl], buf[s + a + b + kl:e]))
    return out


def text(s):
    return write_vlong(len(s)) + s


def bytes_writable(s):
    return len(s).to_bytes(4, "big") + s


def content(key_class, key):
    """The bytes the comparator of `key_class` compares."""
    if key_class == TEXT:
        return key[read_vlong(key, 0)[1]:] if key else key
    if key_class == BYTES:
        return key[4:]
    return key


def make_key(key_class, c):
    return text(c) if key_class == TEXT else bytes_writable(c) if key_class == BYTES else c


def merged_records(runs, key_class):
    """All (key, value) of the runs (lists of records) in merged order: content, then run, then position."""
    tagged = [(content(key_class, k), r, i, k, v) for r, run in enumerate(runs) for i, (k, v) in enumerate(run)]
    tagged.sort(key=lambda t: t[:3])
    return [(k, v) for _, _, _, k, v in tagged]


def oracle_merge(runs, key_class):
    """The merged stream's records as record bytes."""
    return [record(k, v) for k, v in merged_records(runs, key_class)]


def fold(records, key_class, op):
    """The merged records combined: the first record of each group of equal contents, its value the sum of the
    group's values. sum.int: 4 bytes big-endian, wrapping; sum.vint: one VInt each, wrapped to 32 bits and
    written canonically."""
    out = []
    for k, v in records:
        x = int.from_bytes(v, "big", signed=True) if op == "sum.int" else read_vlong(v, 0)[0]
        if out and content(key_class, out[-1][0]) == content(key_class, k):
            out[-1][1] += x
        else:
            out.append([k, x])
    res = []
    for k, x in out:
        x &= 0xFFFFFFFF
        x -= (x >> 31) << 32
        res.append((k, x.to_bytes(4, "big", signed=True) if op == "sum.int" else write_vlong(x)))
    return res


def f1_goes_serial(buf, geo):
    """Whether the parallel F1 index hands this run to the serial walk: the chain of record starts (and the EOF
    marker's) enters a chunk, or a superchunk, at an offset the entry table does not hold. That is a record
    longer than f1_entries bytes that crosses a chunk end by at least that much."""
    chunk, entries = geo["f1_chunk"], geo["f1_entries"]
    span = chunk * geo["f1_super_chunks"]
    starts, end = walk(buf, require_eof=False)
    prev = 0
    for q in starts[1:] + [end]:
        if q >= len(buf):
            break
        if q // span != prev // span:
            if q % span >= entries:
                return True
        elif q // chunk != prev // chunk and q % chunk >= entries:
            return True
        prev = q
    return False


# ------------------------------------------------------------------------------------------------ cases
class Case:
    def __init__(self, name, key_class, runs, geo, passes=None, **meta):
        self.name, self.key_class, self.meta = name, key_class, meta
        self.runs = tuple(tuple(r) for r in runs)
        for r in self.runs:  # a run is sorted, equal keys in the order given
            cs = [content(key_class, k) for k, _ in r]
            assert cs == sorted(cs), name
        self.streams = tuple(stream(r) for r in self.runs)
        self.records = sum(len(r) for r in self.runs)
        self.longest = max((len(record(k, v)) for r in self.runs for k, v in r), default=0)
        self.expect = {"f1_serial_runs": sum(f1_goes_serial(s, geo) for s in self.streams)}
        if passes is not None:
            self.expect["passes"] = passes

    @functools.cached_property
    def merged(self):
        return merged_records(self.runs, self.key_class)

    @functools.cached_property
    def expected(self):
        return b"".join(oracle_merge(self.runs, self.key_class))


def _by_content(key_class, recs):
    return sorted(recs, key=lambda kv: content(key_class, kv[0]))


def _size(kv):
    return len(record(*kv))


def _land(recs, j, target, vmin, vmax, rng, first=0, upto=None):
    """Resize the values of recs[first:j] (or of recs[first:upto]) within [vmin, vmax] bytes (one VInt size
    class, so a record changes by exactly the bytes its value does) until record j starts at byte `target`."""
    assert len(write_vlong(vmin)) == len(write_vlong(vmax))
    delta = target - sum(_size(kv) for kv in recs[:j])
    for i in range(first, j if upto is None else upto):
        k, v = recs[i]
        step = max(vmin - len(v), min(vmax - len(v), delta))
        recs[i] = (k, v[:len(v) + step] if step < 0 else v + rng.randbytes(step))
        delta -= step
    assert delta == 0, (j, target, delta)


def _start_near(recs, target, first=0):
    """The record (after `first`) that starts nearest to `target` as the sizes are now."""
    pos, best = 0, None
    for i, kv in enumerate(recs):
        if i > first and (best is None or abs(pos - target) < best[0]):
            best = (abs(pos - target), i)
        pos += _size(kv)
    return best[1]


STRADDLE_OFFSETS = (-4, -3, -2, -1, 0, 1)  # record starts relative to the chunk end: the header is cut at each byte


def _hdr_straddle(geo, rng, long_keys):
    """One run per offset: a record with a multi-byte header starts at chunk + offset, and another one at
    2 * chunk + offset. Short keys: VInt(k) and a 2-byte VInt(v). Long keys: a 2-byte VInt(k), whose key opens
    with the 2-byte VInt of its Text length, and VInt(v)."""
    chunk = geo["f1_chunk"]
    runs = []
    for off in STRADDLE_OFFSETS:
        if long_keys:
            vmin, vmax = 0, 60
            keys = [bytes(rng.choice(b"abc") for _ in range(rng.randint(128, 150))) for _ in range(3 * chunk // 170)]
        else:
            vmin, vmax = 128, 180
            keys = [b"%0*d" % (rng.randint(2, 9), rng.randrange(100)) for _ in range(3 * chunk // 160)]
        recs = _by_content(TEXT, [(text(k), rng.randbytes(rng.randint(vmin, vmax))) for k in keys])
        j = _start_near(recs, chunk + off)
        _land(recs, j, chunk + off, vmin, vmax, rng)
        j2 = _start_near(recs, 2 * chunk + off, first=j)
        _land(recs, j2, 2 * chunk + off, vmin, vmax, rng, first=j)
        runs.append(recs)
    return runs


def _entry_edge(geo, rng):
    """Runs of short records with one record of f1_entries - 1, f1_entries and f1_entries + 1 bytes starting one
    byte before the first chunk end (it leaves the chunk at entries - 2, - 1 and at `entries`, which the table
    does not hold), then a run with a record ending exactly on the first chunk end and one on the second."""
    chunk, entries = geo["f1_chunk"], geo["f1_entries"]
    runs, sizes = [], []

    def small(n):
        return [(text(b"k%05d" % rng.randrange(10 ** 5)), rng.randbytes(rng.randint(20, 60))) for _ in range(n)]

    for size in (entries - 1, entries, entries + 1):
        recs = _by_content(TEXT, small(3 * chunk // 50))
        j = _start_near(recs, chunk - 1)
        big_key = recs[j][0]  # an equal key keeps the run sorted
        val = size - len(record(big_key, b"")) - 1  # the value's VInt takes 2 bytes, not 1
        big = (big_key, rng.randbytes(val))
        assert _size(big) == size
        recs.insert(j, big)
        _land(recs, j, chunk - 1, 20, 60, rng)
        runs.append(recs)
        sizes.append(size)
    for ends_at in (chunk, 2 * chunk):
        recs = _by_content(TEXT, small(3 * chunk // 50))
        _land(recs, _start_near(recs, ends_at), ends_at, 20, 60, rng)
        runs.append(recs)
    return runs, sizes


def run_length_targets(geo):
    chunk = geo["f1_chunk"]
    span = chunk * geo["f1_super_chunks"]
    return (chunk - 1, chunk, chunk + 1, 2 * chunk, 2 * chunk + 1, span - 1, span, span + 1, 2 * span + 1)


def _run_of_length(total, rng):
    """Text records of 20..60 bytes with one-byte headers whose stream, EOF marker included, has `total` bytes."""
    left, sizes = total - len(EOF), []
    while left > 80:
        sizes.append(rng.randint(20, 60))
        left -= sizes[-1]
    sizes += [left] if left <= 60 else [left // 2, left - left // 2]
    recs = []
    for s in sizes:
        c = rng.randint(1, 12)
        recs.append((text(b"%0*d" % (c, rng.randrange(10 ** min(c, 6)))), rng.randbytes(s - 3 - c)))
        assert _size(recs[-1]) == s
    return _by_content(TEXT, recs)


def _raw_wide(geo, rng, width):
    """Fixed-width raw keys (no key framing for the parallel index to check), 3 runs of at least 70 chunks:
    signed numbers as big-endian bytes, so the negatives sort after the positives; half of them from a small
    range, so keys repeat within and across runs. Values of 0, 1 or 8 bytes."""
    need = (geo["f1_super_chunks"] + 6) * geo["f1_chunk"]
    bits = 8 * width
    runs = []
    for _ in range(3):
        recs, size = [], 0
        while size < need:
            x = rng.randint(-50, 50) if rng.random() < 0.5 else rng.randint(-(1 << (bits - 1)), (1 << (bits - 1)) - 1)
            recs.append((x.to_bytes(width, "big", signed=True), rng.randbytes(rng.choice((0, 1, 8)))))
            size += 2 + width + len(recs[-1][1])
        runs.append(_by_content(INT, recs))
    return runs


LEN_EDGES = (0, 1, 7, 8, 9, 15, 16, 17, 24, 25, 32, 33, 126, 127, 128, 129, 255, 256, 300)


def len_edge_lengths(geo):
    cap = geo["len_cap"]
    return LEN_EDGES + (cap - 1, cap, cap + 1, 70000)


def _len_edges(geo, rng, key_class):
    """Contents of every edge length over {00, 61, ff}: prefixes of one body (so two keys tie to the end of
    the shorter one and their lengths decide, beyond the saturated length field too), each also with 1..3
    zero bytes appended (real zeros against the zero padding of the packed words), and independent contents
    of the shorter lengths. 5 runs; the keys above f1_entries bytes go to runs 0..3 only, each placed so that
    it leaves its chunk past the entry table."""
    chunk, entries = geo["f1_chunk"], geo["f1_entries"]
    lengths = len_edge_lengths(geo)
    body = bytes(rng.choice(b"\x00\x61\xff") for _ in range(max(lengths)))
    small, giant = [], []
    for n in lengths:
        if n > 1000:
            giant += [body[:n], body[:n] + bytes(rng.randint(1, 3)), body[:n - 1] + b"\x61"]
        else:
            small += [body[:n]] + [body[:n] + bytes(z) for z in (1, 2, 3)]
            small += [bytes(rng.choice(b"\x00\x61\xff") for _ in range(n)) for _ in range(2)]
    # contents of 9..16 bytes that tie on their first 8 and whose shorter ones sort last: only the bytes
    # behind the packed prefix order them, neither the length nor the run does
    small += [body[:8] + t for t in (b"\xff", b"\x61\x61", b"\x61" * 8, b"\x00" + b"\xff" * 7, b"\xff\x00",
                                     b"\x61\xff\xff")]
    runs = [[] for _ in range(5)]
    for i, c in enumerate(small):
        # short keys: two runs and run 4; a record the entry table cannot hold: two of runs 0..3
        to = {i % 5, (3 * i + 1) % 5, 4} if len(c) + 20 <= entries else {i % 4, (3 * i + 1) % 4}
        for r in to:
            runs[r].append((make_key(key_class, c), b"%d.%d" % (r, i)))
    for i, c in enumerate(giant):
        runs[i % 4].append((make_key(key_class, c), b"%d.%d" % (i % 4, i)))
    out = []
    for r, recs in enumerate(runs):
        recs = _by_content(key_class, recs)
        # filler records in front (the empty content sorts first) that the landing below can resize
        recs = [(make_key(key_class, b""), rng.randbytes(30)) for _ in range(50)] + recs
        if r < 4:
            # move the first long record's end to the middle of a chunk: its start moves by 0..chunk - 1
            j = next(i for i, kv in enumerate(recs) if _size(kv) > 1000)
            start = sum(_size(kv) for kv in recs[:j])
            shift = (chunk // 2 - (start + _size(recs[j]))) % chunk
            _land(recs, j, start + shift, 30, 127, rng, upto=50)
        out.append(recs)
    assert entries < chunk // 2
    return out


TIE_DEPTHS = (22, 23, 24, 25, 31, 32, 33)


def _tie_depth(geo, rng, d, prefix):
    """Contents prefix + c + S + tail: c one of three bytes (unevenly often, so cells and tiles span two of
    them and their common prefix ends at c), S a constant of d bytes, tail 0..3 bytes over {00, 61, ff}. Two
    keys with the same c first differ at content byte len(prefix) + 1 + d, if at all."""
    S = bytes(rng.choice(b"\x00\x61\xff") for _ in range(d))
    tails = [b""] + [bytes(t) for n in (1, 2, 3) for t in _tuples(b"\x00\x61\xff", n)]
    runs = []
    for r in range(4):
        recs = []
        for i in range(750):
            c = rng.choices(b"\x20\x61\xf0", weights=(5, 3, 2))[0]
            recs.append((text(prefix + bytes([c]) + S + rng.choice(tails)), b"%d.%d" % (r, i)))
        runs.append(_by_content(TEXT, recs))
    return runs


def _tuples(alphabet, n):
    if n == 0:
        return [()]
    return [(a,) + t for a in alphabet for t in _tuples(alphabet, n - 1)]


def _big_groups(key_class, shape):
    """3 runs of 1500 records of one key ("one"), or 3 keys of 1100 records each over 3 runs ("three"): groups
    longer than a K-way cell and a pairwise tile. IntWritable values are 4 bytes (run * 10000 + position),
    Text values one-byte VInts, so the combiner's sums apply to them."""
    def key(g):
        return text(b"group-key-%d" % g) if key_class == TEXT else (g * 0x01010101 - 5).to_bytes(4, "big", signed=True)

    def val(r, i):
        return bytes([(41 * r + 3 * i) % 128]) if key_class == TEXT else (r * 10000 + i).to_bytes(4, "big")

    if shape == "one":
        return [[(key(1), val(r, i)) for i in range(1500)] for r in range(3)]
    counts = [(367, 366, 367), (366, 367, 367), (367, 367, 366)]  # 1100 of each key
    order = sorted(range(3), key=lambda g: content(key_class, key(g)))
    runs = [[(key(g), None) for g in order for _ in range(counts[r][g])] for r in range(3)]
    return [[(k, val(r, i)) for i, (k, _) in enumerate(run)] for r, run in enumerate(runs)]


def _fan_in(rng, K):
    """K runs of 0..12 records, more than a third of them empty, and one run 50 times longer."""
    runs = []
    for r in range(K):
        n = 600 if r == K // 2 else 0 if r % 5 in (1, 3) else rng.randint(0, 12)
        runs.append(_by_content(TEXT, [(text(b"w%04d" % rng.randrange(3000)), b"%d.%d" % (r, i)) for i in range(n)]))
    return runs


GATHER_LENGTHS = tuple(range(2, 49)) + (63, 64, 65, 127, 128, 129, 255, 256, 257, 4095, 4096, 4097, 70000)


def _record_of_length(n, key_class, rng):
    """A record of exactly n bytes, header included, its key as short as the class allows plus 0..6 bytes."""
    for c in sorted(range(0, 7), key=lambda _: rng.random()):
        k = make_key(key_class, rng.randbytes(c))
        for hv in (1, 2, 3, 4):  # bytes of the value's VInt
            v = n - len(write_vlong(len(k))) - len(k) - hv
            if v >= 0 and len(write_vlong(v)) == hv:
                return (k, rng.randbytes(v))
    raise AssertionError(n)


def _gather_lengths(rng, key_class):
    lengths = [n for n in GATHER_LENGTHS if n >= (3 if key_class == TEXT else 2)]
    recs = [_record_of_length(n, key_class, rng) for n in lengths for _ in range(1 if n > 1000 else 3)]
    rng.shuffle(recs)
    return [_by_content(key_class, recs[r::3]) for r in range(3)]


NAMES = (["hdr-straddle", "hdr-straddle-keys", "entry-edge", "run-lengths", "raw-wide-long", "raw-wide-int",
          "len-edges-text", "len-edges-bytes"] +
         [f"tie-depth-{d}" for d in TIE_DEPTHS] + [f"tie-depth-{d}-prefixed" for d in TIE_DEPTHS] +
         ["big-groups-text-one", "big-groups-text-three", "big-groups-int-one", "big-groups-int-three"] +
         [f"fan-in-{K}" for K in (1, 127, 128, 129)] + ["gather-lengths-raw", "gather-lengths-text"])
SHARED_PREFIX = b"a-prefix-that-all-keys-of-the-case-share"  # 40 bytes


def case(name, geo):
    return _case(name, tuple(sorted(geo.items())))


@functools.lru_cache(maxsize=None)
def _case(name, geo_items):
    geo = dict(geo_items)
    rng = random.Random("generic-cases/" + name)
    if name == "hdr-straddle":
        return Case(name, TEXT, _hdr_straddle(geo, rng, False), geo)
    if name == "hdr-straddle-keys":
        return Case(name, TEXT, _hdr_straddle(geo, rng, True), geo)
    if name == "entry-edge":
        runs, sizes = _entry_edge(geo, rng)
        return Case(name, TEXT, runs, geo, straddlers=sizes)
    if name == "run-lengths":
        targets = run_length_targets(geo)
        return Case(name, TEXT, [_run_of_length(t, rng) for t in targets], geo, lengths=targets)
    if name.startswith("raw-wide"):
        long_keys = name.endswith("long")
        return Case(name, LONG if long_keys else INT, _raw_wide(geo, rng, 8 if long_keys else 4), geo)
    if name.startswith("len-edges"):
        kc = TEXT if name.endswith("text") else BYTES
        return Case(name, kc, _len_edges(geo, rng, kc), geo)
    if name.startswith("tie-depth"):
        d = int(name.split("-")[2])
        prefix = SHARED_PREFIX if name.endswith("prefixed") else b""
        return Case(name, TEXT, _tie_depth(geo, rng, d, prefix), geo, depth=len(prefix) + 1 + d)
    if name.startswith("big-groups"):
        _, _, kc, shape = name.split("-")
        return Case(name, TEXT if kc == "text" else INT, _big_groups(TEXT if kc == "text" else INT, shape), geo)
    if name.startswith("fan-in"):
        K = int(name.split("-")[2])
        # one run is not merged at all; up to gk_max_runs the K-way cells take one pass
        passes = 0 if K == 1 else 1 if K <= geo["gk_max_runs"] else None
        return Case(name, TEXT, _fan_in(rng, K), geo, passes=passes)
    if name.startswith("gather-lengths"):
        kc = INT if name.endswith("raw") else TEXT
        return Case(name, kc, _gather_lengths(rng, kc), geo)
    raise KeyError(name)


# ------------------------------------------------------------------------------------------------ corrupt runs
# name -> whether the merge must fail. The broken run is the middle one of three.
CORRUPT = {"body-cut": True, "header-cut-in-vint": True, "header-cut-after-klen": True, "negative-klen": True,
           "overclaim-at-chunk-end": True, "half-eof": True, "no-eof": False}


def corrupt_case(name, geo):
    return _corrupt_case(name, tuple(sorted(geo.items())))


@functools.lru_cache(maxsize=None)
def _corrupt_case(name, geo_items):
    """(the three runs as records, their streams with the middle one broken as `name` says, must fail). The
    middle run is about 3 chunks of Text records with one-byte headers, so the parallel index takes it."""
    geo = dict(geo_items)
    chunk = geo["f1_chunk"]
    rng = random.Random("generic-corrupt/" + name)

    def run(n):
        return _by_content(TEXT, [(text(b"c%05d" % rng.randrange(10 ** 5)), rng.randbytes(rng.randint(20, 60)))
                                  for _ in range(n)])

    good = [run(120), run(3 * chunk // 50), run(90)]
    mid = stream(good[1])
    starts, _ = walk(mid)
    j = len(starts) - 6
    if name == "body-cut":  # ends in the middle of a record
        bad = mid[:(starts[j] + starts[j + 1]) // 2]
    elif name == "header-cut-in-vint":  # ends after the first byte of a 2-byte VInt
        bad = mid[:starts[j]] + b"\x8f"
    elif name == "header-cut-after-klen":  # a whole key length, no value length
        bad = mid[:starts[j]] + b"\x05"
    elif name == "negative-klen":  # 0x85: a negative VInt of 3 more bytes
        bad = b"\x85\x03" + mid
    elif name == "overclaim-at-chunk-end":  # a 5-byte key and a value of 2^31 - 1 bytes, 6 bytes before a chunk end
        recs = list(good[1])
        at = 2 * chunk - 6
        i = _start_near(recs, at)
        _land(recs, i, at, 20, 60, rng)
        good[1] = recs
        bad = stream(recs[:i], eof=False) + b"\x05\x8c\x7f\xff\xff\xff" + stream(recs[i:])
        assert walk(stream(recs[:i], eof=False), require_eof=False)[1] == at
    elif name == "half-eof":
        bad = mid[:-1]
    elif name == "no-eof":  # ends on a record boundary: accepted
        bad = mid[:-2]
    else:
        raise KeyError(name)
    runs = tuple(tuple(r) for r in good)
    return runs, (stream(runs[0]), bad, stream(runs[2])), CORRUPT[name]
