"""The generic-merge cases of tests/generic_cases.py on the host: the pure-Python oracle against the CPU heap
merge, the module's IFile codec against the package's, and self-checks that every case still lies on the
kernel boundary it was built for (the boundaries come from native.gpu_generic_geometry())."""
import pytest

from tests import generic_cases as gc
from uda_amd import ops
from uda_amd.utils.ifile import decode_stream, encode_stream, vint_decode, vint_encode


@pytest.fixture(scope="module")
def geo(native):
    return native.gpu_generic_geometry()


def _chunk_crossers(buf, geo):
    """(record start, record size) of every record that begins before a chunk end and ends after it."""
    starts, end = gc.walk(buf)
    chunk = geo["f1_chunk"]
    return [(s, e - s) for s, e in zip(starts, starts[1:] + [end]) if s // chunk != (e - 1) // chunk]


def test_geometry_binding(geo):
    assert set(geo) == {"f1_chunk", "f1_halo", "f1_entries", "f1_super_chunks", "f1_chase", "gk_cap", "gk_max_runs",
                        "generic_tile", "staged_key_bytes", "len_cap"}
    assert all(isinstance(v, int) and v > 0 for v in geo.values())
    assert geo["f1_entries"] < geo["f1_chunk"] and geo["f1_halo"] >= 18  # two 9-byte VInts fit the halo


def test_vlong_codec_known_vectors(native):
    """Hadoop's encoding, byte for byte, at every length step."""
    known = {0: "00", 127: "7f", -112: "90", 128: "8f80", 255: "8fff", 256: "8e0100", -113: "8770", -1: "ff",
             -129: "8780", -257: "860100", 65535: "8effff", 65536: "8d010000", 1 << 31: "8c80000000",
             (1 << 63) - 1: "887fffffffffffffff", -(1 << 63): "807fffffffffffffff"}
    for v, hx in known.items():
        assert gc.write_vlong(v).hex() == hx, v
        assert gc.read_vlong(bytes.fromhex(hx), 0) == (v, len(hx) // 2)
    for k in range(64):
        for v in ((1 << k) - 1, 1 << k, -(1 << k), -(1 << k) - 1):
            if -(1 << 63) <= v < 1 << 63:
                e = gc.write_vlong(v)
                assert e == vint_encode(v) == bytes(native.vint_encode(v))
                assert gc.read_vlong(e, 0) == vint_decode(e) == (v, len(e))
    with pytest.raises(gc.CorruptStream):
        gc.read_vlong(b"\x8e\x01", 0)


def test_content_offsets():
    long_text = gc.text(b"x" * 128 + b"tail")
    assert long_text[:2] == b"\x8f\x84" and gc.content(gc.TEXT, long_text) == b"x" * 128 + b"tail"
    assert gc.content(gc.TEXT, gc.text(b"x" * 70000))[:3] == b"xxx" and gc.text(b"x" * 70000)[:4] == b"\x8d\x01\x11\x70"
    assert gc.content(gc.TEXT, gc.text(b"")) == b"" and gc.content(gc.BYTES, gc.bytes_writable(b"ab")) == b"ab"
    assert gc.content(gc.LONG, b"\xff" * 8) == b"\xff" * 8


@pytest.mark.parametrize("name", gc.NAMES)
def test_oracle_equals_cpu_merge(geo, name):
    c = gc.case(name, geo)
    body, _ = ops.merge_runs(list(c.streams), c.key_class, "cpu")
    assert body == c.expected
    assert len(gc.walk(c.expected, require_eof=False)[0]) == c.records


@pytest.mark.parametrize("name", gc.NAMES)
def test_codec_agrees_with_the_package(geo, name):
    c = gc.case(name, geo)
    for run, s in zip(c.runs, c.streams):
        assert s == encode_stream(run)
        assert gc.parse(s) == decode_stream(s) == list(run)
        starts, end = gc.walk(s)
        assert len(starts) == len(run) and end == len(s) - 2


@pytest.mark.parametrize("name,op", [("big-groups-int-one", "sum.int"), ("big-groups-int-three", "sum.int"),
                                     ("big-groups-text-one", "sum.vint"), ("big-groups-text-three", "sum.vint")])
def test_folded_oracle_equals_cpu_combine(geo, name, op):
    c = gc.case(name, geo)
    body, _ = ops.merge_runs(list(c.streams), c.key_class, "cpu", combine=op)
    want = gc.fold(c.merged, c.key_class, op)
    assert body == gc.stream(want, eof=False)
    assert len(want) == (1 if name.endswith("one") else 3)


def test_gather_lengths_cpu_with_a_buffer_of_one_record(geo):
    c = gc.case("gather-lengths-raw", geo)
    body, cuts = ops.merge_runs(list(c.streams), c.key_class, "cpu", kv_buf=c.longest + 2)
    assert body == c.expected and max(b - a for a, b in zip(cuts, cuts[1:])) == c.longest


# ------------------------------------------------------------------------------------------------ geometry
@pytest.mark.parametrize("name", ["hdr-straddle", "hdr-straddle-keys"])
def test_hdr_straddle_geometry(geo, name):
    c = gc.case(name, geo)
    chunk = geo["f1_chunk"]
    assert len(c.streams) == len(gc.STRADDLE_OFFSETS)
    for off, s in zip(gc.STRADDLE_OFFSETS, c.streams):
        starts, _ = gc.walk(s)
        assert len(s) > 2.5 * chunk
        for at in (chunk + off, 2 * chunk + off):
            assert at in starts
            _, a = gc.read_vlong(s, at)
            _, b = gc.read_vlong(s, at + a)
            assert a + b == 3  # a multi-byte header; offsets -2 and -1 cut it at the chunk end
        sizes = [e - b for b, e in zip(starts, starts[1:])]
        assert max(sizes) < geo["f1_entries"]
        for st in starts:  # every header is multi-byte: no record takes the single-byte fast path
            assert s[st] >= 0x80 or s[st + 1] >= 0x80
    if name == "hdr-straddle-keys":
        assert all(128 <= len(gc.content(gc.TEXT, k)) <= 150 and k[0] == 0x8f for r in c.runs for k, _ in r)
    assert c.expect["f1_serial_runs"] == 0


def test_entry_edge_geometry(geo):
    c = gc.case("entry-edge", geo)
    chunk, entries = geo["f1_chunk"], geo["f1_entries"]
    assert c.meta["straddlers"] == [entries - 1, entries, entries + 1]
    serial = 0
    for size, s in zip(c.meta["straddlers"], c.streams):
        cross = _chunk_crossers(s, geo)
        assert (chunk - 1, size) in cross
        assert [sz for _, sz in cross if sz > 100] == [size]  # the only long record of the run
        serial += gc.f1_goes_serial(s, geo)
        assert gc.f1_goes_serial(s, geo) == (size > entries)
    assert chunk in gc.walk(c.streams[3])[0] and 2 * chunk in gc.walk(c.streams[4])[0]
    assert serial == 1 and c.expect["f1_serial_runs"] == 1


def test_run_lengths_geometry(geo):
    c = gc.case("run-lengths", geo)
    chunk = geo["f1_chunk"]
    span = chunk * geo["f1_super_chunks"]
    assert [len(s) for s in c.streams] == [chunk - 1, chunk, chunk + 1, 2 * chunk, 2 * chunk + 1, span - 1, span,
                                           span + 1, 2 * span + 1]
    for s, run in zip(c.streams, c.runs):
        assert all(20 <= len(gc.record(k, v)) <= 60 for k, v in run)
    assert c.expect["f1_serial_runs"] == 0


@pytest.mark.parametrize("name,width", [("raw-wide-long", 8), ("raw-wide-int", 4)])
def test_raw_wide_geometry(geo, name, width):
    c = gc.case(name, geo)
    assert len(c.streams) == 3
    assert min(len(s) for s in c.streams) >= 70 * geo["f1_chunk"] > geo["f1_super_chunks"] * geo["f1_chunk"]
    for run in c.runs:
        keys = [k for k, _ in run]
        assert {len(k) for k in keys} == {width} and {len(v) for _, v in run} == {0, 1, 8}
        assert keys[0][0] < 0x80 <= keys[-1][0]  # negative numbers sort after the positive ones
        assert len(set(keys)) < len(keys)
    assert c.expect["f1_serial_runs"] == 0


@pytest.mark.parametrize("name", ["len-edges-text", "len-edges-bytes"])
def test_len_edges_geometry(geo, name):
    c = gc.case(name, geo)
    cap = geo["len_cap"]
    lens = {len(gc.content(c.key_class, k)) for r in c.runs for k, _ in r}
    assert lens >= {0, 1, 7, 8, 9, 15, 16, 17, 24, 25, 32, 33, 126, 127, 128, 129, 255, 256, 300, cap - 1, cap, cap + 1,
                    70000}
    contents = {gc.content(c.key_class, k) for r in c.runs for k, _ in r}
    assert {bytes([x]) for x in b"".join(contents)} == {b"\x00", b"\x61", b"\xff"}
    for n in gc.len_edge_lengths(geo):  # a key and the same key with real zero bytes behind it
        assert any(len(x) == n and any(x + bytes(z) in contents for z in (1, 2, 3)) for x in contents), n
    merged = [gc.content(c.key_class, k) for k, _ in c.merged]
    # two neighbours in the output that differ only in length, both beyond the saturated length field
    assert any(len(a) >= cap and len(b) > len(a) and b.startswith(a) for a, b in zip(merged, merged[1:]))
    holds_long = [any(len(gc.record(k, v)) > geo["f1_entries"] for k, v in r) for r in c.runs]
    assert holds_long == [True, True, True, True, False] and len(c.runs) == 5
    assert [gc.f1_goes_serial(s, geo) for s in c.streams] == holds_long
    assert c.expect["f1_serial_runs"] == 4


@pytest.mark.parametrize("name", [n for n in gc.NAMES if n.startswith("tie-depth")])
def test_tie_depth_geometry(geo, name):
    c = gc.case(name, geo)
    depth = c.meta["depth"]
    staged = geo["staged_key_bytes"]
    assert 2800 <= c.records <= 3200 and len(c.runs) == 4
    assert depth - (len(gc.SHARED_PREFIX) if name.endswith("prefixed") else 0) - 1 in gc.TIE_DEPTHS
    assert {staged - 2, staged - 1, staged, staged + 1, staged + 7, staged + 8, staged + 9} == set(gc.TIE_DEPTHS)
    merged = [gc.content(gc.TEXT, k) for k, _ in c.merged]

    def first_diff(a, b):
        n = next((i for i in range(min(len(a), len(b))) if a[i] != b[i]), min(len(a), len(b)))
        return None if a == b else n

    diffs = {first_diff(a, b) for a, b in zip(merged, merged[1:])}
    # neighbours differ at the tail's first byte (content byte 1 + d behind the prefix) and just behind it;
    # where the first byte c changes they differ right behind the shared prefix, and some are equal
    assert {depth, depth + 1, depth + 2, None} <= diffs <= {depth - 1 - d_of(name), depth, depth + 1, depth + 2, None}


def d_of(name):
    return int(name.split("-")[2])


@pytest.mark.parametrize("name", [n for n in gc.NAMES if n.startswith("big-groups")])
def test_big_groups_geometry(geo, name):
    c = gc.case(name, geo)
    groups = {}
    for k, _ in c.merged:
        groups[k] = groups.get(k, 0) + 1
    assert min(groups.values()) > max(geo["gk_cap"], geo["generic_tile"])
    assert sorted(groups.values()) == ([4500] if name.endswith("one") else [1100] * 3)
    # neighbours in the output carry different values, so a swapped pair of equal keys changes the bytes
    vals = [v for _, v in c.merged]
    assert sum(a == b for a, b in zip(vals, vals[1:])) < len(vals) // 50


@pytest.mark.parametrize("K", [1, 127, 128, 129])
def test_fan_in_geometry(geo, K):
    c = gc.case(f"fan-in-{K}", geo)
    sizes = sorted(len(r) for r in c.runs)
    assert len(c.runs) == K and {127, 128, 129} == {geo["gk_max_runs"] - 1, geo["gk_max_runs"], geo["gk_max_runs"] + 1}
    assert sizes[-1] == 600 and (K == 1 or (sizes[-2] <= 12 and 3 * sizes.count(0) >= K))
    assert c.expect.get("passes") == {1: 0, 127: 1, 128: 1, 129: None}[K]


@pytest.mark.parametrize("name,least", [("gather-lengths-raw", 2), ("gather-lengths-text", 3)])
def test_gather_lengths_geometry(geo, name, least):
    c = gc.case(name, geo)
    sizes = {len(gc.record(k, v)) for r in c.runs for k, v in r}
    assert sizes == set(range(least, 49)) | {63, 64, 65, 127, 128, 129, 255, 256, 257, 4095, 4096, 4097, 70000}
    assert len(c.runs) == 3 and c.longest == 70000


# ------------------------------------------------------------------------------------------------ corrupt runs
@pytest.mark.parametrize("name", list(gc.CORRUPT))
def test_corrupt_runs_on_the_cpu(geo, name):
    """What the device must do with each broken run is what the CPU merge does: fail, or (a run that ends on a
    record boundary without EOF marker) merge it."""
    good, streams, raises = gc.corrupt_case(name, geo)
    assert len(streams) == 3 and len(streams[1]) > 2.5 * geo["f1_chunk"]
    if raises:
        with pytest.raises(gc.CorruptStream):
            gc.walk(streams[1])
        with pytest.raises(Exception):
            ops.merge_runs(list(streams), gc.TEXT, "cpu")
    else:
        body, _ = ops.merge_runs(list(streams), gc.TEXT, "cpu")
        assert body == b"".join(gc.oracle_merge(good, gc.TEXT))
