"""The assembled decode cases (tests/decode_cases.py) against the host decoders, and the cases against
themselves: every valid stream decodes to the assembler's bytes through the Python oracle and every host
decoder, every corrupt stream is refused by all of them, and the token records show that each family puts
its tokens where it claims to.
"""
import pytest

from tests import decode_cases as dc

FEEDS = (1, 7, 1 << 20)
FAMILIES = ("token-at-window-edge", "extension-runs", "literal-lengths", "match-shapes", "fence", "chunk-ends",
            "lzo-states", "snappy-chunks", "layout", "prefix-targets")


@pytest.fixture(scope="module")
def geom(native):
    return native.gpu_decode_geometry()


@pytest.fixture(scope="module")
def fam(geom):
    return dc.families(geom)


@pytest.fixture(scope="module")
def bad(geom):
    return dc.corrupt_cases(geom)


def chunk_host(native, codec, chunk, cap):
    return {"lzo": native.lzo1x_decompress, "snappy": native.snappy_decompress, "lz4": native.lz4_decompress}[codec](chunk, cap)


def test_geometry_names_the_kernel_constants(geom):
    assert geom == {"reg_window": 256, "reg_align": 4, "lds_window": 2048, "lds_align": 16, "short_copy": 64,
                    "vec_bytes": 16, "wave_step": 1024, "lane_word": 8, "waves_per_block": 4, "prefix_slot": 128}


def test_families_are_small_and_complete(fam):
    assert sorted(fam) == sorted(FAMILIES)
    for name, cases in fam.items():
        assert len({c.name for c in cases}) == len(cases), name
        for c in cases:
            assert len(c.stream) <= 100_000 and len(c.raw) <= 100_000, c.name
    for name in ("token-at-window-edge", "literal-lengths", "match-shapes", "fence", "chunk-ends", "layout",
                 "prefix-targets"):
        assert all(dc.of_codec(fam[name], codec) for codec in dc.CODECS), name
    assert {c.codec for c in fam["extension-runs"]} == {"lzo", "lz4"}


@pytest.mark.parametrize("family", FAMILIES)
def test_valid_cases_decode_identically_everywhere(native, fam, family):
    for c in fam[family]:
        cid = dc.CODEC_ID[c.codec]
        assert dc.stream_decode(c.codec, c.stream) == (c.raw, len(c.braws)), c.name
        for feed in FEEDS:
            assert native.block_decompress(cid, c.stream, feed) == c.raw, (c.name, feed)
        if c.codec == "lzo":
            assert native.lzo_lane_decode_host(c.stream, len(c.raw)) == c.raw, c.name
        for (raw_len, chunks), want in zip(dc.blocks_of(c.codec, c.stream), c.braws):
            assert raw_len == len(want)
            got = b"".join(chunk_host(native, c.codec, ch, raw_len) for ch in chunks)
            assert got == want, c.name


def test_lzo_marker_alone_is_the_empty_chunk(native):
    assert dc.lzo_decode(dc.LZO_MARKER) == b"" == native.lzo1x_decompress(dc.LZO_MARKER, 0)


def test_snappy_cases_through_an_independent_decoder(fam):
    pa = pytest.importorskip("pyarrow")
    n = 0
    for family in FAMILIES:
        for c in dc.of_codec(fam[family], "snappy"):
            got = b""
            for raw_len, chunks in dc.blocks_of(c.codec, c.stream):
                for ch in chunks:
                    size = len(dc.snappy_decode(ch))
                    got += pa.decompress(ch, decompressed_size=size, codec="snappy", asbytes=True)
            assert got == c.raw, c.name
            n += 1
    assert n > 1000


def test_corrupt_cases_are_refused_by_the_oracle_and_every_host_decoder(native, bad):
    assert len({b.name for b in bad}) == len(bad)
    assert {b.codec for b in bad} == {"lzo", "snappy"}  # LZ4's are in test_gpu_lz4_decode.py and test_lz4_codec.py
    for b in bad:
        assert len(b.stream) < 40_000, b.name
        with pytest.raises(ValueError):
            dc.stream_decode(b.codec, b.stream)
        for feed in FEEDS:
            with pytest.raises((ValueError, RuntimeError)):
                native.block_decompress(dc.CODEC_ID[b.codec], b.stream, feed)
        if b.codec == "lzo":
            with pytest.raises((ValueError, RuntimeError)):
                native.lzo_lane_decode_host(b.stream, 1 << 18)
        if b.chunk is not None:
            with pytest.raises(ValueError):
                dc.chunk_decode(b.codec, b.chunk, b.cap)
            with pytest.raises((ValueError, RuntimeError)):
                chunk_host(native, b.codec, b.chunk, b.cap)


def test_corrupt_cases_cover_every_named_check(bad):
    names = {b.name for b in bad}
    for kind in ("lit_ext", "m1s", "m1r", "m2", "m3", "m3_ext", "m4", "m4_ext", "marker"):
        assert any(n.startswith("lzo-cut-%s-" % kind) for n in names), kind
    for kind in ("lit60", "lit61", "lit62", "lit63", "copy1", "copy2", "copy4"):
        assert any(n.startswith("snappy-cut-%s-" % kind) for n in names), kind
    assert "snappy-cut-copy4-4" in names  # copy-4 with 3 of its 4 offset bytes left
    for kind in ("m1s", "m1r", "m2", "m3", "m4"):
        assert "lzo-%s-one-byte-before-the-start" % kind in names
    for k in (1, 2, 4):
        assert {"snappy-copy%d-offset-0" % k, "snappy-copy%d-one-byte-before-the-start" % k} <= names
    assert {"lzo-literal-into-last-3-bytes", "snappy-literal-past-the-chunk", "lzo-block-2-reaches-into-block-1",
            "snappy-block-2-reaches-into-block-1", "snappy-chunk-2-reaches-into-chunk-1",
            "lzo-m1-after-run-with-100-bytes-out", "lzo-output-longer-than-announced",
            "lzo-output-shorter-than-announced", "snappy-block-longer-than-announced",
            "snappy-block-shorter-than-announced", "lzo-marker-length-4", "lzo-marker-then-a-byte",
            "lzo-marker-missing", "lzo-literal-extension-run-to-the-end", "lzo-m3-extension-run-to-the-end",
            "lzo-m4-extension-run-to-the-end", "snappy-length-of-6-bytes", "snappy-length-larger-than-the-block",
            "snappy-copy4-top-offset-byte"} <= names


# ------------------------------------------------------------------------ the cases hit what they claim
def _token_at(c, x):
    hits = [t for t in c.toks if t.ip == x]
    assert len(hits) == 1, (c.name, x)
    return hits[0]


def test_window_edge_family_covers_every_offset_for_every_token_kind(geom, fam):
    kinds = {"lzo": dc.LZO_EDGE_KINDS, "snappy": dc.SNAPPY_EDGE_KINDS, "lz4": dc.LZ4_EDGE_KINDS}
    seen = {(c.codec,) + c.tag for c in fam["token-at-window-edge"]}
    assert dc.edge_offsets(geom) == [(w, x) for w in (256, 512, 2048) for x in range(w - 7, w + 5)]
    assert seen == {(codec, k, w, x) for codec in dc.CODECS for k in kinds[codec] for w, x in dc.edge_offsets(geom)}
    for c in fam["token-at-window-edge"]:
        kind, w, x = c.tag
        t = _token_at(c, x)
        if c.codec == "lzo":
            base = {"lit_ext": "lit", "m3_ext": "m3", "m4_hi": "m4", "m4_ext": "m4"}.get(kind, kind)
            assert t.kind == base, c.name
            if kind == "lit":
                assert t.size == 1 and t.state == 0
            elif kind == "lit_ext":
                assert t.size == 4 and t.state == 0  # 0, two zero bytes, the final byte
            elif kind in ("m3_ext", "m4_ext"):
                assert t.size == 6  # the token, two zero bytes, the final byte, two offset bytes
            elif kind == "m4":
                assert t.size == 3 and 16385 <= t.dist < 32768
            elif kind == "m4_hi":
                assert t.size == 3 and t.dist >= 32768
            elif kind == "m1s":
                assert t.state in (1, 2, 3) and t.length == 2
            elif kind == "m1r":
                assert t.state == 4 and t.length == 3 and t.dist > 2048
        elif c.codec == "snappy":
            assert t.kind == kind and t.size == {"lit": 1, "lit60": 2, "lit61": 3, "lit62": 4, "lit63": 5, "copy1": 2,
                                                 "copy2": 3, "copy4": 5}[kind], c.name
        else:
            assert t.kind == ("last" if kind == "last" else "seq"), c.name
            if kind != "last":  # token, extension bytes of either side, offset
                assert t.size == 3 + 2 * (kind in ("lit_ext", "both_ext")) + 2 * (kind in ("match_ext", "both_ext"))
        # the register window stepped from multiple to multiple on the way: a token sits on each
        for a in range(geom["reg_window"], w, geom["reg_window"]):
            assert any(k.ip == a or (c.codec == "lz4" and k.ip < a == k.ip + k.size - 2 + k.trail) for k in c.toks), (c.name, a)


def test_extension_runs_end_on_every_offset(geom, fam):
    seen = {(c.codec,) + c.tag for c in fam["extension-runs"] if len(c.tag) == 4}
    want = {(codec, kind, k, w, x) for codec, kinds in (("lzo", ("lit_ext", "m3_ext", "m4_ext")), ("lz4", ("lit_ext", "match_ext")))
            for kind in kinds for k in dc.RUN_BYTES for w, x in dc.edge_offsets(geom)}
    assert seen == want
    chunk = lambda c: next(dc.blocks_of(c.codec, c.stream))[1][0]
    for c in fam["extension-runs"]:
        if len(c.tag) == 4:
            kind, k, w, x = c.tag
            body, fill = chunk(c), b"\x00" if c.codec == "lzo" else b"\xff"
            assert body[x - k:x] == fill * k and body[x:x + 1] != fill, c.name
            if c.codec == "lz4":  # the run is exactly k bytes long (LZO: the token before it is 0x00 / 0x20 / 0x10)
                assert body[x - k - 1:x - k] != fill, c.name
    lens = {c.tag for c in fam["extension-runs"] if len(c.tag) == 2 and c.codec == "lzo"}
    assert lens >= {("lit_len", n) for n in (18, 19, 273, 274)} | {("m3_len", n) for n in (33, 34, 288, 289)}
    for c in fam["extension-runs"]:
        if len(c.tag) == 2 and c.codec == "lzo":
            assert any(t.length == c.tag[1] and t.kind == c.tag[0][:-4] for t in c.toks), c.name


def test_literal_lengths_cover_the_alignments(geom, fam):
    for codec in dc.CODECS:
        seen = {c.tag for c in dc.of_codec(fam["literal-lengths"], codec)}
        assert seen >= {("lit", n, pi, po) for n in dc.LITERAL_LENGTHS for pi in range(geom["reg_align"])
                        for po in (0, 1, geom["vec_bytes"] - 1)}
        if codec != "snappy":
            assert seen >= {("late_lit", s, geom["short_copy"]) for s in range(190, 256)}
    assert set(dc.LITERAL_LENGTHS) == {1, 2, 3, 4, 15, 16, 17, 63, 64, 65, 79, 80, 81, 1023, 1024, 1025, 1039, 1040, 2049}


def test_match_shapes_hold_all_relations_on_both_sides_of_the_short_copy(geom, fam):
    sc = geom["short_copy"]
    for codec in dc.CODECS:
        rel = {(dc.relation(d, n), n <= sc) for _, d, n in (c.tag for c in dc.of_codec(fam["match-shapes"], codec))}
        sides = (True,) if codec == "snappy" else (True, False)  # Snappy's longest copy is 64 bytes
        assert rel == {(r, s) for r in ("off<len", "off==len", "off>len") for s in sides}, codec
        for c in dc.of_codec(fam["match-shapes"], codec):
            _, d, n = c.tag
            assert any(t.dist == d and t.length == n for t in c.toks), c.name
    lzo = {c.tag for c in dc.of_codec(fam["match-shapes"], "lzo")}
    assert {k for k, _, _ in lzo} == {"m1s", "m1r", "m2", "m3", "m4"}
    assert {d for _, d, _ in lzo} == set(dc.MATCH_OFFSETS) and {n for _, _, n in lzo} == set(dc.MATCH_LENGTHS)
    assert {("m1r", 2049, 3), ("m1r", 3072, 3), ("m4", 16385, 3), ("m4", 49151, 1030), ("m3", 16384, 1030)} <= lzo
    assert {d for _, d, _ in (c.tag for c in dc.of_codec(fam["match-shapes"], "lz4"))} == set(dc.MATCH_OFFSETS)
    assert ("copy4", 69999, 40) in {c.tag for c in dc.of_codec(fam["match-shapes"], "snappy")}


def test_lzo_soups_walk_every_allowed_transition(fam):
    soups = fam["lzo-states"]
    assert 50 <= len(soups) <= 70
    toks = [t for c in soups for t in c.toks]
    allowed = {(s, k) for s in range(5) for k in dc.LZO_SOUP_KINDS if dc.lzo_allowed(s, k)}
    assert {(t.state, t.kind) for t in toks if t.kind != "first"} == allowed
    assert {(t.kind, t.trail) for t in toks if t.kind.startswith("m")} == {(k, n) for k in ("m1s", "m1r", "m2", "m3", "m4")
                                                                            for n in range(4)}
    firsts = [c.toks[0] for c in soups]
    assert {min(t.length, 4) for t in firsts if t.kind == "first"} == {1, 2, 3, 4}  # first byte 18, 19, 20, >= 21
    assert any(t.kind == "lit" and t.ip == 0 for t in firsts)                        # first byte <= 15
    assert any(t.kind == "m4" and t.dist >= 32768 for t in toks) and any(t.kind == "m4" and t.dist < 32768 for t in toks)
    assert any(t.kind == "m3" and t.size > 3 for t in toks) and any(t.kind == "m4" and t.size > 3 for t in toks)


def test_chunk_ends_have_the_lengths_they_claim(geom, fam):
    for codec in dc.CODECS:
        seen = {c.tag for c in dc.of_codec(fam["chunk-ends"], codec)}
        assert seen >= {(end, n) for end in ("lit", "match") for n in dc.chunk_end_lengths(geom)}
    assert dc.chunk_end_lengths(geom) == [*range(253, 261), *range(509, 517), *range(2045, 2053)]
    for c in fam["chunk-ends"]:
        if c.tag[0] != "empty":
            (raw_len, chunks), = dc.blocks_of(c.codec, c.stream)
            assert len(chunks) == 1 and len(chunks[0]) == c.tag[1], c.name
            want = {"lzo": "end", "lz4": "last", "snappy": "lit" if c.tag[0] == "lit" else "copy"}[c.codec]
            assert c.toks[-1].kind.startswith(want), c.name
            if c.codec == "lzo":
                assert c.toks[-2].kind == ("lit" if c.tag[0] == "lit" else "m2"), c.name
    empty, = [c for c in fam["chunk-ends"] if c.tag[0] == "empty"]
    assert empty.raw == b"" and empty.braws == () and set(empty.stream) == {0}


def test_snappy_chunk_blocks_and_layouts(geom, fam):
    per = {}
    for c in fam["snappy-chunks"]:
        (raw_len, chunks), = dc.blocks_of(c.codec, c.stream)
        per.setdefault(len(chunks), set())
        for ch in chunks:
            vlen = next(i + 1 for i, b in enumerate(ch) if not b & 0x80)
            per[len(chunks)].add(vlen)
        starts = [t for t in c.toks if t.op == 0]  # every chunk opens with a literal ...
        nexts = [c.toks[c.toks.index(t) + 1] for t in starts]
        assert all(t.kind.startswith("lit") for t in starts) and len(starts) == len(chunks)
        assert all(n.kind.startswith("copy") and n.dist == n.op for n in nexts), c.name  # ... and a copy to its start
    assert set(per) == {1, 2, 5} and per[2] | per[5] == {1, 2, 3} and per[5] == {1, 2, 3}
    for codec in dc.CODECS:
        assert {len(c.braws) for c in dc.of_codec(fam["layout"], codec)} == {1, 3, 4, 5, 9}
    w = geom["waves_per_block"]
    assert {n % w for n in (1, 3, 4, 5, 9)} == {0, 1, 3} and 9 > 2 * w


def test_batch_places_every_stream_on_the_asked_phase(geom, fam):
    align = geom["lds_align"]
    for codec in dc.CODECS:
        cases = dc.of_codec(fam["chunk-ends"], codec)
        for phase in range(align):
            streams, outs, braws = dc.batch(codec, cases, phase, align)
            pos, starts = 0, {}
            for s in streams:
                starts[pos] = s
                pos += len(s)
            mine = [p for p, s in starts.items() if any(s is c.stream for c in cases)]
            assert len(mine) == len(cases) and all(p % align == phase for p in mine), (codec, phase)
            assert b"".join(outs) == b"".join(braws)
            for s, o in zip(streams, outs):
                assert dc.stream_decode(codec, s)[0] == o
