"""Every device block-decode kernel on the assembled cases of tests/decode_cases.py: token kinds the
in-tree encoders never emit (LZO M1 in both forms, hand-set M4, Snappy copy-4 and literal tags 61..63),
tokens cut by the register and LDS windows, the copy thresholds, the store-fence bookkeeping, chunk ends,
block layouts, the prefix decode looked at byte by byte, and one corrupt stream per check.

A family is one launch per kernel variant. The expected bytes are the assembler's, which the CPU test has
already held against the Python oracle and the host decoders.
"""
import re

import pytest

from tests import decode_cases as dc

pytestmark = pytest.mark.gpu

VARIANTS = {
    "lzo-lean": ("lzo", {}),
    "lzo-register-window": ("lzo", {"UDA_DECODE_WINDOW": "reg"}),
    "lzo-lds-window": ("lzo", {"UDA_DECODE_WINDOW": "lds"}),
    "lzo-lane": ("lzo", {"UDA_LZO_LANE": "1"}),
    "snappy-register-window": ("snappy", {}),
    "snappy-lds-window": ("snappy", {"UDA_DECODE_WINDOW": "lds"}),
    "lz4-lean": ("lz4", {}),
}
FAMILIES = {
    "lzo": ("token-at-window-edge", "extension-runs", "literal-lengths", "match-shapes", "fence", "chunk-ends",
            "lzo-states", "layout", "prefix-targets"),
    "snappy": ("token-at-window-edge", "literal-lengths", "match-shapes", "fence", "chunk-ends", "snappy-chunks",
               "layout", "prefix-targets"),
    "lz4": ("token-at-window-edge", "extension-runs", "literal-lengths", "match-shapes", "fence", "chunk-ends",
            "layout", "prefix-targets"),
}
PAIRS = [(v, f) for v, (codec, _) in VARIANTS.items() for f in FAMILIES[codec]]
SENTINEL = 0xA5
GUARD = 256


@pytest.fixture(scope="module")
def geom(native):
    return native.gpu_decode_geometry()


@pytest.fixture(scope="module")
def fam(geom):
    return dc.families(geom)


@pytest.fixture(scope="module")
def bad(geom):
    return dc.corrupt_cases(geom)


def use(monkeypatch, variant):
    codec, env = VARIANTS[variant]
    for k in ("UDA_DECODE_WINDOW", "UDA_LZO_LANE"):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    return codec


def first_chunk_phase(geom):
    """A stream that starts here has its first chunk on a multiple of lds_align (8 bytes of headers), so
    chunk offsets are window offsets in the kernels that base their window on the address."""
    return (geom["lds_align"] - 8) % geom["lds_align"]


def wrong_streams(cases, streams, got, outs):
    by_stream = {id(c.stream): c.name for c in cases}
    return [by_stream.get(id(s), "filler") for s, g, o in zip(streams, got, outs) if g != o]


def decode_and_compare(native, codec, cases, phase, geom):
    streams, outs, braws = dc.batch(codec, cases, phase, geom["lds_align"])
    got, blocks, _ = native.gpu_block_decode(codec, streams)
    assert blocks == len(braws)
    wrong = wrong_streams(cases, streams, got, outs)
    assert not wrong, "%d of %d streams decoded wrong: %s" % (len(wrong), len(streams), wrong[:12])


@pytest.mark.parametrize("variant,family", PAIRS)
def test_valid_cases_decode_to_the_oracle_bytes(require_gpu, native, monkeypatch, geom, fam, variant, family):
    codec = use(monkeypatch, variant)
    decode_and_compare(native, codec, dc.of_codec(fam[family], codec), first_chunk_phase(geom), geom)


@pytest.mark.parametrize("variant", VARIANTS)
def test_block_sources_at_every_address_modulo_the_vector_width(require_gpu, native, monkeypatch, geom, fam, variant):
    """The layout blocks and the chunk ends with every stream at each address modulo lds_align: the LDS
    fill's aligned and bytewise paths, and the unaligned 4- and 16-byte loads. (A stream of fewer than four
    bytes is not a block stream, so the streams in front are 13..28-byte blocks.)"""
    codec = use(monkeypatch, variant)
    cases = dc.of_codec(fam["layout"], codec) + dc.of_codec(fam["chunk-ends"], codec)[::3]
    for phase in range(geom["lds_align"]):
        decode_and_compare(native, codec, cases, phase, geom)


def prefix_expected(braws, clip):
    want = bytearray([SENTINEL]) * (len(braws) * clip + GUARD)
    for b, raw in enumerate(braws):
        want[b * clip:b * clip + min(clip, len(raw))] = raw[:clip]
    return bytes(want)


def check_prefix(native, codec, cases, clip, geom):
    streams, _, braws = dc.batch(codec, cases, first_chunk_phase(geom), geom["lds_align"])
    got, blocks, _ = native.gpu_block_decode(codec, streams, clip=clip)
    assert blocks == len(braws)
    want = prefix_expected(braws, clip)
    assert len(got) == len(want)
    if got != want:
        slots = [b for b in range(len(braws)) if got[b * clip:(b + 1) * clip] != want[b * clip:(b + 1) * clip]]
        first = next(i for i in range(len(want)) if got[i] != want[i])
        raise AssertionError("clip %d: %d of %d slots wrong (first %s), guard %s, first wrong byte %d of slot %d: %#x not %#x"
                             % (clip, len(slots), len(braws), slots[:8], "intact" if got[-GUARD:] == want[-GUARD:] else "hit",
                                first % clip, first // clip, got[first], want[first]))


@pytest.mark.parametrize("variant,family", [p for p in PAIRS if p[1] != "prefix-targets"])
def test_prefix_decode_writes_the_prefix_and_nothing_else(require_gpu, native, monkeypatch, geom, fam, variant, family):
    """Block b's first min(clip, raw) bytes at b * clip, as production lays the slots out, and every other
    byte of the buffer and of the guard behind it still the fill byte."""
    codec = use(monkeypatch, variant)
    assert dc.prefix_clips(geom) == (1, 11, 63, 64, 65, 127, 128, 129)
    for clip in dc.prefix_clips(geom):
        check_prefix(native, codec, dc.of_codec(fam[family], codec), clip, geom)


@pytest.mark.parametrize("variant", VARIANTS)
def test_prefix_decode_stops_inside_tokens(require_gpu, native, monkeypatch, geom, fam, variant):
    """The clip inside a literal and inside a match of at most short_copy bytes and of more (an overlapping
    one among them), exactly between two tokens, in a Snappy block's second chunk, and one byte short of, at
    and one byte past the block's size."""
    codec = use(monkeypatch, variant)
    cases = dc.of_codec(fam["prefix-targets"], codec)
    whats = {c.tag[0] for c in cases}
    assert whats >= {"short_literal", "long_literal", "short_match", "short_overlapping_match", "long_overlapping_match",
                     "long_match", "token_boundary"} and ("second_chunk" in whats) == (codec == "snappy")
    for clip in sorted({clip for c in cases for clip in c.tag[1]}):
        check_prefix(native, codec, cases, clip, geom)


@pytest.mark.parametrize("variant", [v for v in VARIANTS if v != "lz4-lean"])
def test_corrupt_cases_are_reported(require_gpu, native, monkeypatch, bad, variant):
    """One launch per stream; each is refused by a bounds test ahead of the access it guards (the framing
    walk, ensure() / the three-byte margin of the lean parse, the distance and length tests), in every
    variant. LZ4's cases are in test_gpu_lz4_decode.py."""
    codec = use(monkeypatch, variant)
    mine = [b for b in bad if b.codec == codec]
    assert len(mine) > 25
    accepted = []
    for b in mine:
        try:
            native.gpu_block_decode(codec, [b.stream])
        except Exception as e:
            assert re.search("corrupt|framing", str(e)), (b.name, e)
        else:
            accepted.append(b.name)
    assert not accepted
