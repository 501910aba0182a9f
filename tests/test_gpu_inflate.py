"""Device inflate (csrc/gpu/inflate.hip, one wave per zlib stream) on the hand-assembled cases of
tests/inflate_cases.py, which Python's zlib module has judged (tests/test_inflate_cases_cpu.py), and on
streams zlib wrote at every level and strategy. The binding puts 256 guard bytes of 0xA5 behind every
output and fails on a changed one, so every call here is also a bounds check; the invalid streams return
from their launch with a status word, as the corrupt-block tests of the block decoders do.
"""
import zlib

import pytest

from tests.inflate_cases import ADLER_TEXT, invalid_cases, valid_cases
from tests.test_zlib_codec import roundtrip_streams

pytestmark = pytest.mark.gpu

INVALID = invalid_cases()


@pytest.fixture(scope="module")
def valid(native):
    g = native.gpu_inflate_geometry()
    cases = valid_cases(g["window"], g["literal_stage"])
    assert len(cases) >= 65 and len(cases) % g["waves_per_block"] != 0  # several workgroups, the last partly filled
    return cases


def test_inflate_geometry(native):
    g = native.gpu_inflate_geometry()
    assert g["waves_per_block"] == 4 and g["lds_per_wave"] <= 8192
    assert g["window"] % g["window_align"] == 0 and g["literal_stage"] == 64


def test_valid_cases_in_one_launch(require_gpu, native, valid):
    streams = [c[1] for c in valid]
    outs, consumed, _ = native.gpu_inflate_streams(streams, [len(c[2]) for c in valid])
    for (name, stream, want), out, used in zip(valid, outs, consumed):
        assert out == want, name
        assert used == len(stream), name


def test_valid_cases_one_launch_each(require_gpu, native, valid):
    for name, stream, want in valid:
        outs, consumed, _ = native.gpu_inflate_streams([stream], [len(want)])
        assert outs == [want] and consumed == [len(stream)], name


def test_valid_cases_with_four_trailing_bytes(require_gpu, native, valid):
    """An IFile checksum behind the stream is not the stream's: consumed = len - 4."""
    streams = [c[1] + zlib.crc32(c[1]).to_bytes(4, "big") for c in valid]
    outs, consumed, _ = native.gpu_inflate_streams(streams, [len(c[2]) for c in valid])
    for (name, stream, want), out, used in zip(valid, outs, consumed):
        assert out == want and used == len(stream), name


def test_levels_and_strategies_in_one_launch(require_gpu, native):
    cases = roundtrip_streams()
    assert max(len(raw) for _, _, raw in cases) <= 300_000
    outs, consumed, _ = native.gpu_inflate_streams([st for _, st, _ in cases], [len(raw) for _, _, raw in cases])
    for (name, st, raw), out, used in zip(cases, outs, consumed):
        assert out == raw, name
        assert used == len(st), name


@pytest.mark.parametrize("name", [c[0] for c in INVALID])
def test_invalid_case_raises(require_gpu, native, name):
    """One launch per case; it returns with the stream's status set (every check is a bounds test ahead of the
    access), and the guards behind the 64 KiB output are untouched."""
    stream = dict(INVALID)[name]
    # (the two streams whose only fault is their Adler-32 decode in full: they get their true raw length)
    raw = len(ADLER_TEXT) if name.startswith("adler_mismatch") else 1 << 16
    with pytest.raises(Exception, match="corrupt|truncated|Adler"):
        native.gpu_inflate_streams([stream], [raw])


def test_invalid_cases_beside_valid_ones(require_gpu, native, valid):
    """A refused stream in a workgroup does not disturb its neighbours' outputs: the error names it."""
    name, stream = INVALID[5]
    streams = [valid[0][1], stream, valid[1][1], valid[2][1], valid[3][1]]
    raws = [len(valid[0][2]), 4096, len(valid[1][2]), len(valid[2][2]), len(valid[3][2])]
    with pytest.raises(Exception, match="map output #1"):
        native.gpu_inflate_streams(streams, raws)


@pytest.mark.parametrize("delta", [-1, 1])
def test_raw_len_off_by_one_raises(require_gpu, native, valid, delta):
    """A raw length one too small (the output would pass it: nothing is written there, the guards say) and
    one too large both raise."""
    picked = [c for c in valid if c[0] in ("len_258_dist_1", "stored_65535", "match_ends_at_last_byte",
                                          "literals_64_then_match", "sync_flushed_segments", "dynamic_15_bit_codes")]
    assert len(picked) == 6
    for name, stream, want in picked:
        with pytest.raises(Exception, match="corrupt|decodes to"):
            native.gpu_inflate_streams([stream], [len(want) + delta])
