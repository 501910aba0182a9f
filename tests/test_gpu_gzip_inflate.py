"""Device inflate in gzip mode (csrc/gpu/inflate.hip, one wave per member, and the batched CRC-32 behind it)
on the members of tests/gzip_cases.py, which Python's zlib module has judged (tests/test_gzip_cases_cpu.py):
every valid body behind the bare header, the header matrix that lays the body's first byte on every alignment
of the kernel's window base and on each side of its first register window, what gzip.compress writes, and
members that are wrong. The binding puts 256 guard bytes of 0xA5 behind every output and fails on a changed
one, so every call here is also a bounds check; an invalid member returns from its launch with a status."""
import zlib

import pytest

from tests.gzip_cases import gzip_valid_cases, header_matrix, invalid_members, invalid_raw_len, multi_member_cases
from tests.inflate_cases import valid_cases
from tests.test_gzip_codec import level_streams

pytestmark = pytest.mark.gpu

INVALID = invalid_members()


@pytest.fixture(scope="module")
def geometry(native):
    return native.gpu_inflate_geometry()


@pytest.fixture(scope="module")
def valid(geometry):
    cases = gzip_valid_cases(geometry["window"], geometry["literal_stage"])
    assert len(cases) >= 65 and len(cases) % geometry["waves_per_block"] != 0  # several workgroups, the last partly filled
    return cases


@pytest.fixture(scope="module")
def matrix(geometry):
    return header_matrix(geometry["window"], geometry["literal_stage"])


def inflate(native, streams, raws):
    return native.gpu_inflate_streams(streams, raws, 0, "gzip")


def test_valid_cases_in_one_launch(require_gpu, native, valid):
    outs, consumed, _ = inflate(native, [c[1] for c in valid], [len(c[2]) for c in valid])
    for (name, stream, want), out, used in zip(valid, outs, consumed):
        assert out == want, name
        assert used == len(stream), name


def test_header_matrix_in_one_launch(require_gpu, native, matrix):
    outs, consumed, _ = inflate(native, [c[1] for c in matrix], [len(c[2]) for c in matrix])
    for (name, stream, want, _), out, used in zip(matrix, outs, consumed):
        assert out == want, name
        assert used == len(stream), name


def test_four_trailing_bytes(require_gpu, native, valid, matrix):
    """An IFile checksum behind the member is not the member's: consumed = len(member)."""
    cases = [c[:3] for c in valid] + [c[:3] for c in matrix]
    streams = [c[1] + zlib.crc32(c[1]).to_bytes(4, "big") for c in cases]
    outs, consumed, _ = inflate(native, streams, [len(c[2]) for c in cases])
    for (name, stream, want), out, used in zip(cases, outs, consumed):
        assert out == want and used == len(stream), name


def test_gzip_compress_levels_in_one_launch(require_gpu, native):
    cases = level_streams()
    assert max(len(raw) for _, _, raw in cases) <= 300_000
    outs, consumed, _ = inflate(native, [st for _, st, _ in cases], [len(raw) for _, _, raw in cases])
    for (name, st, raw), out, used in zip(cases, outs, consumed):
        assert out == raw, name
        assert used == len(st), name


@pytest.mark.parametrize("name", [c[0] for c in INVALID])
def test_invalid_member_raises(require_gpu, native, name):
    """One launch per case; it returns with the member's status set (every header step and every copy is a
    bounds test ahead of its access), and the guards behind the output are untouched."""
    with pytest.raises(Exception, match="corrupt|truncated|CRC-32|length") as e:
        inflate(native, [dict(INVALID)[name]], [invalid_raw_len(name)])
    assert "guard" not in str(e.value)


def test_invalid_member_beside_valid_ones(require_gpu, native, valid):
    """A refused member in a workgroup does not disturb its neighbours: the error names it."""
    stream = dict(INVALID)["fhcrc_off_by_one"]
    streams = [valid[0][1], stream, valid[1][1], valid[2][1], valid[3][1]]
    raws = [len(valid[0][2]), invalid_raw_len("fhcrc_off_by_one"), len(valid[1][2]), len(valid[2][2]), len(valid[3][2])]
    with pytest.raises(Exception, match="map output #1"):
        inflate(native, streams, raws)


@pytest.mark.parametrize("delta", [-1, 1])
def test_raw_len_off_by_one_raises(require_gpu, native, valid, delta):
    picked = [c for c in valid if c[0] in ("len_258_dist_1", "stored_65535", "match_ends_at_last_byte",
                                          "literals_64_then_match", "sync_flushed_segments", "dynamic_15_bit_codes")]
    assert len(picked) == 6
    for name, stream, want in picked:
        with pytest.raises(Exception, match="corrupt|decodes to"):
            inflate(native, [stream], [len(want) + delta])


def test_two_member_stream_raises(require_gpu, native, geometry):
    """The device inflate decodes one member per stream: a second one behind it is said so, with or without
    an IFile checksum behind the two and whichever raw length the index gives."""
    for name, stream, want, members in multi_member_cases(geometry["window"], geometry["literal_stage"]):
        for tail in (b"", zlib.crc32(stream).to_bytes(4, "big")):
            with pytest.raises(Exception, match="holds more than one member"):
                inflate(native, [stream + tail], [max(len(want), 1)])


def test_zlib_container_is_unharmed(require_gpu, native, geometry):
    """The same binding, default container: the kernel's zlib path next to its new branch."""
    cases = valid_cases(geometry["window"], geometry["literal_stage"])
    outs, consumed, _ = native.gpu_inflate_streams([c[1] for c in cases], [len(c[2]) for c in cases])
    for (name, stream, want), out, used in zip(cases, outs, consumed):
        assert out == want and used == len(stream), name
    outs, consumed, _ = native.gpu_inflate_streams([c[1] for c in cases[:9]], [len(c[2]) for c in cases[:9]], 0, "zlib")
    assert outs == [c[2] for c in cases[:9]]
    with pytest.raises(Exception, match="corrupt zlib stream"):  # a gzip member is no zlib stream, and the reverse
        native.gpu_inflate_streams([gzip_valid_cases()[0][1]], [len(cases[0][2])])
    with pytest.raises(Exception, match="corrupt gzip stream"):
        inflate(native, [cases[0][1]], [len(cases[0][2])])
