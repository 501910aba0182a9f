"""The hand-assembled zlib streams of tests/inflate_cases.py: first against Python's zlib module, an oracle
that is not ours (so the cases themselves are right), then through the in-tree host inflater: the one-shot
zlib_decompress and the incremental Inflater behind BlockDecoder, fed 1, 7 and 4096 bytes at a time."""
import zlib

import pytest

from tests.inflate_cases import BOUNDARY_FAMILIES, boundary_cases, boundary_starts, invalid_cases, valid_cases

ZLIB = 4
FEEDS = (1, 7, 4096)


@pytest.fixture(scope="module")
def geometry(native):
    return native.gpu_inflate_geometry()


@pytest.fixture(scope="module")
def valid(geometry):
    return valid_cases(geometry["window"], geometry["literal_stage"])


INVALID = invalid_cases()


def test_case_set_is_what_the_device_tests_need(valid, geometry):
    names = [c[0] for c in valid]
    assert len(set(names)) == len(names)
    assert len(valid) >= 65  # several workgroups, the last one partly filled
    assert len(valid) % geometry["waves_per_block"] != 0
    assert max(len(c[2]) for c in valid) <= 300_000
    for kind in BOUNDARY_FAMILIES:
        assert sum(n.startswith(kind) for n in names) >= 20


def test_boundary_cases_cross_the_window_boundary(geometry):
    """From the assembler's own bit positions: around each of the first two refills of the kernel's input
    window (stream byte m * window; the window's base is a multiple of window_align, which divides it), every
    family has an item starting at every bit from 8 bytes before the boundary to 2 bytes behind it, and items
    that lie across it: a code with its extra bits, a LEN / NLEN field at each of its three straddling
    positions, and a dynamic header with the boundary in every eighth byte of it."""
    window, align = geometry["window"], geometry["window_align"]
    assert window % align == 0
    cases = boundary_cases(window)
    for m in (1, 2):
        edge = 8 * m * window
        for family in BOUNDARY_FAMILIES:
            mine = [c for c in cases if c[3] == family and c[4] == m]
            assert set(boundary_starts(window, m)) <= {c[5] for c in mine}, (family, m)
            across = [c for c in mine if c[5] < edge < c[6]]
            if family == "code_straddles_refill":
                # the boundary after each of the code's first 23 bits
                assert {edge - c[5] for c in across} >= set(range(1, 24)), (family, m)
            elif family == "stored_len_straddles_refill":
                # LEN / NLEN begins 1, 2 and 3 bytes before the boundary
                assert {edge - (c[6] - 32) for c in mine} >= {8, 16, 24}, (family, m)
                assert all((c[6] - 32) % 8 == 0 for c in mine)
            else:
                assert all(c[6] - c[5] > 8 * 150 for c in mine)  # (the header is 153 bytes)
                assert all(c[5] < edge < c[6] for c in mine if c[5] < edge)
                assert {(edge - c[5]) // 64 for c in across} >= set(range(0, 20)), (family, m)
    # and the streams are what valid_cases() hands to every decoder
    by_name = {c[0]: c for c in valid_cases(window, geometry["literal_stage"])}
    for c in cases:
        assert by_name[c[0]][1:] == c[1:3], c[0]


def test_phase_cases_present(valid):
    names = [c[0] for c in valid]
    assert {"stored_entered_at_phase_%d" % p for p in range(8)} <= set(names)
    assert {"end_of_block_at_phase_%d" % p for p in range(8)} <= set(names)


def test_valid_cases_by_python_zlib(valid):
    for name, stream, want in valid:
        d = zlib.decompressobj()
        assert d.decompress(stream) == want, name
        assert d.eof and d.unused_data == b"", name


def test_invalid_cases_by_python_zlib():
    for name, stream in INVALID:
        d = zlib.decompressobj()
        try:
            d.decompress(stream)
        except zlib.error:
            continue
        assert not d.eof, name


def test_valid_cases_one_shot(native, valid):
    for name, stream, want in valid:
        out, used = native.zlib_decompress(stream, len(want))
        assert out == want and used == len(stream), name
        # bytes behind the stream are not its own: reported as not consumed
        out, used = native.zlib_decompress(stream + b"\x01\x02\x03\x04", len(want))
        assert out == want and used == len(stream), name


def test_valid_cases_more_output_than_cap(native, valid):
    for name, stream, want in valid:
        if want:
            with pytest.raises(ValueError):
                native.zlib_decompress(stream, len(want) - 1)


@pytest.mark.parametrize("feed", FEEDS)
def test_valid_cases_incremental(native, valid, feed):
    for name, stream, want in valid:
        assert native.block_decompress(ZLIB, stream, feed) == want, name


@pytest.mark.parametrize("name", [c[0] for c in INVALID])
def test_invalid_case_refused(native, name):
    stream = dict(INVALID)[name]
    with pytest.raises(ValueError):
        native.zlib_decompress(stream, 1 << 20)
    for feed in FEEDS:
        with pytest.raises((ValueError, RuntimeError)):
            native.block_decompress(ZLIB, stream, feed)
