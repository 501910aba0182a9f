"""The gzip members of tests/gzip_cases.py, judged by Python's zlib module alone (wbits=31: gzip framing), an
oracle that is not ours, so that the cases themselves are right before any decoder of this tree sees them.
Nothing here needs the native library."""
import gzip
import zlib

from tests.gzip_cases import (GZ_TEXT, gzip_valid_cases, header_matrix, header_shapes, invalid_members,
                              matrix_header_lengths, multi_member_cases)

WINDOW, STAGE = 256, 64  # inflate_geometry() of the device kernel; tests/test_gzip_codec.py holds them against it
TAIL = b"\x01\x02\x03\x04"


def judged(stream):
    """(output, eof, unused_data) or None if zlib raises."""
    d = zlib.decompressobj(31)
    try:
        out = d.decompress(stream)
    except zlib.error:
        return None
    return out, d.eof, d.unused_data


def test_every_valid_body_under_the_bare_header():
    cases = gzip_valid_cases(WINDOW, STAGE)
    assert len(cases) >= 65 and len(cases) % 4 != 0  # several workgroups, the last partly filled
    for name, stream, want in cases:
        assert stream[:4] == b"\x1f\x8b\x08\x00" and len(stream) >= 20, name
        assert judged(stream + TAIL) == (want, True, TAIL), name


def test_every_valid_body_under_every_header_shape():
    shapes = header_shapes()
    assert [n for n, _ in shapes] == ["bare", "fname_245", "fextra_xlen_0", "fextra_xlen_65535", "fhcrc",
                                      "flg_1e_all_fields", "ftext"]
    assert [h[3] for _, h in shapes] == [0, 8, 4, 4, 2, 0x1e, 1]
    assert len(shapes[1][1]) == WINDOW and len(shapes[3][1]) == 12 + 65535
    from tests.gzip_cases import bodies, member
    for name, body, want in bodies(WINDOW, STAGE):
        for sname, hdr in shapes:
            assert judged(member(body, want, hdr) + TAIL) == (want, True, TAIL), (name, sname)


def test_header_matrix():
    cases = header_matrix(WINDOW, STAGE)
    lengths = matrix_header_lengths(WINDOW)
    assert set(lengths) >= {10, 11, 12, 13} | set(range(WINDOW - 6, WINDOW + 7))
    names = {c[0].split("@")[0] for c in cases}
    assert len(names) >= 10
    assert {"stored_65535", "dynamic_15_bit_codes", "literals_64_then_match", "match_ends_at_last_byte"} <= names
    for body in names:
        mine = [c for c in cases if c[0].split("@")[0] == body]
        assert {c[3] for c in mine} >= set(lengths), body
        assert {c[3] % 4 for c in mine if c[3] < 14} == {0, 1, 2, 3}, body
    for name, stream, want, hlen in cases:
        assert judged(stream) == (want, True, b""), name
        assert judged(stream + TAIL) == (want, True, TAIL), name
        # the header is as long as the matrix says: the deflate data alone decodes from there
        d = zlib.decompressobj(-15)
        assert d.decompress(stream[hlen:]) == want and d.eof and len(d.unused_data) == 8, name


def test_invalid_members_are_refused():
    cases = invalid_members()
    names = [n for n, _ in cases]
    assert len(set(names)) == len(names) and len(names) == 59  # 32 wrapper faults, 27 deflate-level ones
    for name, stream in cases:
        r = judged(stream)
        assert r is None or not r[1], name
    # the trailer flips really are the only fault of their members
    for name, stream in cases:
        if name.startswith(("crc_bit", "isize_bit")):
            d = zlib.decompressobj(-15)
            assert d.decompress(stream[10:]) == GZ_TEXT and d.eof and len(d.unused_data) == 8, name


def test_multi_member_cases():
    cases = multi_member_cases(WINDOW, STAGE)
    assert {c[3] for c in cases} == {2, 3}
    assert any("empty_in_the_middle" in c[0] for c in cases)
    for name, stream, want, members in cases:
        assert gzip.decompress(stream) == want, name
        rest, n = stream, 0
        while rest:  # member by member, as zlib hands them out
            out, eof, rest = judged(rest)
            assert eof, name
            n += 1
        assert n == members, name
