"""Gzip members (RFC 1952) for the host and device gzip decoders, assembled around the deflate bodies of
tests/inflate_cases.py: a body is one of its zlib streams minus the 2-byte header and the 4-byte Adler-32.
Python's zlib module with wbits=31 judges every case first (tests/test_gzip_cases_cpu.py); only then do the
in-tree decoders see it.

  gzip_valid_cases     every valid body behind the bare 10-byte header Hadoop's writers emit
  header_matrix        about a dozen bodies under every header shape and at header lengths that put the
                       body's first byte at every alignment of the kernel's 4-byte-aligned window base and on
                       each side of the first register window
  invalid_members      members zlib refuses: header, trailer and re-wrapped deflate-level faults
  multi_member_cases   two and three members back to back, one of which decodes to nothing
"""
import struct
import zlib

from tests.inflate_cases import invalid_cases, valid_cases

FTEXT, FHCRC, FEXTRA, FNAME, FCOMMENT = 1, 2, 4, 8, 16
GZ_TEXT = b"CRC-32 and ISIZE cover the decoded bytes" * 11  # what the header and trailer cases decode to

# the bodies the header matrix is laid over: the first case is added to these
MATRIX_BODIES = ("stored_65535", "stored_entered_at_phase_3", "dynamic_15_bit_codes", "literals_64_then_match",
                 "match_ends_at_last_byte", "len_258_dist_1", "pending_literals_dist_1", "literals_63_then_match",
                 "literals_65_then_match", "sync_flushed_segments", "match_source_at_byte_0")
# invalid_cases() whose fault lies in the deflate data (the others' lies in the zlib wrapper)
DEFLATE_INVALID = ("btype_3", "stored_len_nlen", "hlit_287", "hlit_288", "hdist_31", "hdist_32",
                   "oversubscribed_literal_lengths", "oversubscribed_distance_lengths",
                   "oversubscribed_code_length_code", "incomplete_literal_lengths", "incomplete_distance_lengths",
                   "incomplete_distance_single_2_bit_code", "incomplete_code_length_code",
                   "repeat_16_with_no_previous_length", "repeat_past_the_last_length", "no_code_for_end_of_block",
                   "fixed_literal_length_symbol_286", "fixed_literal_length_symbol_287", "fixed_distance_code_30",
                   "fixed_distance_code_31", "distance_beyond_output", "distance_beyond_output_at_start")
DEFLATE_CUT = ("cut_inside_dynamic_header", "cut_inside_symbols", "cut_inside_extra_bits", "cut_inside_stored_len",
               "cut_inside_stored_bytes")


def header(flg=0, extra=None, name=None, comment=None, mtime=0, xfl=0, os_code=255):
    """A member header. The optional fields are written when given, FHCRC when its bit is in flg."""
    flg |= (FEXTRA if extra is not None else 0) | (FNAME if name is not None else 0) | (FCOMMENT if comment is not None else 0)
    h = b"\x1f\x8b\x08" + bytes([flg]) + struct.pack("<I", mtime) + bytes([xfl, os_code])
    if extra is not None:
        h += struct.pack("<H", len(extra)) + extra
    for field in (name, comment):
        if field is not None:
            assert 0 not in field
            h += field + b"\x00"
    if flg & FHCRC:
        h += struct.pack("<H", zlib.crc32(h) & 0xFFFF)
    return h


def trailer(raw):
    return struct.pack("<II", zlib.crc32(raw), len(raw) & 0xFFFFFFFF)


def member(body, raw, hdr=None):
    return (header() if hdr is None else hdr) + body + trailer(raw)


def _filler(n, seed=7):
    """n bytes, none of them zero."""
    return bytes(1 + (seed * 37 + i * 11) % 255 for i in range(n))


def header_of_length(n):
    """The bare header (10) or one with an FNAME that makes it n bytes long."""
    assert n >= 10
    return header() if n == 10 else header(name=_filler(n - 11))


def header_shapes():
    """The seven shapes: (name, header bytes)."""
    return [
        ("bare", header()),
        ("fname_245", header(name=_filler(245))),
        ("fextra_xlen_0", header(extra=b"")),
        ("fextra_xlen_65535", header(extra=bytes(i * 7 & 0xFF for i in range(65535)))),
        ("fhcrc", header(FHCRC)),
        ("flg_1e_all_fields", header(FHCRC, extra=b"\x41\x70\x04\x00abcd", name=b"part-r-00000", comment=b"map output")),
        ("ftext", header(FTEXT, mtime=0x5F3759DF, xfl=2, os_code=3)),
    ]


def bodies(window=256, stage=64):
    """[(name, deflate body, raw)] of every valid case."""
    return [(name, stream[2:-4], want) for name, stream, want in valid_cases(window, stage)]


def gzip_valid_cases(window=256, stage=64):
    """[(name, member, raw)]: every valid body behind the bare header."""
    return [(name, member(body, want), want) for name, body, want in bodies(window, stage)]


def matrix_bodies(window=256, stage=64):
    every = bodies(window, stage)
    by_name = {b[0]: b for b in every}
    picked = [every[0]] + [by_name[n] for n in MATRIX_BODIES if n in by_name and n != every[0][0]]
    assert len(picked) >= 10 and any(n.startswith("stored") for n, _, _ in picked)
    return picked


def matrix_header_lengths(window=256):
    """10..13: the body at every alignment of the window's 4-byte-aligned base; window - 6 .. window + 6: the
    body's first byte on each side of the first register window."""
    return [10, 11, 12, 13] + list(range(window - 6, window + 7))


def header_matrix(window=256, stage=64):
    """[(name, member, raw, header length)]"""
    out = []
    for bname, body, want in matrix_bodies(window, stage):
        for n in matrix_header_lengths(window):
            out.append(("%s@hdr%d" % (bname, n), member(body, want, header_of_length(n)), want, n))
        for sname, hdr in header_shapes():
            out.append(("%s@%s" % (bname, sname), member(body, want, hdr), want, len(hdr)))
    return out


def _base_member():
    c = zlib.compressobj(6, zlib.DEFLATED, -15)
    return c.compress(GZ_TEXT) + c.flush()


def invalid_members():
    """[(name, bytes)]: zlib's inflate with wbits=31 refuses each (an error, or never reaching the end)."""
    body = _base_member()
    good = member(body, GZ_TEXT)
    hdr = header()
    out = [
        ("magic_1f_8c", b"\x1f\x8c" + good[2:]),
        ("cm_7", good[:2] + b"\x07" + good[3:]),
        ("flg_0x20", good[:3] + b"\x20" + good[4:]),
    ]
    h = header(FHCRC)
    bad = h[:-2] + struct.pack("<H", (struct.unpack("<H", h[-2:])[0] + 1) & 0xFFFF)
    out.append(("fhcrc_off_by_one", member(body, GZ_TEXT, bad)))
    for k in range(1, 10):
        out.append(("header_cut_after_%d" % k, hdr[:k]))
    out.append(("fname_without_terminator", header(name=_filler(40))[:-1]))
    out.append(("fname_without_terminator_long", header(name=_filler(700))[:-1]))
    out.append(("xlen_past_the_end", b"\x1f\x8b\x08\x04" + b"\x00" * 6 + struct.pack("<H", 5000) + b"x" * 100))
    out.append(("xlen_field_cut", b"\x1f\x8b\x08\x04" + b"\x00" * 6 + b"\x10"))
    out.append(("fhcrc_field_cut", header(FHCRC)[:-1]))
    for k in range(1, 9):
        out.append(("trailer_cut_by_%d" % k, good[:-k]))
    for bit in (0, 13, 31):
        flipped = bytearray(good)
        flipped[len(good) - 8 + bit // 8] ^= 1 << (bit % 8)
        out.append(("crc_bit_%d_flipped" % bit, bytes(flipped)))
        flipped = bytearray(good)
        flipped[len(good) - 4 + bit // 8] ^= 1 << (bit % 8)
        out.append(("isize_bit_%d_flipped" % bit, bytes(flipped)))
    streams = dict(invalid_cases())
    for name in DEFLATE_INVALID:  # the fault comes ahead of the trailer: what the trailer says does not matter
        out.append(("deflate_" + name, hdr + streams[name][2:-4] + b"\x00" * 8))
    for name in DEFLATE_CUT:
        out.append(("deflate_" + name, hdr + streams[name][2:]))
    return out


def invalid_raw_len(name):
    """The output room a decoder is given for an invalid member: the true length where the deflate data is
    whole (so that only the fault named is in the way), 64 KiB otherwise."""
    return 1 << 16 if name.startswith("deflate_") else len(GZ_TEXT)


def multi_member_cases(window=256, stage=64):
    """[(name, bytes, raw, members)]: concatenated members decode to the concatenated outputs."""
    picked = matrix_bodies(window, stage)
    a, b, c = picked[0], picked[3], picked[4]
    empty = member(b"\x03\x00", b"")
    ma, mb, mc = (member(x[1], x[2]) for x in (a, b, c))
    fn = member(b[1], b[2], header(FHCRC, name=b"second"))
    return [
        ("two_members", ma + mb, a[2] + b[2], 2),
        ("two_members_second_has_fields", ma + fn, a[2] + b[2], 2),
        ("three_members", ma + mb + mc, a[2] + b[2] + c[2], 3),
        ("three_members_empty_in_the_middle", ma + empty + mc, a[2] + c[2], 3),
        ("two_members_first_empty", empty + mb, b[2], 2),
        ("two_members_last_empty", ma + empty, a[2], 2),
        ("two_empty_members", empty + empty, b"", 2),
    ]
