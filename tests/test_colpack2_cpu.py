"""colpack version 2 on the host (csrc/codec/colpack.{h,cc}): the encoder against an independent
numpy / Python-int implementation of the format (tests/colpack2_cases.py), both decoders, ranges that
start inside a buffer, header rejection with its reasons, version 1 pieces through the same open and
decode, and the stand-alone selftest under ASan + UBSan."""
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

from tests.colpack2_cases import CASES, FLAG_DELTA, HEADER_BYTES, layout, reference
from tests.colpack_cases import np_encode


def _paths(native):
    return ("scalar", "bmi2") if native.colpack_have_bmi2() else ("scalar",)


@pytest.mark.parametrize("name", list(CASES))
def test_colpack2_encode_matches_numpy_and_roundtrips(native, name):
    c = CASES[name]
    recs, buf = c["recs"], c["buf"]
    n, L = recs.shape
    raw = recs.tobytes()
    want, packed, delta, S, offs, gbits = reference(name)
    got = native.colpack2_encode(raw, L, buf, c["ko"], c["kl"])
    assert got[:HEADER_BYTES] == want[:HEADER_BYTES]
    assert got == want
    assert len(got) % 64 == 0
    if c["delta"] is not None:
        assert delta == c["delta"]
    if c["packed"] is not None:
        assert packed == c["packed"]
    if not packed:
        assert len(got) == HEADER_BYTES
        with pytest.raises(ValueError, match="raw piece"):
            native.colpack_decode(got, L, n)
        return
    table = (-(-n // buf) * 16 + 63) // 64 * 64 if delta else 0
    end = HEADER_BYTES + table + S * n
    assert len(got) >= end + 8 and got[end:] == bytes(len(got) - end)
    for path in _paths(native):
        assert native.colpack_decode(got, L, n, path) == raw, path
    assert native.colpack_decode(got, L, n) == raw
    # ranges as the consumers take them (whole buffers) and ranges whose first row is no restart row
    starts = {0, n - 1, n // 3, min(n - 1, buf), min(n - 1, buf + 1), min(n - 1, 2 * buf - 1), max(0, n - buf - 3)}
    for row0 in sorted(starts):
        for rows in {1, min(n - row0, buf + 2), n - row0}:
            for path in _paths(native):
                assert native.colpack_decode(got, L, n, path, row0, rows) == raw[row0 * L:(row0 + rows) * L], (path, row0, rows)


def test_colpack2_sorted_terasort_beats_version_1(native):
    c = CASES["terasort_sorted"]
    _, packed, delta, S, _, _ = reference("terasort_sorted")
    S1 = np_encode(c["recs"], c["buf"])[2]
    assert packed and delta and S < S1
    shuffled = reference("terasort_shuffled")
    assert not shuffled[2]  # wrapped differences are as wide as the keys: plain (or raw)


def test_colpack2_layout_edges():
    """The two layouts the cases are built for: a word ending exactly at bit 64 of its load stays
    where the cursor is, one bit more moves it to the next byte boundary."""
    assert reference("fits_64_exactly")[4:6] == ([0, 5, 64], [5, 59, 9])
    assert reference("realigned_at_65")[4:6] == ([0, 8, 68], [5, 60, 9])
    offs, gbits = reference("group_64_after_misaligned")[4:6]
    assert gbits[:4] == [3, 64, 2, 1] and offs[:4] == [0, 8, 72, 74]
    assert layout([7, 0, 57, 1]) == ([0, 7, 7, 64], 9)


def test_colpack2_buf_records_1_turns_delta_off(native):
    c = CASES["buf_records_1"]
    got = native.colpack2_encode(c["recs"].tobytes(), 104, 1, 3, 10)
    assert struct.unpack_from("<I", got, 12)[0] & FLAG_DELTA == 0


def test_colpack_decode_still_takes_version_1(native):
    c = CASES["terasort_sorted"]
    recs = c["recs"]
    v1 = native.colpack_encode(recs.tobytes(), 104, c["buf"])
    assert v1 == np_encode(recs, c["buf"])[0]
    for path in _paths(native):
        assert native.colpack_decode(v1, 104, 2520, path) == recs.tobytes()
        assert native.colpack_decode(v1, 104, 2520, path, 79, 100) == recs[79:179].tobytes()


def _patched(piece: bytes, off: int, fmt: str, value) -> bytes:
    return piece[:off] + struct.pack(fmt, value) + piece[off + struct.calcsize(fmt):]


def test_colpack2_bad_headers_rejected_with_their_reason(native):
    c = CASES["terasort_sorted"]
    recs = c["recs"]
    n, L = recs.shape
    good = native.colpack2_encode(recs.tobytes(), L, c["buf"], 3, 10)
    assert native.colpack_decode(good, L, n) == recs.tobytes()
    flags = struct.unpack_from("<I", good, 12)[0]
    assert flags & FLAG_DELTA
    bo1 = struct.unpack_from("<H", good, 64 + 512 + 2)[0]
    plain = native.colpack2_encode(recs.tobytes(), L, c["buf"], 0, 0)  # no table: its rows start earlier
    bad = {
        "unknown version": _patched(good, 4, "<I", 3),
        "key field outside the record": _patched(good, 36, "<I", 95),  # key_off 95 + key_len 10 > 104
        "delta piece without buffer restarts": _patched(good, 24, "<I", 0),
        "group offsets do not match the masks": _patched(good, 64 + 512 + 2, "<H", bo1 + 1),
        "table and rows exceed the piece's length": good[:len(good) - 64],
        "delta piece without a key": _patched(plain, 12, "<I", 3),
        "row stride does not match the masks": _patched(good, 28, "<I", struct.unpack_from("<I", good, 28)[0] + 1),
    }
    for why, piece in bad.items():
        for path in ("auto", "scalar"):
            with pytest.raises(ValueError, match=why):  # raised by the open: nothing was unpacked
                native.colpack_decode(piece, L, n, path)
    # a key length past 16 bytes, and a delta flag set on a piece that has no table (rows past the length)
    with pytest.raises(ValueError, match="key field outside the record"):
        native.colpack_decode(_patched(good, 40, "<I", 17), L, n)
    one_buf = native.colpack2_encode(recs[:78].tobytes(), L, 78, 0, 0)
    forged = _patched(_patched(_patched(one_buf, 12, "<I", 3), 40, "<I", 10), 24, "<I", 1)  # 78 entries: 1280 more bytes
    with pytest.raises(ValueError, match="table and rows exceed the piece's length"):
        native.colpack_decode(forged, L, 78)


def test_colpack2_native_selftest_under_sanitizers(tmp_path):
    """tests/native/colpack2_selftest.cc, a program of its own, built with csrc/codec/colpack.cc under
    ASan + UBSan: the version 2 encoder and both decoders on exact-size heap buffers with guard bytes
    around dst, ranges that start inside a buffer, and corrupted or truncated pieces."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "colpack2_selftest")
    subprocess.run([cxx, "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I" + os.path.join(root, "csrc"), os.path.join(root, "tests", "native", "colpack2_selftest.cc"),
                    os.path.join(root, "csrc", "codec", "colpack.cc"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert " 0 failures" in r.stdout
