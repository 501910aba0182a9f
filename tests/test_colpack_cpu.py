"""colpack on the host (csrc/codec/colpack.{h,cc}): the reference encoder against a pure-numpy
implementation of the format, both decoders, header rejection, and the stand-alone selftest under
ASan + UBSan."""
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

from tests.colpack_cases import BUF_RECORDS, HEADER_BYTES, cases, np_encode

CASES = cases()


@pytest.mark.parametrize("name", list(CASES))
def test_colpack_encode_matches_numpy_and_roundtrips(native, name):
    recs, expect = CASES[name]
    n, L = recs.shape
    raw = recs.tobytes()
    want, packed, S = np_encode(recs, BUF_RECORDS)
    got = native.colpack_encode(raw, L, BUF_RECORDS)
    assert got == want
    assert len(got) % 64 == 0
    if expect == "raw":
        assert not packed and len(got) == HEADER_BYTES
        with pytest.raises(ValueError):
            native.colpack_decode(got, L, n)
        return
    assert packed
    if expect is not None:
        assert S <= expect
    assert len(got) >= HEADER_BYTES + S * n + 8 and got[HEADER_BYTES + S * n:] == bytes(len(got) - HEADER_BYTES - S * n)
    scalar = native.colpack_decode(got, L, n, "scalar")
    assert scalar == raw
    assert native.colpack_decode(got, L, n) == raw
    if native.colpack_have_bmi2():
        assert native.colpack_decode(got, L, n, "bmi2") == scalar
    # a range of rows, as the consumers unpack buffer by buffer
    for row0, rows in ((0, 1), (n - 1, 1), (n // 3, n - n // 3), (min(n, BUF_RECORDS), n - min(n, BUF_RECORDS))):
        for path in ("scalar", "bmi2") if native.colpack_have_bmi2() else ("scalar",):
            assert native.colpack_decode(got, L, n, path, row0, rows) == raw[row0 * L:(row0 + rows) * L], (path, row0)


def test_colpack_this_cpu_runs_the_bmi2_path(native):
    with open("/proc/cpuinfo") as f:
        flags = f.read()
    assert native.colpack_have_bmi2() == (" bmi2" in flags)


def _patched(piece: bytes, off: int, fmt: str, value) -> bytes:
    return piece[:off] + struct.pack(fmt, value) + piece[off + struct.calcsize(fmt):]


def test_colpack_bad_headers_rejected(native):
    recs, _ = CASES["terasort_257"]
    n, L = recs.shape
    good = native.colpack_encode(recs.tobytes(), L, BUF_RECORDS)
    assert native.colpack_decode(good, L, n) == recs.tobytes()
    S = struct.unpack_from("<I", good, 28)[0]
    bad = {
        "magic": _patched(good, 0, "<I", 0x12345678),
        "version": _patched(good, 4, "<I", 2),
        "L": _patched(good, 8, "<I", 96),
        "L_zero": _patched(good, 8, "<I", 0),
        "records_more": _patched(good, 16, "<Q", n + 1),
        "records_huge": _patched(good, 16, "<Q", 1 << 62),
        "S_more": _patched(good, 28, "<I", S + 1),
        "S_less": _patched(good, 28, "<I", S - 1),
        "groups": _patched(good, 32, "<I", 12),
        "gb": _patched(good, 64 + 512 + 3, "<B", 8),
        "mask": _patched(good, 64 + 8, "<Q", 0x0505050505050505),
        "truncated_rows": good[:len(good) - 64],
        "truncated_header": good[:HEADER_BYTES - 1],
        "empty": b"",
    }
    for name, piece in bad.items():
        with pytest.raises(ValueError):
            native.colpack_decode(piece, L if name not in ("L", "L_zero") else 0, n if "records" not in name else 0)
    with pytest.raises(ValueError):  # a well-formed piece of another record count than the item says
        native.colpack_decode(good, L, n - 1)
    with pytest.raises(ValueError):
        native.colpack_decode(good, 100, n)


def test_colpack_native_selftest_under_sanitizers(tmp_path):
    """tests/native/colpack_selftest.cc, a program of its own, built with csrc/codec/colpack.cc under
    ASan + UBSan: encode and both decoders on exact-size heap buffers, and corrupted or truncated
    pieces, which must be rejected without a read out of bounds."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "colpack_selftest")
    subprocess.run([cxx, "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I" + os.path.join(root, "csrc"), os.path.join(root, "tests", "native", "colpack_selftest.cc"),
                    os.path.join(root, "csrc", "codec", "colpack.cc"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert " 0 failures" in r.stdout
