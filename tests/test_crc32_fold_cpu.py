"""crc32_fold_state (csrc/engine/ifile_checksum.cc): a running CRC register carried over a segment whose own
register from zero is known, state * x^(8 * len) + seg_state. It is how the over-budget GPU merge chains the
per-slice device states of a partition (mapred.uda.ifile.checksum.over.budget=verify). No GPU needed.

The oracle of a segment's state is zlib.crc32(seg, 0xFFFFFFFF) ^ 0xFFFFFFFF: zlib takes its start value in
the finalized domain, so that is the register after the segment from a zero register.
"""
import os
import random
import shutil
import subprocess
import zlib

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

M = 0xFFFFFFFF
K256 = 256 << 10


def seg_state(seg):
    return zlib.crc32(seg, M) ^ M


def fold_all(native, segs):
    s = M
    for seg in segs:
        s = native.crc32_fold_state(s, seg_state(seg), len(seg))
    return s ^ M


def cut(buf, lengths):
    out, at = [], 0
    for n in lengths:
        out.append(buf[at:at + n])
        at += n
    assert at <= len(buf)
    out.append(buf[at:])
    return out


def test_fixed_lengths_fold_to_the_crc_of_the_whole(native):
    lengths = [0, 1, 15, 16, 17, 1024, 0, K256 - 1, K256, K256 + 1, 0]
    buf = random.Random(41).randbytes(sum(lengths) + 333)
    segs = cut(buf, lengths)
    assert [len(s) for s in segs[:-1]] == lengths and b"".join(segs) == buf
    assert fold_all(native, segs) == zlib.crc32(buf)


@pytest.mark.parametrize("seed", range(6))
def test_random_cuts_fold_to_the_crc_of_the_whole(native, seed):
    rng = random.Random(100 + seed)
    buf = rng.randbytes(rng.randint(1, 3 * K256))
    points = sorted(rng.randint(0, len(buf)) for _ in range(rng.randint(0, 12)))
    points += points[:2]  # repeated cut points: zero-length segments
    points = [0] + sorted(points) + [len(buf)]
    segs = [buf[a:b] for a, b in zip(points, points[1:])]
    assert b"".join(segs) == buf and any(len(s) == 0 for s in segs) == (len(set(points)) < len(points))
    assert fold_all(native, segs) == zlib.crc32(buf)


def test_a_zero_length_segment_is_the_identity(native):
    rng = random.Random(43)
    for _ in range(50):
        s = rng.getrandbits(32)
        assert native.crc32_fold_state(s, 0, 0) == s


def test_a_zero_state_stays_zero_over_any_length(native):
    for n in (0, 1, 15, 16, 17, 1024, K256 - 1, K256, K256 + 1, (1 << 31) + 5, 1 << 40):
        assert native.crc32_fold_state(0, 0, n) == 0
        assert seg_state(bytes(min(n, 4096))) == 0  # (the oracle agrees: zero bytes leave a zero register zero)


def test_fold_equals_crc32_combine_on_finalized_values(native):
    """The map is linear, so it is crc32_combine in the other domain: presets and inversions cancel."""
    rng = random.Random(47)
    a, b = rng.randbytes(777), rng.randbytes(K256 + 3)
    run = native.crc32_fold_state(zlib.crc32(a) ^ M, seg_state(b), len(b)) ^ M
    assert run == zlib.crc32(a + b) == native.crc32_combine(zlib.crc32(a), zlib.crc32(b), len(b))


def test_running_crc_selftest_under_sanitizers(tmp_path):
    """tests/native/crc32_fold_selftest.cc (uda::Crc32Running: device states and host bytes mixed) with
    csrc/engine/ifile_checksum.cc under ASan + UBSan, as a program of its own; never loaded into Python."""
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "crc32_fold_selftest")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I" + os.path.join(ROOT, "csrc", "include"),
                    os.path.join(ROOT, "tests", "native", "crc32_fold_selftest.cc"),
                    os.path.join(ROOT, "csrc", "engine", "ifile_checksum.cc"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert " 0 failures" in r.stdout
