"""The shuffle job's host-only round planner (csrc/gpu/shuffle_plan.cc): send counts, receive layout, send
slices, staged spans, verification / own-cell lists and H2D copy lists of every rank of a simulated job,
against a brute-force oracle, under ASan + UBSan in a program of its own."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_shuffle_plan_native_selftest_under_sanitizers(tmp_path):
    """tests/native/shuffle_plan_selftest.cc with csrc/gpu/shuffle_plan.cc, which needs neither HIP nor
    the device engine's header; never loaded into Python."""
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "shuffle_plan_selftest")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I" + os.path.join(ROOT, "csrc", "gpu"),
                    os.path.join(ROOT, "tests", "native", "shuffle_plan_selftest.cc"),
                    os.path.join(ROOT, "csrc", "gpu", "shuffle_plan.cc"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert " checks, 0 failures" in r.stdout
