"""The host-only RPQ planner (csrc/consumer/rpq_plan.cc): sparse-index walk, boundary search, splitter
choice and round slicing of the GPU hybrid merges, against a brute-force oracle, under ASan + UBSan in a
program of its own."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_rpq_plan_native_selftest_under_sanitizers(tmp_path):
    """tests/native/rpq_plan_selftest.cc with csrc/consumer/rpq_plan.cc and the IFile engine (ifile.cc, and
    the combiner its KVWriter links against); never loaded into Python."""
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "rpq_plan_selftest")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I" + os.path.join(ROOT, "csrc", "include"), "-I" + os.path.join(ROOT, "csrc", "consumer"),
                    os.path.join(ROOT, "tests", "native", "rpq_plan_selftest.cc"),
                    os.path.join(ROOT, "csrc", "consumer", "rpq_plan.cc"),
                    os.path.join(ROOT, "csrc", "engine", "combine.cc"),
                    os.path.join(ROOT, "csrc", "engine", "ifile.cc"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert " checks, 0 failures" in r.stdout
