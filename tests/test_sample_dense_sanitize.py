"""The per-row text of csrc/pn_adapt.h (the row controller and the plan / coefficients of a row's interpolated outputs) compiled
with AddressSanitizer + UndefinedBehaviorSanitizer on the CPU as a stand-alone program (tests/native/rows_dense_selftest.cpp)."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")
def test_row_plan_and_controller_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "rows_dense_selftest")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "pnode_amd", "csrc"),
           os.path.join(ROOT, "tests", "native", "rows_dense_selftest.cpp"), "-o", exe]
    subprocess.run(cmd, check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="halt_on_error=1")
    out = subprocess.run([exe], env=env, capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "rows dense selftest ok" in out.stdout
