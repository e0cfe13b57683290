"""The host entry points behind dL/dt of a per-sample solve (pn_rows_dense_tgrad_host, pn_rows_tgrad_scatter_host: the shared text of
csrc/pn_adapt.h) compiled with AddressSanitizer + UndefinedBehaviorSanitizer on the CPU as a stand-alone program
(tests/native/rows_tgrad_selftest.cpp)."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")
def test_row_time_gradient_host_entry_points_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "rows_tgrad_selftest")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "pnode_amd", "csrc"),
           os.path.join(ROOT, "tests", "native", "rows_tgrad_selftest.cpp"), os.path.join(ROOT, "pnode_amd", "csrc", "pn_ts.cpp"),
           "-o", exe]
    subprocess.run(cmd, check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="halt_on_error=1")
    out = subprocess.run([exe], env=env, capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "rows tgrad selftest ok" in out.stdout
