"""raiko_amd/csrc/poly_lazy.hpp, the lazy 64-bit accumulation of the DEEP stage's streaming kernels, on the host: a
stand-alone program (tests/poly_lazy/check_poly_lazy.cpp) built with the undefined-behaviour sanitizer feeds the
accumulate / fold / finish functions their worst cases and compares with `% p` arithmetic in 128-bit integers."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_poly_lazy_worst_cases(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler")
    exe = str(tmp_path / "check_poly_lazy")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(ROOT, "raiko_amd", "csrc"), "-o", exe,
                    os.path.join(ROOT, "tests", "poly_lazy", "check_poly_lazy.cpp")], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "poly_lazy ok" in r.stdout
