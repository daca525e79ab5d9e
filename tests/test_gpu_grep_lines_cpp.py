"""Builds tests/cpp/spec_grep_lines.cpp against include/aha/ac.hpp and runs it on the GPU: AC::grep_lines_batch gives the
example of the header under AHA_GREP_LINES."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def build_spec_grep_lines(tmp_path):
    exe = str(tmp_path / "spec_grep_lines")
    cmd = ["g++", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "cpp", "spec_grep_lines.cpp"), "-L", os.path.join(ROOT, "aha_amd"), "-laha_hip",
           "-Wl,-rpath," + os.path.join(ROOT, "aha_amd"), "-Wl,-rpath,/opt/rocm/lib", "-o", exe]
    subprocess.check_call(cmd)
    return exe


@pytest.mark.gpu
def test_cpp_grep_lines_spec_passes_on_gpu(tmp_path):
    exe = build_spec_grep_lines(tmp_path)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
