"""Builds tests/cpp/spec_feed_sep.cpp against include/aha/ac.hpp and runs it on the GPU: a Feed opened with a BitArray reports
whole-word hits one byte late at every cut, finish ends a sequence, count equals match, cover and select are refused.  (That it
compiles is checked without a GPU by tests/test_feed_sep_host.py.)"""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def build_spec_feed_sep(tmp_path):
    exe = str(tmp_path / "spec_feed_sep")
    cmd = ["g++", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "cpp", "spec_feed_sep.cpp"), "-L", os.path.join(ROOT, "aha_amd"), "-laha_hip",
           "-Wl,-rpath," + os.path.join(ROOT, "aha_amd"), "-Wl,-rpath,/opt/rocm/lib", "-o", exe]
    subprocess.check_call(cmd)
    return exe


@pytest.mark.gpu
def test_cpp_feed_sep_spec_passes_on_gpu(tmp_path):
    exe = build_spec_feed_sep(tmp_path)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
