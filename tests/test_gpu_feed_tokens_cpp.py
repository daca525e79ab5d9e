"""Builds tests/cpp/spec_feed_tokens.cpp against include/aha/ac.hpp and runs it on the GPU: Feed::tokens_batch and Feed::tokens
on the header's four examples, call by call, mixing, and the stream laws in both gap modes."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def build_spec_feed_tokens(tmp_path):
    exe = str(tmp_path / "spec_feed_tokens")
    cmd = ["g++", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "cpp", "spec_feed_tokens.cpp"), "-L", os.path.join(ROOT, "aha_amd"), "-laha_hip",
           "-Wl,-rpath," + os.path.join(ROOT, "aha_amd"), "-Wl,-rpath,/opt/rocm/lib", "-o", exe]
    subprocess.check_call(cmd)
    return exe


def test_cpp_feed_tokens_spec_compiles(tmp_path):
    assert os.path.exists(build_spec_feed_tokens(tmp_path))


@pytest.mark.gpu
def test_cpp_feed_tokens_spec_passes_on_gpu(tmp_path):
    exe = build_spec_feed_tokens(tmp_path)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
