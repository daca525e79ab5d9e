"""Builds tests/cpp/spec_post_common.hip -- every helper of aha_amd/csrc/post_common.hpp in a tiny kernel, against plain host
loops -- for gfx950; on a GPU it is run as well."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def build_spec_post_common(tmp_path):
    makefile = open(os.path.join(ROOT, "aha_amd", "csrc", "Makefile")).read()
    hipcc = os.environ.get("HIPCC") or re.search(r"^HIPCC \?= (\S+)", makefile, re.M).group(1)
    exe = str(tmp_path / "spec_post_common")
    subprocess.check_call([hipcc, "-O2", "-std=c++17", "-Wall", "--offload-arch=gfx950",
                           os.path.join(ROOT, "tests", "cpp", "spec_post_common.hip"), "-o", exe])
    return exe


def test_cpp_post_common_spec_builds_for_gfx950(tmp_path):
    assert os.path.getsize(build_spec_post_common(tmp_path)) > 0


@pytest.mark.gpu
def test_cpp_post_common_spec_passes_on_gpu(tmp_path):
    exe = build_spec_post_common(tmp_path)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
