"""ku_traverse's chain from one probe to the next, read off the ISA of the build (scan_unit.hip): what the
trip computes in the probe's shadow must stay in front of the hand-written wait.  The numbers are tripwires against a
compiler that sinks the hoisted code back behind the wait or grows the loop, not performance claims: the measurements are
in profiles/trip_chain.txt."""
import importlib.util
import os
import re
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNEL = "ku_traverseILb0ELi22ELb0E"  # ku_traverse<false, 22, false>: cfg 3's


def makefile_flags():
    for line in open(os.path.join(ROOT, "aha_amd", "csrc", "Makefile")):
        m = re.match(r"CXXFLAGS\s*\?=\s*(.*)", line)
        if m:
            return m.group(1).split()
    raise AssertionError("no CXXFLAGS in the Makefile")


@pytest.fixture(scope="module")
def isa(tmp_path_factory):
    """scan_unit.hip as ISA, compiled with the flags of the build"""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not (os.path.exists(hipcc) or shutil.which(hipcc)):
        pytest.skip("no hipcc")
    out = str(tmp_path_factory.mktemp("isa") / "scan_unit.s")
    subprocess.check_call([hipcc, *makefile_flags(), "--offload-arch=gfx950", "-I", os.path.join(ROOT, "include"), "-I",
                           os.path.join(ROOT, "aha_amd", "csrc"), "-S", "--cuda-device-only", "-w", "-o", out,
                           os.path.join(ROOT, "aha_amd", "csrc", "scan_unit.hip")])
    return out


def kernel_lines(path):
    src = open(path).read().splitlines()
    start = next(i for i, t in enumerate(src) if re.match(r"_ZN\S+:", t) and KERNEL in t)
    end = next(i for i in range(start, len(src)) if src[i].strip().startswith("s_endpgm"))
    return src[start:end]


def test_the_audit_passes_on_the_built_sources(isa):
    """The stretch between the probe's issue and its wait has grown: nothing in it may touch the probe's destination."""
    spec = importlib.util.spec_from_file_location("audit_probe", os.path.join(ROOT, "tools", "audit_probe.py"))
    ap = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ap)
    text = open(isa).read()
    seen, bad = ap.audit(text)
    assert seen == 12  # eight instantiations, four of them with the header's load beside the probe
    assert bad + ap.sgpr_hazards(text) + ap.store_data_hazards(text) == []


def test_the_trip_loop_has_not_grown(isa):
    """tools/isa_loop.py on ku_traverse<false,22,false>: no more instructions than before the hoist (165)."""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "isa_loop.py"), isa, KERNEL], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    m = re.search(r"loop instructions: (\d+)", r.stdout)
    assert m and int(m.group(1)) <= 165, r.stdout


def test_what_is_left_behind_the_wait(isa):
    """From the hand-written wait to the end of the active lanes' block -- the resolve: the probe's answer picks among values
    that are ready.  46 instructions before the hoist, 27 with it."""
    fn = kernel_lines(isa)
    w = next(i for i, t in enumerate(fn) if "s_waitcnt vmcnt(0)" in t and "#ASMSTART" in fn[i - 1])
    assert "#ASMEND" in fn[w + 1]
    n = 0
    for t in fn[w + 2:]:
        body = t.split(";")[0].strip()
        if re.match(r"s_or_b64\s+exec,", body):
            break
        assert not re.match(r"(s_cbranch|s_branch|global_|ds_)", body), body  # one straight block without memory instructions
        if body and not body.endswith(":") and not body.startswith("."):
            n += 1
    assert 0 < n <= 27, n
