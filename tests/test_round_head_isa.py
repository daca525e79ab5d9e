"""ku_traverse's round -- what runs once per 16 bytes of a lane's chunk, around the trips -- read off the ISA of the build
(scan_unit.hip): an input line is requested by four loads back to back with no wait between them, the issue
priority is set only in the round that requests a line, and the round has not grown.
The counts are tripwires against a compiler that lays the round out differently, not performance claims: the measurements
are in profiles/round_head.txt, where the parent's counts (tools/isa_loop.py --round at the parent commit) stand beside them.

Not asserted: "no _f64 instruction".  The round's 64-bit clamps still go through doubles (hipcc's min<int64_t> / max<int64_t>
with an int beside them).  Integer selects in their place were built and measured twice, in two forms: 14 instructions fewer
per round and the step 0.6 and 0.7 % SLOWER than without them (2.1490 against 2.1363 ms and 2.1327 against 2.1178 ms, medians of
eight and of six alternating runs), so by the bar every part of this work was held to they are not in the tree.  They are
tools/lab/round_head_dropped.patch, which also puts that assertion and the smaller counts into this file."""
import os
import re
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNEL = "ku_traverseILb0ELi22ELb0E"  # ku_traverse<false, 22, false>: cfg 3's

# tools/isa_loop.py --round: the cheapest static way once round the round loop, outside the trip loop
ROUND_NO_LINE = 177  # the parent: 208
ROUND_LINE = 247     # the parent: 276


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


def traversals(path):
    """mangled name -> (the kernel's instructions, its metadata entry from .name on) of every ku_traverse instantiation"""
    text = open(path).read()
    src = text.splitlines()
    out = {}
    for i, t in enumerate(src):
        m = re.match(r"(_ZN\S*ku_traverseIL\S+):", t)
        if m:
            end = next(j for j in range(i, len(src)) if src[j].strip().startswith("s_endpgm"))
            at = re.search(r"\.name:\s+" + re.escape(m.group(1)) + r"\s*\n", text).end()  # (the fields of an entry are sorted by name)
            out[m.group(1)] = (src[i:end], text[at:text.index(".wavefront_size", at)])
    return out


def round_report(isa):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "isa_loop.py"), isa, KERNEL, "--round"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    return r.stdout


def test_every_instantiation_stays_in_its_budget(isa):
    ks = traversals(isa)
    assert len(ks) == 8
    for name, (body, meta) in ks.items():
        assert int(re.search(r"\.vgpr_count:\s+(\d+)", meta).group(1)) <= 128, name             # four waves per SIMD
        assert int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", meta).group(1)) == 0, name  # no scratch
        assert not [t for t in body if re.match(r"\s*scratch_", t)], name


def test_the_present_invocation_of_the_tool_still_works(isa):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "isa_loop.py"), isa, KERNEL], capture_output=True, text=True)
    assert r.returncode == 0 and re.search(r"loop instructions: \d+", r.stdout) and "round" not in r.stdout, r.stdout + r.stderr


def test_a_line_is_requested_by_four_loads_with_no_wait_between_them(isa):
    m = re.search(r"runs of four 16-byte loads in one block: (\d+) vmcnt waits inside: (\d+)", round_report(isa))
    assert m and int(m.group(1)) == 1 and int(m.group(2)) == 0, round_report(isa)


def test_the_priority_is_set_only_behind_the_line_branch(isa):
    m = re.search(r"s_setprio: (\d+) outside the round: (\d+) sides of the line branch without a load: (\d+) s_setprio on them: (\d+)",
                  round_report(isa))
    assert m and [int(x) for x in m.groups()] == [4, 0, 1, 0], round_report(isa)


def test_the_round_has_not_grown(isa):
    out = round_report(isa)
    no_line = re.search(r"no line: (\d+) instructions", out)
    line = re.search(r" line: (\d+) instructions", out[out.index("no line") + 8:])
    assert no_line and line, out
    assert int(no_line.group(1)) <= ROUND_NO_LINE and int(line.group(1)) <= ROUND_LINE, out
