"""tools/audit_probe.py on hand-written ISA: ku_traverse's probe sits behind an exec mask that is set and put back inside
the asm statement (only the probing lanes ask memory for something), so the audit has to find a hand-issued load anywhere
inside a statement and to check that the statement leaves exec as it found it."""
import importlib.util
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def ap():
    spec = importlib.util.spec_from_file_location("audit_probe", os.path.join(ROOT, "tools", "audit_probe.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def block(*body):
    return "\t;;#ASMSTART\n" + "".join("\t%s\n" % t for t in body) + "\t;;#ASMEND\n"


LOAD = "global_load_dwordx2 v[70:71], v[92:93], off"
MASKED = block("s_and_saveexec_b64 s[14:15], s[90:91]", LOAD, "s_mov_b64 exec, s[14:15]")
WAIT = block("s_waitcnt vmcnt(0)")
WORK = "\tv_add_u32_e32 v20, v75, v66\n\tds_read2_b32 v[90:91], v90 offset1:1\n"
USE = "\tv_bfe_u32 v93, v70, v89, 1\n"


def test_a_masked_block_passes(ap):
    assert ap.audit(MASKED + WORK + WAIT + USE) == (1, [])
    # ... exec saved by a plain move, and two loads under two masks in one statement (the header beside the probe)
    two = block("s_mov_b64 s[14:15], exec", "s_mov_b64 exec, s[90:91]", LOAD, "s_mov_b64 exec, s[88:89]",
                "global_load_dword v72, v[94:95], off", "s_mov_b64 exec, s[14:15]")
    assert ap.audit(two + WORK + WAIT + USE + "\tv_mov_b32_e32 v1, v72\n") == (2, [])


def test_a_block_that_leaves_exec_changed_fails(ap):
    for body in ((("s_and_saveexec_b64 s[14:15], s[90:91]", LOAD)),                                  # never put back
                 (("s_and_saveexec_b64 s[14:15], s[90:91]", LOAD, "s_mov_b64 exec, s[16:17]")),      # ... from another pair
                 (("s_mov_b64 exec, s[90:91]", LOAD, "s_mov_b64 exec, s[14:15]")),                   # never saved
                 (("s_and_saveexec_b64 s[14:15], s[90:91]", LOAD, "s_mov_b64 s[14:15], s[2:3]", "s_mov_b64 exec, s[14:15]")),
                 (("s_and_saveexec_b64 s[14:15], s[90:91]", LOAD, "s_mov_b64 exec, s[14:15]", "s_mov_b64 exec, s[90:91]"))):
        n, bad = ap.audit(block(*body) + WORK + WAIT + USE)
        assert n == 1 and bad and any("exec" in t for _, t in bad), (body, bad)


def test_a_read_of_the_destination_between_load_and_wait_fails(ap):
    n, bad = ap.audit(MASKED + WORK + USE + WAIT)
    assert n == 1 and len(bad) == 1 and "v70" in bad[0][1]
    n, bad = ap.audit(MASKED + "\tv_mov_b64_e32 v[16:17], v[70:71]\n" + WAIT)  # (a copy of the pair)
    assert n == 1 and len(bad) == 1
    # ... inside the statement itself, behind the load
    n, bad = ap.audit(block("s_and_saveexec_b64 s[14:15], s[90:91]", LOAD, "v_mov_b32_e32 v1, v71", "s_mov_b64 exec, s[14:15]") + WAIT)
    assert n == 1 and len(bad) == 1 and "v71" in bad[0][1]
    # ... and a load that is not the statement's first instruction is found at all: without a wait behind it, that is said
    n, bad = ap.audit(MASKED + WORK)
    assert n == 1 and len(bad) == 1 and "no hand-written wait" in bad[0][1]
