"""CPU: sbn_g1_small_sums without a device — the symbol is exported and a call without a context is SBN_EINVAL that writes nothing; the
constants of small_sum_kernels.cuh cover a canonical scalar and give every (term, bit of a window) its own lane; and in the SHIPPED gfx950
code object k_window_sums has no scratch segment and k_sums_to_host signals behind drained stores (the method of test_isa_product_step.py
and test_isa_handover.py)."""
import ctypes as C
import os
import re
import shutil
import subprocess
import tempfile

import pytest
from conftest import PKG_DIR

LLVM = "/opt/rocm/lib/llvm/bin"
R_MOD = 0x30644e72e131a029b85045b68181585d2833e84879b9709143e1f593f0000001


def test_the_symbol_is_exported_and_a_call_without_a_context_is_refused(sbn):
    L = sbn.lib()
    assert hasattr(L, "sbn_g1_small_sums") and "sbn_g1_small_sums" in sbn.EXPORTED_SYMBOLS
    out, inf = (C.c_uint8 * 64)(*([7] * 64)), (C.c_uint8 * 1)(7)
    one = (C.c_uint32 * 1)(1)
    assert L.sbn_g1_small_sums(None, (C.c_uint8 * 64)(), (C.c_uint8 * 32)(), one, C.c_size_t(1), out, inf) == -1      # SBN_EINVAL
    assert L.sbn_g1_small_sums(None, None, None, None, C.c_size_t(0), None, None) == -1
    assert bytes(out) == bytes([7] * 64) and bytes(inf) == b"\x07"


def test_the_windows_cover_a_canonical_scalar_and_the_lanes_cover_a_window():
    src = open(os.path.join(PKG_DIR, "csrc", "small_sum_kernels.cuh")).read()
    k = {n: int(v) for ln in src.splitlines() if ln.startswith("constexpr int ") for n, v in re.findall(r"\b(SS_[A-Z_]+) = (\d+)[,;]", ln)}
    bits, windows, terms = k["SS_WINDOW_BITS"], k["SS_WINDOWS"], k["SS_TERMS_MAX"]
    assert bits * windows >= R_MOD.bit_length() == 254
    assert bits * (windows - 1) == 252                              # window 63 holds bits 252 and 253 only
    assert terms * bits == 256                                      # __launch_bounds__(256): lane = 4 * term + bit
    assert terms >= 2 * 20 + 4                                      # 2 lg n + 4 up to PE_SIDE_MAX = 20
    assert k["SS_DESC_IDX"] >= 1 and k["SS_DESC_SCAL"] >= k["SS_DESC_IDX"] + terms
    # the kernel's sum, in integers: per window the set bits of the digit select 2^k P, the host folds sum_w 16^w S_w
    P = 0x1234567
    for s in (0, 1, 15, 16, R_MOD - 1, 1 << 251, 1 << 252, 1 << 253, (1 << 253) - 1, 3 << 252):
        S = [sum((1 << b) * P for b in range(bits) if (s >> (bits * w + b)) & 1) for w in range(windows)]
        acc = 0
        for w in reversed(range(windows)):
            acc = (acc << bits) + S[w]
        assert acc == s * P


@pytest.fixture(scope="module")
def code_object():
    so = os.path.join(PKG_DIR, "libsbn254_hip.so")
    # no skip: "no scratch segment" is a requirement of the kernel, and the tools come with the compiler that built the library
    for tool in ("llvm-objdump", "llvm-readelf"):
        assert os.path.exists(f"{LLVM}/{tool}"), f"{tool} is missing: the shipped code object cannot be checked"
    tmp = tempfile.mkdtemp(prefix="isa_ssum_")
    try:
        dst = os.path.join(tmp, "lib.so")
        shutil.copy(so, dst)
        subprocess.run([f"{LLVM}/llvm-objdump", "--offloading", dst], check=True, stdout=subprocess.DEVNULL, cwd=tmp)
        cos = [os.path.join(tmp, f) for f in os.listdir(tmp) if "gfx950" in f]
        assert cos, "no gfx950 code object in the library"
        dis = subprocess.run([f"{LLVM}/llvm-objdump", "-d", "--mcpu=gfx950", "--no-show-raw-insn", cos[0]], check=True, capture_output=True, text=True).stdout
        notes = subprocess.run([f"{LLVM}/llvm-readelf", "--notes", cos[0]], check=True, capture_output=True, text=True).stdout
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    code, cur = {}, None
    for line in dis.splitlines():
        m = re.match(r"^[0-9a-f]+ <([^>]+)>:", line)
        if m:
            cur = m.group(1)
            code[cur] = []
            continue
        if cur is not None:
            ins = line.split("//")[0].strip()
            if ins and re.match(r"^[a-z]", ins):
                code[cur].append(ins)
    meta = {}
    for rec in re.split(r"\n\s*- \.agpr_count:", notes)[1:]:
        name = re.search(r"\.name:\s+(\S+)", rec)
        if name:
            meta[name.group(1)] = {k: int(v) for k, v in re.findall(r"\.(max_flat_workgroup_size|private_segment_fixed_size|vgpr_spill_count|sgpr_spill_count|vgpr_count):\s+(\d+)", rec)}
    return code, meta


def _one(code, stem):
    names = [k for k in code if stem in k]
    assert len(names) == 1, names
    return names[0]


def test_window_sums_has_no_scratch_segment(code_object):
    code, meta = code_object
    name = _one(code, "k_window_sums")
    ins = code[name]
    assert "s_endpgm" in ins and not [i for i in ins if i.startswith("scratch_")], "k_window_sums spills"
    assert any(i.startswith("s_setprio") for i in ins[:40]), "no helper priority at the kernel's start"
    m = meta[name]
    assert m["max_flat_workgroup_size"] == 256
    assert m["private_segment_fixed_size"] == 0
    assert m.get("vgpr_spill_count", 0) == 0 and m.get("sgpr_spill_count", 0) == 0


def test_sums_to_host_raises_its_flag_behind_drained_stores(code_object):
    code, meta = code_object
    name = _one(code, "k_sums_to_host")
    ins = code[name]
    assert meta[name]["private_segment_fixed_size"] == 0
    wb = [i for i, c in enumerate(ins) if c.startswith("buffer_wbl2")]
    assert len(wb) == 1, "one release, one flag"
    flag = next(i for i in range(wb[0], len(ins)) if ins[i].startswith("global_store_dword ") and "sc0 sc1" in ins[i])
    assert any(c.startswith("s_waitcnt") and "vmcnt(0)" in c for c in ins[wb[0]:flag]), "the flag may overtake the release's write-back"
    bar = max(i for i in range(wb[0]) if ins[i] == "s_barrier")
    payload = [i for i, c in enumerate(ins) if c.startswith(("global_store_dwordx4", "flat_store_dwordx4"))]
    assert payload and max(payload) < bar, "a payload store behind the barrier"
    drain = [i for i in range(max(payload), bar) if ins[i].startswith("s_waitcnt") and "vmcnt(0)" in ins[i]]
    assert drain, "no s_waitcnt vmcnt(0) between the payload stores and the barrier"
