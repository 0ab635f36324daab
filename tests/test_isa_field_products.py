"""CPU: what the field products of the point additions compile to, checked in the SHIPPED gfx950 code object.

A product widens its 29-bit limbs to 64 bits where it multiplies.  When the compiler shares those widened limbs across a branch (the
exact zero test of an addition's P runs a product of its own behind one), the later products no longer see that the upper halves
are zero: each limb product becomes a 64 x 64 multiply — a second `v_mad_u64_u32` or a `v_mul_lo_u32` whose factor is a register
that holds the constant 0 — and the column accumulator's halves are moved into and out of that instruction's tied operand
(fp.cuh: fe_pin32).  This file pins the result of removing that, and the register budgets the removal must respect:

  * k_acc_first<1>, k_acc_first<2>, k_acc_extra: at most 168 VGPRs (three waves per SIMD: 512 / 168 rounded up to 8) and no scratch;
  * no multiply of k_acc_first<1> / <2> has a factor register whose every write in the kernel is the constant 0 (or a copy of such
    a register);
  * k_reduce_l1, k_reduce_combine, k_reduce_combine_quad: at most 256 VGPRs and no scratch;
  * the comb kernels that had no scratch keep none.

The counting is tools/isa_stats.py's (the same functions print the table in profiles/r14_isa_field_products.txt).  No GPU needed:
llvm-objdump / llvm-readelf on the in-tree .so."""
import importlib.util
import os
import shutil

import pytest
from conftest import PKG_DIR, ROOT

ACC = ("k_acc_first<1>", "k_acc_first<2>", "k_acc_extra")
REDUCE = ("k_reduce_l1", "k_reduce_combine", "k_reduce_combine_quad")
NO_SCRATCH = ACC + REDUCE + ("k_comb_rows", "k_comb_rows_flat", "k_comb_rows_const", "k_comb_fold")


def _isa_stats():
    spec = importlib.util.spec_from_file_location("isa_stats", os.path.join(ROOT, "tools", "isa_stats.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def kernels():
    """short demangled kernel name -> (descriptor metadata, instruction counts)"""
    so = os.path.join(PKG_DIR, "libsbn254_hip.so")
    if not os.path.exists(so):
        pytest.skip("spartan-bn254_amd/libsbn254_hip.so has not been built")
    st = _isa_stats()
    if not os.path.exists(f"{st.LLVM}/llvm-objdump"):
        pytest.skip("no llvm-objdump in this image")
    tmp, co = st.extract(so)
    try:
        meta, cnt = st.metadata(co), st.disasm_counts(co)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    out = {}
    for sym, pretty in st.demangle(sorted(meta)).items():
        short = pretty.replace("void ", "", 1).split("(")[0].replace("sbn::", "")
        if sym in cnt:
            out[short] = (meta[sym], cnt[sym])
    return out


def test_kernels_found(kernels):
    for k in NO_SCRATCH:
        assert k in kernels, f"{k} missing from the code object: {sorted(kernels)[:40]}"


@pytest.mark.parametrize("name", ACC)
def test_accumulate_kernels_keep_three_waves_per_simd(kernels, name):
    meta, _ = kernels[name]
    assert meta["vgpr_count"] + meta.get("agpr_count", 0) <= 168, meta
    assert meta["private_segment_fixed_size"] == 0 and meta.get("vgpr_spill_count", 0) == 0, meta


@pytest.mark.parametrize("name", REDUCE)
def test_reduction_kernels_fit_the_register_file(kernels, name):
    meta, _ = kernels[name]
    assert meta["vgpr_count"] + meta.get("agpr_count", 0) <= 256, meta
    assert meta["private_segment_fixed_size"] == 0 and meta.get("vgpr_spill_count", 0) == 0, meta


@pytest.mark.parametrize("name", NO_SCRATCH)
def test_no_scratch(kernels, name):
    meta, cnt = kernels[name]
    assert meta["private_segment_fixed_size"] == 0 and cnt["scratch"] == 0, (meta, cnt)


@pytest.mark.parametrize("name", ACC[:2])
def test_no_multiply_by_a_constant_zero_register(kernels, name):
    _, cnt = kernels[name]
    assert cnt["v_mad_u64_u32"] > 1000 and cnt["v_mul_lo_u32"] > 50, cnt         # the products are there to be looked at
    assert cnt["zero_mul"] == 0, f"{name}: {cnt['zero_mul']} multiplies take a register that only ever holds 0 as a factor"


def test_zero_register_analysis_sees_the_pattern():
    """the analysis on the pattern itself, as the parent commit's k_acc_first had it: v25 = 0 once, v11 a copy, both used as factors"""
    st = _isa_stats()
    code = [("v_mov_b32", ["v25", "0"]), ("v_mov_b32", ["v11", "v25"]), ("v_mov_b32", ["v12", "v40"]), ("v_mov_b32", ["v13", "0"]), ("v_add_u32", ["v13", "v13", "v1"]),
            ("v_mad_u64_u32", ["v[14:15]", "s[26:27]", "v12", "v12", "v[14:15]"]), ("v_mul_lo_u32", ["v110", "v12", "v25"]),
            ("v_mad_u64_u32", ["v[112:113]", "s[26:27]", "v11", "v114", "v[112:113]"]), ("v_mad_u64_u32", ["v[112:113]", "s[26:27]", "v13", "v114", "v[112:113]"])]
    assert st.zero_registers(code) == {25, 11}
    assert st.regs("v[4:6]") == [4, 5, 6] and st.regs("s[26:27]") == [] and st.regs("0") == []
