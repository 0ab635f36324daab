"""CPU: the column-wise field product (fp.cuh: fe_mulu_cols) as it compiles, checked in the SHIPPED gfx950 code object.

The word-serial product adds every column's carry into a column that already holds a partial sum: 17 64-bit additions (v_lshl_add_u64)
per 162 multiply-adds, 17.5 over the whole accumulate kernel.  The column-wise product visits the columns in order with one
accumulator that starts as the carry, so the carry is the next v_mad_u64_u32's 64-bit addend and 1 addition per product is left.
The compiler undoes this (it reassociates the sums back, instruction for instruction) unless every partial sum is pinned
(fp.cuh: fe_pin64); this file pins the result in k_acc_first<1> and <2>: at most 6 64-bit additions per 162 v_mad_u64_u32.

The parent has 590 / 593 additions for 5 638 v_mad_u64_u32 (17.0 per 162).  With the unsigned products by columns alone the kernels
still had 302 / 305 (8.7): 270 of them belonged to the 18 SIGNED, word-serial products of the two inlined rare paths (xyzz_dbl_affine
7, the two exact zero tests 1 each, per addition).  The signed product cannot go by columns (k_comb_build, k_scale_points and
k_mul_generator go to 512 VGPRs and 6.5 - 7.6 KB of scratch with it: profiles/r18_isa_column_products.txt); instead six of
xyzz_dbl_affine's seven products, whose operands are never negative, are the unsigned products (g1.cuh), which return the same limbs.

The register and scratch limits are those of tests/test_isa_field_products.py.  The counting is tools/isa_stats.py's (the same
functions print profiles/r18_isa_column_products.txt).  No GPU needed: llvm-objdump / llvm-readelf on the in-tree .so."""
import importlib.util
import os
import shutil

import pytest
from conftest import PKG_DIR, ROOT

ACC = ("k_acc_first<1>", "k_acc_first<2>")


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


@pytest.mark.parametrize("name", ACC)
def test_carry_rides_in_the_multiply_add(kernels, name):
    _, cnt = kernels[name]
    assert cnt["v_mad_u64_u32"] > 1000, cnt                                          # the products are there to be looked at
    per_product = cnt["add64"] * 162.0 / cnt["v_mad_u64_u32"]
    print(f"{name}: {cnt['add64']} 64-bit additions, {cnt['v_mad_u64_u32']} v_mad_u64_u32: {per_product:.2f} per 162; s_nop {cnt['s_nop']}")
    assert per_product <= 6.0, f"{name}: {cnt['add64']} 64-bit additions for {cnt['v_mad_u64_u32']} v_mad_u64_u32 ({per_product:.1f} per 162)"


@pytest.mark.parametrize("name", ACC)
def test_register_and_scratch_limits_hold(kernels, name):
    meta, cnt = kernels[name]
    assert meta["vgpr_count"] + meta.get("agpr_count", 0) <= 168, meta               # three waves per SIMD
    assert meta["private_segment_fixed_size"] == 0 and meta.get("vgpr_spill_count", 0) == 0 and cnt["scratch"] == 0, (meta, cnt)


def test_counter_sees_both_forms_of_a_64_bit_addition(tmp_path):
    """the counting on a listing with one v_lshl_add_u64 and one carry-chained pair"""
    st = _isa_stats()
    listing = "\n".join(["0000000000001000 <k>:", "\tv_mad_u64_u32 v[0:1], s[2:3], v4, v5, v[0:1]", "\tv_lshl_add_u64 v[2:3], v[0:1], 0, v[2:3]",
                         "\tv_add_co_u32_e32 v6, vcc, v6, v8", "\tv_addc_co_u32_e32 v7, vcc, v7, v9, vcc", "\ts_nop 0", "\ts_endpgm", ""])
    fake = tmp_path / "objdump"
    fake.mkdir()
    exe = fake / "llvm-objdump"
    exe.write_text("#!/bin/sh\ncat <<'EOF'\n" + listing + "EOF\n")
    exe.chmod(0o755)
    old = st.LLVM
    st.LLVM = str(fake)
    try:
        cnt = st.disasm_counts("unused")
    finally:
        st.LLVM = old
    assert cnt["k"]["add64"] == 2 and cnt["k"]["v_mad_u64_u32"] == 1 and cnt["k"]["s_nop"] == 1 and cnt["k"]["other_valu"] == 3, cnt
