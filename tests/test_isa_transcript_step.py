"""CPU: the transcript step kernel of sbn_sumcheck_prove in the SHIPPED gfx950 code object (same method as test_isa_handover.py).

The step takes no part in a hand-over inside a launch: it reads the round kernel's sums and writes r_j for the next launch, and both
orderings are the stream's (kernel boundaries).  So it must contain no signal at all — no ticket add, no release write-back, no
write-through flag store — and the round kernels' device-memory-challenge variants, which keep their hand-over, must be in the
library under the stems test_isa_handover.py checks."""
import os
import re
import shutil
import subprocess
import tempfile

import pytest
from conftest import PKG_DIR

LLVM = "/opt/rocm/lib/llvm/bin"


@pytest.fixture(scope="module")
def kernels():
    so = os.path.join(PKG_DIR, "libsbn254_hip.so")
    if not os.path.exists(f"{LLVM}/llvm-objdump"):
        pytest.skip("no llvm-objdump in this image")
    tmp = tempfile.mkdtemp(prefix="isa_step_")
    try:
        dst = os.path.join(tmp, "lib.so")
        shutil.copy(so, dst)
        subprocess.run([f"{LLVM}/llvm-objdump", "--offloading", dst], check=True, stdout=subprocess.DEVNULL, cwd=tmp)
        cos = [os.path.join(tmp, f) for f in os.listdir(tmp) if "gfx950" in f]
        assert cos, "no gfx950 code object in the library"
        txt = subprocess.run([f"{LLVM}/llvm-objdump", "-d", "--mcpu=gfx950", "--no-show-raw-insn", cos[0]], check=True, capture_output=True, text=True).stdout
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    out, cur = {}, None
    for line in txt.splitlines():
        m = re.match(r"^[0-9a-f]+ <([^>]+)>:", line)
        if m:
            cur = m.group(1)
            out[cur] = []
            continue
        if cur is not None:
            ins = line.split("//")[0].strip()
            if ins and re.match(r"^[a-z]", ins):
                out[cur].append(ins)
    return out


def test_step_kernel_signals_nothing(kernels):
    names = [k for k in kernels if "k_tr_sumcheck_step" in k]
    assert len(names) == 1, names
    code = kernels[names[0]]
    assert len(code) > 1000 and "s_endpgm" in code
    for ins in code:
        assert not ins.startswith(("global_atomic", "flat_atomic", "buffer_atomic")), ins
        assert not ins.startswith(("buffer_wbl2", "buffer_inv")), ins
        assert not (ins.startswith(("global_store", "flat_store")) and "sc1" in ins), f"write-through store in the step: {ins}"
        assert not ins.startswith("scratch_"), f"the step spills: {ins}"
    assert sum(1 for ins in code if ins.startswith("ds_bpermute_b32")) >= 18 * 2      # the lane-parallel Keccak round, per block


def test_device_challenge_variants_are_checked_by_the_handover_test(kernels):
    names = " ".join(kernels)
    for frag in ("k_sc_bind_evalILi0ELi2ENS_11ScScalarDevE", "k_sc_bind_eval_tinyILi0ENS_11ScScalarDevE", "k_sc_bind_eval_pfILi0ENS_11ScScalarDevE",
                 "k_sc_comb_bind_evalILb0ENS_11ScScalarDevE", "k_sc_comb_bind_evalILb1ENS_11ScScalarDevE", "k_sc_round_mixedILb0ENS_11ScScalarDevE",
                 "k_sc_round_mixedILb1ENS_11ScScalarDevE"):
        assert frag in names, f"{frag} missing from the code object"
        assert re.search(r"k_sc_(eval|bind_eval|comb_eval|comb_bind_eval|round_mixed|finals)", frag)
