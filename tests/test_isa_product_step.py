"""CPU: the layer-boundary step kernel of sbn_product_proof_prove in the SHIPPED gfx950 code object (same method as
test_isa_transcript_step.py): one wavefront per workgroup, no scratch memory (nothing spills, no private segment)."""
import os
import re
import shutil
import subprocess
import tempfile

import pytest
from conftest import PKG_DIR

LLVM = "/opt/rocm/lib/llvm/bin"
STEPS = ["k_tr_layer_step"]


@pytest.fixture(scope="module")
def code_object():
    so = os.path.join(PKG_DIR, "libsbn254_hip.so")
    if not os.path.exists(f"{LLVM}/llvm-objdump") or not os.path.exists(f"{LLVM}/llvm-readelf"):
        pytest.skip("no llvm-objdump / llvm-readelf in this image")
    tmp = tempfile.mkdtemp(prefix="isa_pstep_")
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
    # the kernels' metadata records: "- .agpr_count: ..." up to the next record, keyed by .name
    meta = {}
    for rec in re.split(r"\n\s*- \.agpr_count:", notes)[1:]:
        name = re.search(r"\.name:\s+(\S+)", rec)
        if name:
            meta[name.group(1)] = {k: int(v) for k, v in re.findall(r"\.(max_flat_workgroup_size|private_segment_fixed_size|vgpr_spill_count|sgpr_spill_count):\s+(\d+)", rec)}
    return code, meta


@pytest.mark.parametrize("stem", STEPS)
def test_step_is_one_wave_without_scratch(code_object, stem):
    code, meta = code_object
    names = [k for k in code if stem in k]
    assert len(names) == 1, names
    ins = code[names[0]]
    assert len(ins) > 1000 and "s_endpgm" in ins
    assert not [i for i in ins if i.startswith("scratch_")], "the step spills"
    assert sum(1 for i in ins if i.startswith("ds_bpermute_b32")) >= 18      # the lane-parallel Keccak round
    m = meta[names[0]]
    assert m["max_flat_workgroup_size"] == 64
    assert m["private_segment_fixed_size"] == 0
    assert m.get("vgpr_spill_count", 0) == 0 and m.get("sgpr_spill_count", 0) == 0
