#!/usr/bin/env python3
"""ISA accounting of the shipped gfx950 code object: per kernel, the instruction mix that prices the field arithmetic.

    python tools/isa_stats.py [--so spartan-bn254_amd/libsbn254_hip.so | --co device.o] [--kernels k_acc_first,k_comb_rows,...] [--json out.json]

Extracts the gfx950 code object from the .so (llvm-objdump --offloading), reads the kernel descriptors' metadata
(llvm-readelf --notes: VGPRs, SGPRs, scratch, LDS) and disassembles it (llvm-objdump -d --mcpu=gfx950), then counts per kernel:
  v_mad_u64_u32   (+ v_mad_i64_i32) the only wide multiplier of the CDNA4 VALU: 4.2 cycles per wave-instruction (tools/micro/ibench.hip)
  v_mul_lo_u32    the Montgomery quotient digits (4.2)
  other VALU      shifts, masks, limb additions, selects, moves: 2.3 cycles for plain VOP2 forms, 4.2 for VOP3 / 64-bit / carry forms
  add64           64-bit additions among them: v_lshl_add_u64, plus the carry-chained pairs v_add_co_u32 + v_addc_co_u32 (counted once, at the
                  v_addc_co_u32).  The word-serial field product has 17 per 162 multiply-adds (a column's carry is added into a partial
                  sum); the column-wise product (fp.cuh: fe_mulu_cols) has 1, because the carry rides as the next multiply-add's addend
  v_mov           the v_mov_b32 among them (register-to-register copies and constants: work no formula asks for)
  mov>mad         v_mov_b32 straight into the destination pair of the v_mad_u64_u32 that follows it: a 64-bit column whose halves
                  the register allocator did not keep adjacent is shuffled into the multiply-add's tied operand and out again
  zero*           multiplies (v_mad_u64_u32 / v_mad_i64_i32 / v_mul_lo_u32) with a factor register that only ever holds the constant 0
                  (every write to it is `v_mov_b32 r, 0` or a copy of such a register): a 64 x 64 product of a zero-extended limb
  s_nop           padding the compiler inserts for a hazard (e.g. before a VALU instruction that reads a register an inline asm has as an output)
  SALU, VMEM (global/buffer/scratch), LDS, waitcnt
and prices them roughly: cycles ~ 4.2 * (mad + mul_lo) + 3 * other VALU; `mult_share` = the multiplier's part of that (1.0 = nothing
but products).  Needs no GPU (runs on the build machine)."""
import argparse
import json
import os
import re
import shutil
import subprocess
import sys
import tempfile

LLVM = "/opt/rocm/lib/llvm/bin"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAD_CYC, VALU_CYC = 4.2, 3.0


def extract(so):
    tmp = tempfile.mkdtemp(prefix="isa_")
    dst = os.path.join(tmp, os.path.basename(so))
    shutil.copy(so, dst)
    subprocess.run([f"{LLVM}/llvm-objdump", "--offloading", dst], check=True, stdout=subprocess.DEVNULL, cwd=tmp)
    cos = [os.path.join(tmp, f) for f in os.listdir(tmp) if "gfx950" in f]
    if not cos:
        raise SystemExit(f"no gfx950 code object inside {so}")
    return tmp, cos[0]


def metadata(co):
    """kernel symbol -> descriptor metadata.  A kernel's record in the amdhsa.kernels list starts at its first key (`- .agpr_count:`) and
    its keys come in alphabetical order, so .symbol precedes .vgpr_count: records are closed at the next record's start."""
    txt = subprocess.run([f"{LLVM}/llvm-readelf", "--notes", co], check=True, capture_output=True, text=True).stdout
    out = {}
    cur = None
    keep = ("vgpr_count", "sgpr_count", "agpr_count", "private_segment_fixed_size", "group_segment_fixed_size", "vgpr_spill_count", "sgpr_spill_count", "max_flat_workgroup_size")

    def flush():
        if cur and cur.get("symbol", "").endswith(".kd"):
            out[cur["symbol"][:-3]] = cur

    for line in txt.splitlines():
        m = re.match(r"^(\s*)(- )?\.(\w+):\s*(.*)$", line)
        if not m:
            continue
        dash, k, v = m.group(2), m.group(3), m.group(4).strip()
        if dash and k == "agpr_count":
            flush()
            cur = {}
        if cur is None:
            continue
        if k in keep:
            cur[k] = int(v)
        elif k == "symbol":
            cur["symbol"] = v.strip("'\"")
    flush()
    return out


def demangle(names):
    p = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True)
    d = p.stdout.splitlines() if p.returncode == 0 else names
    return dict(zip(names, d))


def regs(tok):
    """VGPR numbers named by one operand token: v7 -> [7], v[4:5] -> [4, 5], anything else -> []"""
    m = re.fullmatch(r"v(\d+)", tok)
    if m:
        return [int(m.group(1))]
    m = re.fullmatch(r"v\[(\d+):(\d+)\]", tok)
    if m:
        return list(range(int(m.group(1)), int(m.group(2)) + 1))
    return []


def operands(line):
    t = line.split("//")[0].strip().split(None, 1)
    if len(t) < 2:
        return []
    return [x.strip() for x in t[1].split(",")]


MULS = ("v_mad_u64_u32", "v_mad_i64_i32", "v_mul_lo_u32")


def zero_registers(code):
    """VGPRs that hold nothing but the constant 0 in this kernel.  code: [(op, operands)].  Every VALU / memory instruction's
    first operand is taken as its destination (v_swap_b32 and v_readlane do not occur in these kernels' products); a register is
    zero if each of its writes is `v_mov_b32 r, 0` or `v_mov_b32 r, z` with z zero (fixpoint, starting from all candidates)."""
    writes = {}
    for op, ops in code:
        if not ops or not op.startswith(("v_", "global_load", "flat_load", "buffer_load", "scratch_load", "ds_read", "ds_bpermute", "ds_permute", "ds_swizzle")):
            continue
        if op.startswith(("v_cmp", "v_cmpx", "v_readlane", "v_readfirstlane", "v_nop")):
            continue
        dsts = list(ops[:1]) + (list(ops[1:2]) if op == "v_swap_b32" else [])
        for d in dsts:
            for r in regs(d):
                writes.setdefault(r, []).append((op, ops[1] if len(ops) > 1 else ""))
    zero = {r for r, w in writes.items() if all(o == "v_mov_b32" and (s == "0" or regs(s)) for o, s in w)}
    while True:
        drop = {r for r in zero if any(s != "0" and not (regs(s) and regs(s)[0] in zero) for _, s in writes[r])}
        if not drop:
            return zero
        zero -= drop


def disasm_counts(co):
    p = subprocess.Popen([f"{LLVM}/llvm-objdump", "-d", "--mcpu=gfx950", "--no-show-raw-insn", co], stdout=subprocess.PIPE, text=True)
    counts = {}
    code = {}
    cur = None
    for line in p.stdout:
        m = re.match(r"^[0-9a-f]+ <([^>]+)>:", line)
        if m:
            cur = m.group(1)
            counts[cur] = {"total": 0, "v_mad_u64_u32": 0, "v_mul_lo_u32": 0, "other_valu": 0, "add64": 0, "v_mov": 0, "mov_mad": 0, "zero_mul": 0, "s_nop": 0, "salu": 0, "vmem": 0, "scratch": 0, "lds": 0, "waitcnt": 0}
            code[cur] = []
            continue
        if cur is None:
            continue
        t = line.strip().split()
        if not t:
            continue
        op = t[0]
        if not re.match(r"^[a-z]", op) or op.startswith("//"):
            continue
        op = re.sub(r"_e(32|64)$", "", op)                      # the disassembler's encoding suffix
        code[cur].append((op, operands(line)))
        c = counts[cur]
        c["total"] += 1
        if op in ("v_mad_u64_u32", "v_mad_i64_i32"):          # the wide multiplier, unsigned and signed form
            c["v_mad_u64_u32"] += 1
        elif op == "v_mul_lo_u32":
            c["v_mul_lo_u32"] += 1
        elif op.startswith("v_"):
            c["other_valu"] += 1
            if op == "v_mov_b32":
                c["v_mov"] += 1
            elif op in ("v_lshl_add_u64", "v_addc_co_u32"):
                c["add64"] += 1
        elif op == "s_nop":
            c["s_nop"] += 1
        elif op == "s_waitcnt":
            c["waitcnt"] += 1
        elif op.startswith("scratch_"):
            c["scratch"] += 1
        elif op.startswith(("global_", "buffer_", "flat_")):
            c["vmem"] += 1
        elif op.startswith("ds_"):
            c["lds"] += 1
        elif op.startswith("s_"):
            c["salu"] += 1
    p.wait()
    for name, ins in code.items():
        c = counts[name]
        for (op, ops), (nop, nops) in zip(ins, ins[1:]):
            if op == "v_mov_b32" and nop == "v_mad_u64_u32" and ops and nops and regs(ops[0]) and regs(ops[0])[0] in regs(nops[0]):
                c["mov_mad"] += 1
        zero = zero_registers(ins)
        for op, ops in ins:
            if op in MULS:
                fac = ops[2:4] if op != "v_mul_lo_u32" else ops[1:3]      # v_mad: vdst, sdst, src0, src1, src2
                if any(regs(f) and regs(f)[0] in zero for f in fac):
                    c["zero_mul"] += 1
    return counts


def waves_per_simd(vgprs):
    alloc = -(-max(vgprs, 1) // 8) * 8
    return min(8, 512 // alloc)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--so", default=os.path.join(ROOT, "spartan-bn254_amd", "libsbn254_hip.so"))
    ap.add_argument("--kernels", default="k_acc_first,k_acc_extra,k_comb_rows,k_reduce_l1,k_reduce_combine,k_sc_eval,k_sc_bind_eval,k_sc_round,k_bind_top,k_dot,k_digits_store,k_sort_rows,k_scatter_lds",
                    help="comma-separated substrings of the (demangled) kernel names to report; 'all' for every kernel")
    ap.add_argument("--co", default=None, help="a gfx950 code object (a device-only compile) instead of the library")
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    tmp, co = (None, args.co) if args.co else extract(args.so)
    try:
        meta = metadata(co)
        cnt = disasm_counts(co)
    finally:
        if tmp:
            shutil.rmtree(tmp, ignore_errors=True)
    names = sorted(meta.keys())
    dm = demangle(names)
    want = None if args.kernels == "all" else [w for w in args.kernels.split(",") if w]
    rows = []
    for n in names:
        pretty = re.sub(r"^void ", "", dm.get(n, n))
        short = re.sub(r"\(.*$", "", pretty)
        if want and not any(w in short for w in want):
            continue
        c = cnt.get(n)
        if not c:
            continue
        m = meta[n]
        mult = c["v_mad_u64_u32"] + c["v_mul_lo_u32"]
        cyc_mult = MAD_CYC * mult
        cyc_other = VALU_CYC * c["other_valu"]
        rows.append({"kernel": short, "vgpr": m.get("vgpr_count"), "agpr": m.get("agpr_count", 0), "sgpr": m.get("sgpr_count"), "scratch_B": m.get("private_segment_fixed_size"),
                     "lds_B": m.get("group_segment_fixed_size"), "waves_per_simd": waves_per_simd((m.get("vgpr_count") or 0) + (m.get("agpr_count") or 0)),
                     **c, "mult_share": round(cyc_mult / (cyc_mult + cyc_other), 3) if (cyc_mult + cyc_other) else None,
                     "products_equiv": round(c["v_mad_u64_u32"] / 162.0, 1)})
    hdr = f"{'kernel':44s} {'vgpr':>4s} {'w/S':>3s} {'scr':>4s} {'instr':>6s} {'mad64':>6s} {'mullo':>5s} {'oVALU':>6s} {'add64':>5s} {'v_mov':>5s} {'mov>mad':>7s} {'zero*':>5s} {'s_nop':>5s} {'vmem':>4s} {'lds':>4s} {'mult%':>6s}"
    print(hdr)
    for r in rows:
        print(f"{r['kernel'][:44]:44s} {r['vgpr']:4d} {r['waves_per_simd']:3d} {r['scratch_B']:4d} {r['total']:6d} {r['v_mad_u64_u32']:6d} {r['v_mul_lo_u32']:5d} {r['other_valu']:6d} {r['add64']:5d} {r['v_mov']:5d} {r['mov_mad']:7d} {r['zero_mul']:5d} {r['s_nop']:5d} {r['vmem'] + r['scratch']:4d} {r['lds']:4d} {100 * (r['mult_share'] or 0):6.1f}")
    if args.json:
        json.dump(rows, open(args.json, "w"), indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
