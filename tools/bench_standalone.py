#!/usr/bin/env python3
"""The circuit digest at the keyless shape on one MI355X: the leaf kernel alone, the whole sbn_circom_r1cs_digest call (launch, the leaves brought back,
the root on the host), and the alternative it replaces — hashlib.shake_256 over the same .r1cs file's bytes on one host core.

    python tools/bench_standalone.py [--log 20] [--passes 7] [--out profiles/r29_standalone.txt]

The file is the synthetic keyless-shaped circuit of tools/bench_circom.py, written in memory.  The two hashes are not the same function (the digest is
defined over the parsed entries, not the file's bytes): the host figure is what a caller without this call would pay to bind a proof to its circuit at
all.  No time is gated; the figures are written down as they come.  The prover's RandomTape and draw plan for the same shape are timed too (host only), and sbn_spartan's
encode, prove and verify run once each on the same file as child processes: their own stage lines are recorded."""
import argparse
import hashlib
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from __graft_entry__ import load_pkg  # noqa: E402
import bench_circom as bc  # noqa: E402


def cli_stages(np, rm, rng, data, num_vars):
    """sbn_spartan prove and verify on the same file, one child at a time, after this process has closed its context: the stage lines each child prints.
    The witness is random (the synthetic circuit has none that satisfies it): prove runs without --check-sat and proves what it is given, verify then
    refuses, and its stage times are those of a whole check of the R1CS proof's first half at least.  A child that fails is reported, not retried"""
    import subprocess
    import tempfile
    exe = os.path.join(ROOT, "spartan-bn254_amd", "sbn_spartan")
    out = []
    with tempfile.TemporaryDirectory() as d:
        r1, wt, pf = (os.path.join(d, x) for x in ("c.r1cs", "w.wtns", "p.sbnp"))
        data.tofile(r1)
        vals = rm.random_vals(rng, 1 + bc.NUM_INPUTS + num_vars).reshape(-1, 32)
        vals[0] = 0; vals[0, 0] = 1                                                      # wire 0 is the constant one
        le = lambda x, k: int(x).to_bytes(k, "little")                                   # noqa: E731
        with open(wt, "wb") as fh:
            fh.write(b"wtns" + le(2, 4) + le(2, 4) + le(1, 4) + le(40, 8) + le(32, 4) + le(bc.R, 32) + le(len(vals), 4) + le(2, 4) + le(32 * len(vals), 8))
            fh.write(vals.tobytes())
        for mode, target in (("nizk", r1), ("snark", None)):
            cmds = [("prove", [exe, "prove", "--mode", mode, r1, wt, "-o", pf])]
            if mode == "snark":
                target = os.path.join(d, "c.comm")
                cmds.insert(0, ("encode", [exe, "encode", r1, "-o", target]))
            cmds.append(("verify", [exe, "verify", "--mode", mode, target, pf]))
            for what, cmd in cmds:
                try:
                    r = subprocess.run(cmd, capture_output=True, text=True, timeout=240)
                except subprocess.TimeoutExpired:
                    return out + [f"sbn_spartan {what} --mode {mode}: ran into its 240 s limit; the stages behind it: not measured"]
                if r.returncode not in (0, 1):
                    return out + [f"sbn_spartan {what} --mode {mode}: status {r.returncode}: {r.stderr.strip()[-300:]}; the stages behind it: not measured"]
                out.append(f"sbn_spartan {what} --mode {mode} (status {r.returncode}; wall times of one run, a fresh process and context each):")
                out += ["    " + ln for ln in r.stdout.splitlines() if ln.startswith(("stage ", "proof "))]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log", type=int, default=20, help="20: the keyless shape as it is; smaller: the same recipe scaled down (a quick look, not a figure)")
    ap.add_argument("--passes", type=int, default=7)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import numpy as np
    import r1cs_model as rm
    sbn = load_pkg()
    rng = np.random.default_rng(25)
    if a.log == rm.KEYLESS_LOG:
        n, _, mats = rm.keyless_instance()
        real = rm.KEYLESS_REAL_ROWS
    else:
        n = 1 << a.log; real = n - n // 128
        mats = [(rng.integers(0, real, k * n, dtype=np.uint32), rng.integers(0, 2 * n, k * n, dtype=np.uint32), rm.random_vals(rng, k * n)) for k in (3, 1, 2)]
    live = n + 1 + bc.NUM_INPUTS
    mats = [(r, np.where(c >= live, c - live, c).astype(np.uint32), v) for r, c, v in mats]
    data = bc.write_r1cs(np, real, n, bc.NUM_INPUTS, mats)
    lines = [f"circuit: {real} constraints x {n} variables, {bc.NUM_INPUTS} inputs, file {len(data)} bytes"]
    host = []
    for _ in range(3):
        _, ms = bc.timed(lambda: hashlib.shake_256(data).digest(32))
        host.append(ms)
    lines.append(f"host: hashlib.shake_256 over the file's bytes, one core: ms {bc.span(host)} over {len(host)} passes")
    ctx = sbn.Context(0)
    try:
        f = ctx.circom_r1cs_load(data)
        info = f.info()
        leaves = sum((k + 127) // 128 for k in info["nnz"])
        lines.append(f"entries {info['nnz']}, leaves {leaves} ({32 * leaves} bytes brought back), hashed on the device {40 * sum(info['nnz']) + 39 * leaves} bytes")
        first = f.digest()
        call = []
        for _ in range(a.passes):
            d, ms = bc.timed(f.digest)
            assert d == first, "the digest changed between two calls"
            call.append(ms)
        lines.append(f"device: sbn_circom_r1cs_digest, the whole call: ms {bc.span(call)} over {a.passes} passes   digest {first.hex()}")
        ctx.prof_enable(True); ctx.prof_reset()
        for _ in range(a.passes):
            f.digest()
        prof = ctx.prof_get()
        ctx.prof_enable(False)
        for name, v in prof.items():
            lines.append(f"device: kernel {name}: {v[0]:.3f} ms over {v[1]} launches = {v[0] / max(v[1], 1):.3f} ms each")
        dg = ctx.nizk_gens_new(real, n, bc.NUM_INPUTS)
        inst = ctx.nizk_instance_from_circom(f, first)
        tape_ms = []
        for _ in range(a.passes):
            t = sbn.RandomTape(b"proof")
            _, ms = bc.timed(lambda: t.draw_nizk(inst))
            t.free()
            tape_ms.append(ms)
        lines.append(f"host: sbn_random_tape_new + sbn_nizk_draw_rnd ({inst.sizes()[0]} scalars): ms {bc.span(tape_ms)} over {a.passes} passes")
        inst.free(); dg.free(); f.free()
    finally:
        ctx.close()
    lines += cli_stages(np, rm, rng, data, n)
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(text)


if __name__ == "__main__":
    main()
