#!/usr/bin/env python3
"""R1CSProof::prove (r1csproof.rs:241-459), Merlin transcript included, two ways on one MI355X: the one call sbn_r1cs_proof_prove against
the same proof assembled from the entry points that existed before it (tests/r1cs_proof_loop.py: sbn_commit_table, sbn_transcript_*,
sbn_eq_evals, upload of a host-built z, sbn_r1cs_multiply, sbn_zk_sumcheck_prove_r1cs, a one-row sbn_commit_rows per Σ-protocol element
over a gens_1 handle with a lookup table, sbn_r1cs_eval_table, sbn_zk_sumcheck_prove_quad, sbn_table_evaluate, sbn_polyeval_prove).  Both
legs are driven from Python through ctypes — a proof takes tens of milliseconds and the loop makes about 25 calls, so the caller's
overhead is noise.  The legs alternate, `--pairs` times, `--reps` proofs each (the median of a pass is reported); the instance, the witness
table, the generator handles and their derived sets are made outside the timed region, by one warm-up proof per leg.  Both legs must end
with the same bytes.  The last line lists the one call's kernel time and launches per name from the library's HIP-event profiler.

    python tools/bench_r1cs_proof.py [--log-cons 20] [--log-vars 20] [--pairs 5] [--reps 5] [--out profiles/r11_r1cs_proof.jsonl]

The default shape is the keyless one, 2^20 x 2^20, on the synthetic instance of r1cs_model.keyless_instance."""
import argparse
import hashlib
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from __graft_entry__ import load_pkg  # noqa: E402

def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log-cons", type=int, default=20)
    ap.add_argument("--log-vars", type=int, default=20)
    ap.add_argument("--inputs", type=int, default=10)
    ap.add_argument("--pairs", type=int, default=5)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import numpy as np
    import r1cs_model as rm
    import r1cs_proof_loop as loop
    sbn = load_pkg()
    nc, nv = 1 << args.log_cons, 1 << args.log_vars
    if (args.log_cons, args.log_vars) == (rm.KEYLESS_LOG, rm.KEYLESS_LOG):
        _, _, mats = rm.keyless_instance()
    else:
        mats = loop.random_instance(nc, nv, 1)
    rng = np.random.default_rng(11)
    vars_b = rm.random_vals(rng, nv).tobytes()
    input_b = rm.random_vals(rng, args.inputs).tobytes() if args.inputs else b""
    n_rnd, n_proof = sbn.r1cs_proof_sizes(nc, nv)
    rnd = rm.random_vals(rng, n_rnd).tobytes()
    R = 1 << (args.log_vars - args.log_vars // 2)
    ctx = sbn.Context(0)
    lines = []
    try:
        pc, _ = ctx.gens_new(R + 1, b"gens_r1cs_sat", want_points=False)
        g3, _ = ctx.gens_new(3, b"gens_r1cs_sat", want_points=False)
        g4, _ = ctx.gens_new(4, b"gens_r1cs_sat", want_points=False)
        lg = loop.LoopGens(ctx, pc, R)
        inst = ctx.r1cs_upload(nc, nv, mats)
        vt = ctx.table_upload(vars_b)

        def one():
            tr = sbn.Transcript(b"bench r1cs proof")
            out = ctx.r1cs_proof_prove(inst, vt, input_b, pc, g3, g4, rnd, tr)
            return out, tr.state()

        def many():
            tr = sbn.Transcript(b"bench r1cs proof")
            out = loop.prove_loop(sbn, ctx, inst, vt, vars_b, input_b, pc, lg, g3, g4, rnd, tr)
            return out, tr.state()
        legs = {"one_call": one, "loop": many}
        digests = {k: hashlib.sha256(repr(f()).encode()).hexdigest() for k, f in legs.items()}      # warm-up: derived sets, lookup tables, pool
        times = {k: [] for k in legs}
        for _ in range(args.pairs):
            for k, f in legs.items():
                us = []
                for _ in range(args.reps):
                    t0 = time.perf_counter()
                    f()
                    us.append((time.perf_counter() - t0) * 1e6)
                times[k].append(statistics.median(us))
        out = {"bench": "r1cs_proof_prove", "log_cons": args.log_cons, "log_vars": args.log_vars, "inputs": args.inputs, "nnz": [len(m[0]) for m in mats],
               "rnd_scalars": n_rnd, "proof_bytes": n_proof, "pairs": args.pairs, "reps": args.reps}
        for k, xs in times.items():
            out[k + "_us"] = [round(x, 1) for x in xs]
            out[k + "_us_median"] = round(statistics.median(xs), 1)
            out[k + "_us_min_max"] = [round(min(xs), 1), round(max(xs), 1)]
        out["same_bytes"] = digests["one_call"] == digests["loop"]
        lines.append(out)
        print(json.dumps(out), flush=True)
        # where the one call's device time goes: kernel milliseconds and launches per profiler name from the library's HIP events (one proof;
        # the events serialise host and device, so no wall time is taken here)
        ctx.prof_enable(True); ctx.prof_reset()
        try:
            one()
            prof = ctx.prof_get()
        finally:
            ctx.prof_enable(False)
        st = {"bench": "r1cs_proof_prove_kernels", "log_cons": args.log_cons, "log_vars": args.log_vars,
              "kernel_ms_total": round(sum(ms for ms, _ in prof.values()), 3),
              "kernel_ms_launches": {n: [round(ms, 3), int(l)] for n, (ms, l) in sorted(prof.items(), key=lambda kv: -kv[1][0])}}
        lines.append(st)
        print(json.dumps(st), flush=True)
        lg.free(); vt.free(); inst.free(); pc.free(); g3.free(); g4.free()
    finally:
        ctx.close()
    if args.out:
        with open(args.out, "w") as f:
            for ln in lines:
                f.write(json.dumps(ln) + "\n")
    if not lines[0]["same_bytes"]:
        raise SystemExit("the two legs ended with different bytes")


if __name__ == "__main__":
    main()
