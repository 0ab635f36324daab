#!/usr/bin/env python3
"""NIZK::prove and ::verify (snark.rs:202-286) on one MI355X at the keyless shape, each two ways: the one call (sbn_nizk_prove / sbn_nizk_verify) against
the same work through the entry points that existed before it; and the wall time of sbn_nizk_instance_new.

    python tools/bench_nizk.py [--log 20] [--passes 5] [--out profiles/r24_nizk.jsonl]

The instance is the synthetic raw circuit of tools/bench_snark.py: tests/r1cs_model.keyless_instance (2^20 x 2^20, nnz 3,151,183 / 1,040,083 /
2,940,867, the long row, the constant column) as a raw circuit of 1,040,083 constraints, 2^20 variables and 10 inputs, with one correcting entry a real
row in C's constant column so that the random witness satisfies it and the verifier's accepting path is the one that is timed.  The digest is 32 bytes of
the caller's.  `--passes` alternating passes of
    prove:   one_call   sbn_nizk_prove
             sequence   two sbn_transcript_append_message, sbn_r1cs_proof_prove, the proof | rx | ry laid end to end
    verify:  one_call   sbn_nizk_verify
             sequence   the two appends, sbn_r1cs_evaluate at the claimed point, sbn_r1cs_proof_verify, the comparison of the two points
both ending in the same bytes, the same verdict and the same transcript state.  Then the kernels and launches of one call of each (profiling on).
The one call runs the same launches as the sequence: no speed-up is claimed, a difference under 5 % on one box means nothing."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from __graft_entry__ import load_pkg  # noqa: E402

R = 0x30644e72e131a029b85045b68181585d2833e84879b9709143e1f593f0000001
TR = b"bench nizk"
NAME = b"Spartan NIZK proof"
NUM_INPUTS = 10
DIGEST = bytes(range(32))


def span(xs):
    return [round(min(xs), 3), round(max(xs), 3)]


def timed(fn):
    t0 = time.perf_counter(); out = fn()
    return out, (time.perf_counter() - t0) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log", type=int, default=20, help="20: the keyless shape as it is; smaller: the same recipe scaled down (a quick look, not a figure)")
    ap.add_argument("--passes", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import numpy as np
    import r1cs_model as rm
    sbn = load_pkg()
    rng = np.random.default_rng(22)
    if a.log == rm.KEYLESS_LOG:
        n, _, mats = rm.keyless_instance()
        real = rm.KEYLESS_REAL_ROWS
    else:
        n = 1 << a.log; real = n - n // 128
        mats = [(rng.integers(0, real, k * n, dtype=np.uint32), rng.integers(0, 2 * n, k * n, dtype=np.uint32), rm.random_vals(rng, k * n)) for k in (3, 1, 2)]
    live = n + 1 + NUM_INPUTS
    mats = [(r, np.where(c >= live, c - live, c).astype(np.uint32), v) for r, c, v in mats]      # raw columns: vars | 1 | inputs
    vars_b = rm.random_vals(rng, n).tobytes()
    input_b = rm.random_vals(rng, NUM_INPUTS).tobytes()
    ctx = sbn.Context(0)
    lines = []
    try:
        vt = ctx.table_upload(vars_b)
        zt = ctx.table_upload(vars_b + (1).to_bytes(32, "little") + input_b + bytes(32 * (n - 1 - NUM_INPUTS)))
        # the correcting entries of C
        m0 = ctx.r1cs_upload(n, n, mats)
        tabs = ctx.r1cs_multiply(m0, zt)
        Az, Bz, Cz = (rm.from_bytes(ctx.table_download(t)[:32 * real]) for t in tabs)
        for t in tabs:
            t.free()
        m0.free(); zt.free()
        corr = b"".join(((x * y - z) % R).to_bytes(32, "little") for x, y, z in zip(Az, Bz, Cz))
        cr, cc, cv = mats[2]
        mats[2] = (np.concatenate([cr, np.arange(real, dtype=np.uint32)]), np.concatenate([cc, np.full(real, n, np.uint32)]),
                   np.concatenate([cv.reshape(-1, 32), np.frombuffer(corr, dtype=np.uint8).reshape(-1, 32)]))
        nnz = [len(m[0]) for m in mats]
        gens = ctx.nizk_gens_new(real, n, NUM_INPUTS)
        ctx.sync()
        inst, instance_ms = timed(lambda: ctx.nizk_instance_new(real, n, NUM_INPUTS, mats, DIGEST))
        assert ctx.nizk_is_sat(inst, vt, input_b) == (True, 0, 0), "the synthetic witness does not satisfy the circuit"
        n_rnd, n_proof = inst.sizes()
        n_sat_rnd, n_sat_proof = sbn.r1cs_proof_sizes(n, n)
        nx, ny = a.log, a.log + 1
        assert (n_rnd, n_proof) == (n_sat_rnd, n_sat_proof + 32 * (nx + ny))
        rnd = rm.random_vals(rng, n_rnd).tobytes()

        def prefix(tr):
            tr.append_message(b"protocol-name", NAME); tr.append_message(b"R1CSShapeDigest", DIGEST)

        def prove_one():
            tr = sbn.Transcript(TR)
            return ctx.nizk_prove(inst, vt, input_b, gens, rnd, tr), tr.state()

        def prove_seq():
            tr = sbn.Transcript(TR)
            prefix(tr)
            sat, rx, ry = ctx.r1cs_proof_prove(inst.r1cs, vt, input_b, gens.pc, gens.g3, gens.g4, rnd, tr)
            return sat + rx + ry, tr.state()

        want = prove_one()                                            # warm-up of both forms (the derived generator sets are built here), and the bytes
        assert prove_seq() == want and len(want[0]) == n_proof, "the sequence gives other bytes"
        proof = want[0]
        crx, cry = proof[n_sat_proof:n_sat_proof + 32 * nx], proof[n_sat_proof + 32 * nx:]

        def verify_one():
            tr = sbn.Transcript(TR)
            return ctx.nizk_verify(inst, input_b, gens, proof, tr), tr.state()

        def verify_seq():
            tr = sbn.Transcript(TR)
            prefix(tr)
            evals = b"".join(ctx.r1cs_evaluate(inst.r1cs, crx, cry))
            got = ctx.r1cs_proof_verify(n, n, input_b, evals, gens.pc, gens.g3, gens.g4, proof[:n_sat_proof], tr)
            return got is not None and got == (crx, cry), tr.state()

        assert verify_one() == (True, want[1]), "the one call refuses the prover's proof"
        assert verify_seq() == (True, want[1]), "the sequence refuses the prover's proof"
        off = bytearray(proof); off[n_sat_proof] ^= 1                 # a claimed rx[0] that the transcript does not give: both forms refuse
        tr = sbn.Transcript(TR)
        assert ctx.nizk_verify(inst, input_b, gens, bytes(off), tr) is False and tr.state() == sbn.Transcript(TR).state()
        t = {k: [] for k in ("prove_one", "prove_seq", "verify_one", "verify_seq")}
        for _ in range(a.passes):                                     # alternating: other work shares the host
            for name, fn, expect in (("prove_one", prove_one, want), ("prove_seq", prove_seq, want), ("verify_one", verify_one, (True, want[1])), ("verify_seq", verify_seq, (True, want[1]))):
                ctx.sync()
                got, ms = timed(fn)
                assert got == expect, name
                t[name].append(ms)
        out = {"bench": "nizk", "log": a.log, "num_cons": real, "num_vars": n, "num_inputs": NUM_INPUTS, "nnz": nnz, "passes": a.passes, "proof_bytes": n_proof, "digest_bytes": len(DIGEST),
               "prove_one_call_ms": span(t["prove_one"]), "prove_sequence_ms": span(t["prove_seq"]), "verify_one_call_ms": span(t["verify_one"]), "verify_sequence_ms": span(t["verify_seq"]),
               "instance_new_ms": round(instance_ms, 1), "same_bytes_verdict_and_state": True}
        lines.append(out)
        print(json.dumps(out), flush=True)
        for name, fn in (("nizk_prove_kernels", prove_one), ("nizk_verify_kernels", verify_one)):
            ctx.prof_enable(True); ctx.prof_reset()
            try:
                fn()
                prof = ctx.prof_get()
            finally:
                ctx.prof_enable(False)
            st = {"bench": name, "launches": int(sum(l for _, l in prof.values())), "kernel_ms_launches": {k: [round(ms, 3), int(l)] for k, (ms, l) in sorted(prof.items(), key=lambda kv: -kv[1][0])}}
            lines.append(st)
            print(json.dumps(st), flush=True)
        inst.free(); gens.free(); vt.free()
    finally:
        ctx.close()
    if a.out:
        with open(a.out, "w") as f:
            for ln in lines:
                f.write(json.dumps(ln) + "\n")


if __name__ == "__main__":
    main()
