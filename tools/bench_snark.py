#!/usr/bin/env python3
"""SNARK::encode, ::prove and ::verify (snark.rs:417-528) and Instance::is_sat (:137-158) on one MI355X at the keyless shape, each two ways: the one
call (sbn_snark_prove / sbn_snark_verify) against the same work through the entry points that existed before it.

    python tools/bench_snark.py [--log 20] [--passes 5] [--out profiles/r23_snark.jsonl]

The instance is tests/r1cs_model.keyless_instance (2^20 x 2^20, nnz 3,151,183 / 1,040,083 / 2,940,867, the long row, the constant column) given to
sbn_snark_encode as a raw circuit of 1,040,083 constraints, 2^20 variables and 10 inputs: columns past the last input are folded back onto the variables,
and C gets one more entry a real row in the constant column, (Az)_i (Bz)_i - (Cz)_i computed by sbn_r1cs_multiply, so that the random witness
satisfies it (N stays 2^22) and the verifier's accepting path is the one that is timed.  `--passes` alternating passes of
    prove:   one_call   sbn_snark_prove
             sequence   the prefix through sbn_transcript_append_message, sbn_r1cs_proof_prove, sbn_r1cs_evaluate, sbn_sparse_eval_prove
    verify:  one_call   sbn_snark_verify
             sequence   the prefix, sbn_r1cs_proof_verify, sbn_sparse_eval_verify
both ending in the same bytes, the same verdict and the same transcript state.  Then sbn_snark_encode (one pass: it is a per-circuit cost), and
sbn_r1cs_is_sat beside sbn_r1cs_multiply on a ready z (the check adds k_r1cs_build_z and one pass over Az, Bz, Cz: 96 MiB at this shape).
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
TR = b"bench snark"
NUM_INPUTS = 10


def span(xs):
    return [round(min(xs), 3), round(max(xs), 3)]


def timed(fn):
    t0 = time.perf_counter(); out = fn()
    return out, (time.perf_counter() - t0) * 1e3


def prefix(tr, comm):
    """the lines in front of R1CSProof (snark.rs:440-442), from the commitment's bytes"""
    import snark_model as sm
    tr.append_message(b"protocol-name", sm.NAME)
    for k, label in enumerate((b"num_cons", b"num_vars", b"num_inputs", b"batch_size", b"num_ops", b"num_mem_cells")):
        tr.append_message(label, comm[8 * k:8 * k + 8])
    nc, nv, _, _, N, _ = (int.from_bytes(comm[8 * k:8 * k + 8], "little") for k in range(6))
    Lo, Lm = sm.comm_lens(nc, nv, N)
    o = 48
    for label, n in ((b"comm_comb_ops", Lo), (b"comm_comb_mem", Lm)):
        tr.append_message(label, b"poly_commitment_begin")
        for _ in range(n):
            tr.append_message(b"poly_commitment_share", comm[o:o + 32]); o += 32
        tr.append_message(label, b"poly_commitment_end")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log", type=int, default=20, help="20: the keyless shape as it is; smaller: the same recipe scaled down (a quick look, not a figure)")
    ap.add_argument("--passes", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import numpy as np
    import r1cs_model as rm
    import snark_model as sm
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
        m0.free()
        corr = b"".join(((x * y - z) % R).to_bytes(32, "little") for x, y, z in zip(Az, Bz, Cz))
        cr, cc, cv = mats[2]
        mats[2] = (np.concatenate([cr, np.arange(real, dtype=np.uint32)]), np.concatenate([cc, np.full(real, n, np.uint32)]),
                   np.concatenate([cv.reshape(-1, 32), np.frombuffer(corr, dtype=np.uint8).reshape(-1, 32)]))
        nnz = [len(m[0]) for m in mats]
        gens = ctx.snark_gens_new(real, n, NUM_INPUTS, max(nnz))
        key, encode_ms = timed(lambda: ctx.snark_encode(real, n, NUM_INPUTS, mats, gens))
        comm = key.comm()
        inst = ctx.r1cs_upload(n, n, mats)                            # the sequence's own handle (raw = padded columns here: num_vars is a power of two)
        n_rnd, n_proof = key.sizes()
        n_sat_rnd, n_sat_proof = sbn.r1cs_proof_sizes(n, n)
        rnd = rm.random_vals(rng, n_rnd).tobytes()
        dense = key.dense
        nx, ny, N, cells = a.log, a.log + 1, dense.num_ops, dense.num_cells
        Lo = sm.comm_lens(n, n, N)[0]
        comm_h = [ctx.bases_from_compressed(comm[48:48 + 32 * Lo]), ctx.bases_from_compressed(comm[48 + 32 * Lo:])]

        def prove_one():
            tr = sbn.Transcript(TR)
            return ctx.snark_prove(key, vt, input_b, gens, rnd, tr), tr.state()

        def prove_seq():
            tr = sbn.Transcript(TR)
            prefix(tr, comm)
            sat, rx, ry = ctx.r1cs_proof_prove(inst, vt, input_b, gens.pc, gens.g3, gens.g4, rnd[:32 * n_sat_rnd], tr)
            evals = b"".join(ctx.r1cs_evaluate(inst, rx, ry))
            ev = ctx.sparse_eval_prove(dense, rx, ry, evals, gens.ops, gens.mem, gens.derefs, rnd[32 * n_sat_rnd:], tr)
            return sat + evals + ev, tr.state()

        want = prove_one()                                            # warm-up of both forms (the derived generator sets are built here), and the bytes
        assert prove_seq() == want and len(want[0]) == n_proof, "the sequence gives other bytes"
        proof = want[0]

        def verify_one():
            tr = sbn.Transcript(TR)
            return ctx.snark_verify(key, input_b, gens, proof, tr), tr.state()

        def verify_seq():
            tr = sbn.Transcript(TR)
            prefix(tr, comm)
            evals = proof[n_sat_proof:n_sat_proof + 96]
            got = ctx.r1cs_proof_verify(n, n, input_b, evals, gens.pc, gens.g3, gens.g4, proof[:n_sat_proof], tr)
            if got is None:
                return False, tr.state()
            return ctx.sparse_eval_verify(nx, ny, N, cells, 3, comm_h[0], comm_h[1], got[0], got[1], evals, gens.ops, gens.mem, gens.derefs, proof[n_sat_proof + 96:], tr), tr.state()

        assert verify_one() == (True, want[1]), "the one call refuses the prover's proof"
        assert verify_seq() == (True, want[1]), "the sequence refuses the prover's proof"
        t = {k: [] for k in ("prove_one", "prove_seq", "verify_one", "verify_seq", "is_sat", "multiply")}
        for _ in range(a.passes):                                     # alternating: other work shares the host
            for name, fn, expect in (("prove_one", prove_one, want), ("prove_seq", prove_seq, want), ("verify_one", verify_one, (True, want[1])), ("verify_seq", verify_seq, (True, want[1]))):
                ctx.sync()
                got, ms = timed(fn)
                assert got == expect, name
                t[name].append(ms)
            ctx.sync()
            got, ms = timed(lambda: ctx.r1cs_is_sat(inst, vt, input_b))
            assert got == (True, 0, 0)
            t["is_sat"].append(ms)
            ctx.sync()
            tabs, ms = timed(lambda: (ctx.r1cs_multiply(inst, zt), ctx.sync())[0])
            t["multiply"].append(ms)
            for x in tabs:
                x.free()
        out = {"bench": "snark", "log": a.log, "num_cons": real, "num_vars": n, "num_inputs": NUM_INPUTS, "nnz": nnz, "N": N, "passes": a.passes, "proof_bytes": n_proof, "comm_bytes": len(comm),
               "prove_one_call_ms": span(t["prove_one"]), "prove_sequence_ms": span(t["prove_seq"]), "verify_one_call_ms": span(t["verify_one"]), "verify_sequence_ms": span(t["verify_seq"]),
               "encode_ms": round(encode_ms, 1), "is_sat_ms": span(t["is_sat"]), "r1cs_multiply_ms": span(t["multiply"]), "same_bytes_verdict_and_state": True}
        lines.append(out)
        print(json.dumps(out), flush=True)
        ctx.prof_enable(True); ctx.prof_reset()
        try:
            assert ctx.r1cs_is_sat(inst, vt, input_b)[0]
            prof = ctx.prof_get()
        finally:
            ctx.prof_enable(False)
        st = {"bench": "snark_is_sat_kernels", "kernel_ms_launches": {k: [round(ms, 3), int(l)] for k, (ms, l) in sorted(prof.items(), key=lambda kv: -kv[1][0])}}
        lines.append(st)
        print(json.dumps(st), flush=True)
        for h in comm_h:
            h.free()
        inst.free(); key.free(); gens.free(); vt.free(); zt.free()
    finally:
        ctx.close()
    if a.out:
        with open(a.out, "w") as f:
            for ln in lines:
                f.write(json.dumps(ln) + "\n")


if __name__ == "__main__":
    main()
