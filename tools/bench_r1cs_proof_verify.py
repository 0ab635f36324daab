#!/usr/bin/env python3
"""R1CSProof::verify (r1csproof.rs:463-619), Merlin transcript included, two ways on one MI355X at the keyless shape 2^20 x 2^20: the one call
sbn_r1cs_proof_verify against the same verification assembled from the entry points that existed before it.

    python tools/bench_r1cs_proof_verify.py [--log-cons 20] [--log-vars 20] [--passes 5] [--out profiles/r21_r1cs_proof_verify.jsonl]

The proof comes from sbn_r1cs_proof_prove on a satisfied instance (row i: a_i z[i mod num_vars] * 1 = a_i z[i mod num_vars]); A, B, C(rx, ry) from
sbn_r1cs_evaluate.  `--passes` alternating passes of
    one_call   sbn_r1cs_proof_verify (warm handles: the generators' derived sets and lookup tables exist)
    assembled  tests/r1cs_proof_verify_model.verify with the device under it: the proof's points by ONE sbn_g1_decompress, every computed point
               and every equation (the same term lists, each moved to one side) as ONE sbn_msm over host points, the opening by
               sbn_bases_from_compressed + sbn_polyeval_verify, the transcript through sbn_transcript_*
both ending in the same verdict, the same challenges and the same transcript state.  The assembled form is driven from Python: its time is
reported whole and split into the time inside the library's calls (assembled_calls_ms) and the caller's own (assembled_host_ms), so that the
interpreter is not mistaken for the device.  The second line lists, from the library's HIP events, the time of k_pow2_table, of k_select_sum per
launch and of every other kernel of the one call.  The reference publishes 390 ms for a whole SNARK::verify on its CPU (BENCHMARK_RESULTS.md:24)
— context only."""
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
TR = b"bench r1cs proof verify"


def b32(v):
    return int(v % R).to_bytes(32, "little")


class Clock:
    """time spent inside the calls wrapped with it"""

    def __init__(self):
        self.ms, self.calls = 0.0, 0

    def __call__(self, fn, *a, **kw):
        t0 = time.perf_counter(); out = fn(*a, **kw); self.ms += (time.perf_counter() - t0) * 1e3; self.calls += 1
        return out


class DevTranscript:
    """sbn_transcript_* behind the interface of tests/transcript_model.Transcript"""

    def __init__(self, sbn, clock, inner):
        self.sbn, self.clock, self.s = sbn, clock, inner

    def append_message(self, label, msg):
        self.clock(self.s.append_message, label, msg)

    def append_scalar(self, label, x):
        self.clock(self.s.append_message, label, b32(x))

    def challenge_scalar(self, label):
        return int.from_bytes(self.clock(self.s.challenge_scalar, label), "little")

    def clone(self):
        return DevTranscript(self.sbn, self.clock, self.clock(self.s.clone))

    def state(self):
        return self.s.state()


def assembled(sbn, ctx, vm, shape, inputs, evals, gens, pc, proof, clock):
    """-> ((rx, ry) or None, transcript state, number of sbn_msm calls)"""
    nc, nv = shape
    msms = [0]

    class MsmRun(vm.Run):
        def total(self, terms):
            if not terms:
                return vm.INF
            msms[0] += 1
            return clock(ctx.msm, b"".join(b32(s) for _, s in terms), b"".join(self.T[i] for i, _ in terms))[0]

    def decompress(comp):
        xy, ok = clock(ctx.g1_decompress, b"".join(comp))
        return None if 0 in ok else [xy[64 * i:64 * i + 64] for i in range(len(comp))]

    def open_check(t, opening, gens_pc, r, C_Zr, comm_bytes):
        try:
            comm = clock(ctx.bases_from_compressed, comm_bytes)
        except sbn.SbnError:
            return False
        try:
            return clock(ctx.polyeval_verify, pc, comm, b"".join(b32(x) for x in r), opening, t.s, C_Zr_xy=C_Zr)
        finally:
            comm.free()
    tr = DevTranscript(sbn, clock, sbn.Transcript(TR))
    got = vm.verify(tr, proof, nc, nv, inputs, evals, gens, run_cls=MsmRun, decompress=decompress, open_check=open_check)
    return (None if got is None else (b"".join(b32(x) for x in got[0]), b"".join(b32(x) for x in got[1]))), tr.state(), msms[0]


def span(xs):
    return [round(min(xs), 3), round(max(xs), 3)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log-cons", type=int, default=20)
    ap.add_argument("--log-vars", type=int, default=20)
    ap.add_argument("--inputs", type=int, default=10)
    ap.add_argument("--passes", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import numpy as np
    import r1cs_model as rm
    import r1cs_proof_model as rpm
    import r1cs_proof_verify_model as vm
    sbn = load_pkg()
    nc, nv = 1 << a.log_cons, 1 << a.log_vars
    rng = np.random.default_rng(21)
    rows = np.arange(nc, dtype=np.uint32)
    cols = (rows % nv).astype(np.uint32)
    vals = rm.random_vals(rng, nc)
    one = np.zeros((nc, 32), dtype=np.uint8); one[:, 0] = 1
    mats = [(rows, cols, vals), (rows, np.full(nc, nv, np.uint32), one), (rows, cols, vals)]
    vars_b = rm.random_vals(rng, nv).tobytes()
    input_b = rm.random_vals(rng, a.inputs).tobytes() if a.inputs else b""
    inputs = rm.from_bytes(input_b)
    n_rnd, n_proof = sbn.r1cs_proof_sizes(nc, nv)
    rnd = rm.random_vals(rng, n_rnd).tobytes()
    Rn = 1 << (a.log_vars - a.log_vars // 2)
    ctx = sbn.Context(0)
    lines = []
    try:
        pc, pc_xy = ctx.gens_new(Rn + 1, b"gens_r1cs_sat")
        g3, g3_xy = ctx.gens_new(3, b"gens_r1cs_sat")
        g4, g4_xy = ctx.gens_new(4, b"gens_r1cs_sat")
        gens = rpm.make_gens(pc_xy, Rn, g3_xy, g4_xy)
        inst = ctx.r1cs_upload(nc, nv, mats)
        vt = ctx.table_upload(vars_b)
        tp = sbn.Transcript(TR)
        proof, rx, ry = ctx.r1cs_proof_prove(inst, vt, input_b, pc, g3, g4, rnd, tp)
        evals_b = b"".join(ctx.r1cs_evaluate(inst, rx, ry))
        evals = rm.from_bytes(evals_b)
        vt.free(); inst.free()
        want = ((rx, ry), tp.state())

        def one_call():
            t = sbn.Transcript(TR)
            return ctx.r1cs_proof_verify(nc, nv, input_b, evals_b, pc, g3, g4, proof, t), t.state()

        assert one_call() == want, "the one call refuses the prover's proof"                  # warm-up of both forms, and the verdicts
        got = assembled(sbn, ctx, vm, (nc, nv), inputs, evals, gens, pc, proof, Clock())
        assert got[:2] == want, "the assembled verifier disagrees"
        one, whole, inside, ncalls = [], [], [], 0
        for _ in range(a.passes):                          # alternating: other work shares the host
            ctx.sync()
            t0 = time.perf_counter(); r1 = one_call(); one.append((time.perf_counter() - t0) * 1e3)
            assert r1 == want
            ck = Clock()
            t0 = time.perf_counter(); r2 = assembled(sbn, ctx, vm, (nc, nv), inputs, evals, gens, pc, proof, ck); whole.append((time.perf_counter() - t0) * 1e3)
            assert r2[:2] == want
            inside.append(ck.ms); ncalls = ck.calls
        out = {"bench": "r1cs_proof_verify", "log_cons": a.log_cons, "log_vars": a.log_vars, "inputs": a.inputs, "proof_bytes": n_proof, "passes": a.passes,
               "one_call_ms": span(one), "assembled_ms": span(whole), "assembled_calls_ms": span(inside),
               "assembled_host_ms": span([w - i for w, i in zip(whole, inside)]), "assembled_msm_calls": got[2], "assembled_library_calls": ncalls,
               "same_verdict_and_state": True, "reference_snark_verify_ms": 390.0}
        lines.append(out)
        print(json.dumps(out), flush=True)
        ctx.prof_enable(True); ctx.prof_reset()
        try:
            assert one_call() == want
            prof = ctx.prof_get()
        finally:
            ctx.prof_enable(False)
        sel = prof["k_select_sum"]
        st = {"bench": "r1cs_proof_verify_kernels", "k_pow2_table_ms": round(prof["k_pow2_table"][0], 3),
              "k_select_sum_ms_per_launch": round(sel[0] / sel[1], 4), "k_select_sum_launches": int(sel[1]),
              "kernel_ms_total": round(sum(ms for ms, _ in prof.values()), 3),
              "kernel_ms_launches": {n: [round(ms, 3), int(l)] for n, (ms, l) in sorted(prof.items(), key=lambda kv: -kv[1][0])}}
        lines.append(st)
        print(json.dumps(st), flush=True)
        pc.free(); g3.free(); g4.free()
    finally:
        ctx.close()
    if a.out:
        with open(a.out, "w") as f:
            for ln in lines:
                f.write(json.dumps(ln) + "\n")


if __name__ == "__main__":
    main()
