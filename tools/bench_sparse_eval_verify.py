#!/usr/bin/env python3
"""SparseMatPolyEvalProof::verify (sparse_mlpoly_full.rs:1815-1845), Merlin transcript included, two ways on one MI355X at the keyless shape
(N = 2^22 operations, 2^21 cells, batch 3: ell = 25 / 26 / 22): the one call sbn_sparse_eval_verify against the same check assembled from the
entry points that existed before it.

    python tools/bench_sparse_eval_verify.py [--small] [--passes 5] [--out profiles/r22_sparse_eval_verify.txt]

The proof comes from sbn_sparse_eval_prove on the synthetic keyless instance of tests/r1cs_model.py; the computation commitment (the row
commitments of comb_ops and comb_mem) is made once with sbn_commit_table and stays resident, as a verifier holds it.  `--passes` alternating passes of
    one_call   sbn_sparse_eval_verify (warm handles: the generators' derived sets and lookup tables exist)
    assembled  sbn_bases_from_compressed for comm_derefs, three sbn_joint_opening_verify, the transcript through sbn_transcript_*, and the field part
               (ProductLayerProof::verify, the hash checks) in Python, by tests/sparse_eval_model.py
both ending in the same verdict and the same transcript state.  The assembled form is driven from Python: its time is reported whole and split
into the time inside the library's calls (assembled_calls_ms) and the caller's own (assembled_host_ms), so that the interpreter is not mistaken
for the device; the proof's scalars are parsed before the clock starts (a compiled caller holds them deserialised).  The second line lists the
HIP-event kernel totals of one call by kernel name.  (--small: 2^12 x 2^12, a functional check.)"""
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
TR = b"bench sparse eval verify"


def b32(v):
    return int(v % R).to_bytes(32, "little")


def sbs(xs):
    return b"".join(b32(x) for x in xs)


class Clock:
    """time spent inside the calls wrapped with it"""

    def __init__(self):
        self.ms, self.calls = 0.0, 0

    def __call__(self, fn, *a, **kw):
        t0 = time.perf_counter(); out = fn(*a, **kw); self.ms += (time.perf_counter() - t0) * 1e3; self.calls += 1
        return out


class DevTranscript:
    """sbn_transcript_* behind the interface of tests/transcript_model.Transcript"""

    def __init__(self, clock, inner):
        self.clock, self.s = clock, inner

    def append_message(self, label, msg):
        self.clock(self.s.append_message, label, msg)

    def append_scalar(self, label, x):
        self.clock(self.s.append_message, label, b32(x))

    def challenge_scalar(self, label):
        return int.from_bytes(self.clock(self.s.challenge_scalar, label), "little")

    def state(self):
        return self.s.state()


def assembled(sbn, ctx, sem, sevm, shape, parsed, fields, comm_h, rx, ry, evals, gens, clock):
    """-> (accepted, transcript state); parsed: the proof's scalar fields as sparse_eval_model holds them"""
    tr = DevTranscript(clock, sbn.Transcript(TR))
    comp = fields["comm_derefs"]
    tr.append_message(b"protocol-name", sem.NAME)
    tr.append_message(b"derefs_commitment", b"begin_derefs_commitment")
    tr.append_message(b"comm_poly_row_col_ops_val", b"poly_commitment_begin")
    for i in range(len(comp) // 32):
        tr.append_message(b"poly_commitment_share", comp[32 * i:32 * i + 32])
    tr.append_message(b"comm_poly_row_col_ops_val", b"poly_commitment_end")
    tr.append_message(b"derefs_commitment", b"end_derefs_commitment")
    r_hash, r_multiset = tr.challenge_scalar(b"challenge_r_hash"), tr.challenge_scalar(b"challenge_r_hash")
    tr.append_message(b"protocol-name", sem.NAME)
    try:
        comm_d = clock(ctx.bases_from_compressed, comp)
    except sbn.SbnError:
        return False, tr.state()
    try:
        got = sem.product_layer_verify(tr, parsed["prod"], shape.N, shape.cells, evals)
        if got is None:
            return False, tr.state()
        claims_mem, rand_mem, claims_ops, claims_dotp, rand_ops = got
        rx_ext, ry_ext = sem.equalize(rx, ry)
        h = sevm.hash_layer_field(parsed["hash"], shape.b, rand_mem, claims_mem, claims_ops, claims_dotp, rx_ext, ry_ext, r_hash, r_multiset)
        if h is None:
            return False, tr.state()
        tr.append_message(b"protocol-name", b"Sparse polynomial hash layer proof")
        tr.append_message(b"protocol-name", b"Derefs evaluation proof")
        for kind, comm, ev, labels, r in (("derefs", comm_d, h[0], sem.DEREFS_LABELS, rand_ops), ("ops", comm_h[0], h[1], sem.OPS_LABELS, rand_ops), ("mem", comm_h[1], h[2], sem.MEM_LABELS, rand_mem)):
            ok, _ = clock(ctx.joint_opening_verify, gens[kind], comm, sbs(ev), labels, sbs(r), fields["hash.proof_" + kind], tr.s)
            if not ok:
                return False, tr.state()
        return True, tr.state()
    finally:
        comm_d.free()


def span(xs):
    return [round(min(xs), 3), round(max(xs), 3)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--passes", type=int, default=5)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--small", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import numpy as np
    import polyeval_model as pm
    import r1cs_model as rm
    import sparse_eval_loop as loop
    import sparse_eval_model as sem
    import sparse_eval_verify_model as sevm
    sbn = load_pkg()
    ctx = sbn.Context(0)
    lines = []
    try:
        if a.small:
            nx = ny = 12
            mats = loop.random_mats(nx, ny, 1 << 12, 3, a.seed)
        else:
            nc, nv, mats = rm.keyless_instance(a.seed)
            nx, ny = nc.bit_length() - 1, (2 * nv).bit_length() - 1
        dense = ctx.dense_build(nx, ny, mats)
        N, b = dense.num_ops, dense.batch
        shape = sem.Shape(nx, ny, N, b)
        n_rnd, n_proof = sbn.sparse_eval_sizes(nx, ny, N, b)
        gens = {k: ctx.gens_new(shape.R(k) + 1, b"gens_r1cs_eval", want_points=False)[0] for k in ("ops", "mem", "derefs")}
        rng = np.random.default_rng(a.seed + 1)
        rx_b, ry_b = rm.random_vals(rng, nx).tobytes(), rm.random_vals(rng, ny).tobytes()
        rnd = rm.random_vals(rng, n_rnd).tobytes()
        evals_b = loop.evals_of(sbn, ctx, dense, rx_b, ry_b)
        tp = sbn.Transcript(TR)
        proof = ctx.sparse_eval_prove(dense, rx_b, ry_b, evals_b, gens["ops"], gens["mem"], gens["derefs"], rnd, tp)
        comm_h, splits = [], []
        for kind, tab in (("ops", dense.comb_ops), ("mem", dense.comb_mem)):
            Gn, G1 = ctx.bases_split_at(gens[kind], shape.R(kind))
            splits += [Gn, G1]
            xy, _ = ctx.commit_table(Gn, tab, None, 1 << pm.factored_lens(shape.ell[kind])[0], shape.R(kind))
            comm_h.append(ctx.bases_upload(xy))
        dense.free()
        want = (True, tp.state())
        rx, ry, evals = rm.from_bytes(rx_b), rm.from_bytes(ry_b), rm.from_bytes(evals_b)
        sp = sem.field_spans(shape)
        fields = {f: proof[lo:hi] for f, (lo, hi) in sp.items()}
        # the scalar fields as the model holds them; the points stay bytes (no host decompression: the library does it)
        pts = {"comm_derefs", "hash.proof_ops", "hash.proof_mem", "hash.proof_derefs"}
        G = (1).to_bytes(32, "little")                              # the generator (1, 2), compressed: a stand-in that decompresses
        stub = b"".join((G * ((hi - lo) // 32)) if f == "comm_derefs" else (G * ((hi - lo - 64) // 32) + proof[hi - 64:hi]) if f in pts else proof[lo:hi] for f, (lo, hi) in sp.items())
        parsed = sem.proof_from_bytes(stub, shape)

        def one_call():
            t = sbn.Transcript(TR)
            return ctx.sparse_eval_verify(nx, ny, N, shape.cells, b, comm_h[0], comm_h[1], rx_b, ry_b, evals_b, gens["ops"], gens["mem"], gens["derefs"], proof, t), t.state()

        assert one_call() == want, "the one call refuses the prover's proof"                  # warm-up of both forms, and the verdicts
        got = assembled(sbn, ctx, sem, sevm, shape, parsed, fields, comm_h, rx, ry, evals, gens, Clock())
        assert got == want, "the assembled verifier disagrees"
        one, whole, inside, ncalls = [], [], [], 0
        for _ in range(a.passes):                                   # alternating: other work shares the host
            ctx.sync()
            t0 = time.perf_counter(); r1 = one_call(); one.append((time.perf_counter() - t0) * 1e3)
            assert r1 == want
            ck = Clock()
            t0 = time.perf_counter(); r2 = assembled(sbn, ctx, sem, sevm, shape, parsed, fields, comm_h, rx, ry, evals, gens, ck); whole.append((time.perf_counter() - t0) * 1e3)
            assert r2 == want
            inside.append(ck.ms); ncalls = ck.calls
        out = {"bench": "sparse_eval_verify", "num_vars_x": nx, "num_vars_y": ny, "num_ops": N, "batch": b, "ell": shape.ell, "proof_bytes": n_proof, "passes": a.passes,
               "one_call_ms": span(one), "assembled_ms": span(whole), "assembled_calls_ms": span(inside),
               "assembled_host_ms": span([w - i for w, i in zip(whole, inside)]), "assembled_library_calls": ncalls, "same_verdict_and_state": True}
        lines.append(out)
        print(json.dumps(out), flush=True)
        ctx.prof_enable(True); ctx.prof_reset()
        try:
            assert one_call() == want
            prof = ctx.prof_get()
        finally:
            ctx.prof_enable(False)
        st = {"bench": "sparse_eval_verify_kernels", "kernel_ms_total": round(sum(ms for ms, _ in prof.values()), 3),
              "kernel_ms_launches": {n: [round(ms, 3), int(l)] for n, (ms, l) in sorted(prof.items(), key=lambda kv: -kv[1][0])}}
        lines.append(st)
        print(json.dumps(st), flush=True)
        for h in comm_h + splits + list(gens.values()):
            h.free()
    finally:
        ctx.close()
    if a.out:
        with open(a.out, "w") as f:
            for ln in lines:
                f.write(json.dumps(ln) + "\n")


if __name__ == "__main__":
    main()
