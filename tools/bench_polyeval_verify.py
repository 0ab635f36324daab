#!/usr/bin/env python3
"""One Hyrax opening check on one device: sbn_polyeval_verify against the same verification assembled from the entry points that existed
before it, at the four keyless openings (ell = 20, 23, 25, 26: mem, witness, ops, derefs).

    python tools/bench_polyeval_verify.py [--ells 20,23,25,26] [--passes 5]

Per ell: a synthetic table on the device, its commitment by sbn_commit_table, a proof by sbn_polyeval_prove (no blinds), then `--passes`
alternating passes of
    one_call   sbn_polyeval_verify (warm handles: the derived set and its lookup table exist, the commitment is resident)
    assembled  sbn_eq_evals x 2 + downloads, C_LZ by sbn_msm over the commitment's host points, the transcript through sbn_transcript_*,
               the proof's points decompressed by the CPU oracle, s on the host, g_hat by sbn_msm_bases over the resident generators,
               the two sides of nizk/mod.rs:560-565 as two small sbn_msm calls
both ending in the same verdict and the same transcript state.  The assembled form is driven from Python: its time is reported whole and
split into the time inside the library's calls (assembled_calls_ms) and the caller's own (assembled_host_ms), so that the interpreter is not
mistaken for the device.  Prints one JSON line: per ell the min .. max of the passes in milliseconds, and the decompression kernel's time per
point at 8192 points (HIP events).  The reference publishes 390 ms for a whole SNARK::verify (BENCHMARK_RESULTS.md:24), of which four such
openings are the larger part — context only, another machine and the CPU."""
import argparse
import json
import os
import random
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

R = 0x30644e72e131a029b85045b68181585d2833e84879b9709143e1f593f0000001
TR = b"bench polyeval verify"


def b32(v):
    return int(v % R).to_bytes(32, "little")


def ib(b):
    return int.from_bytes(b, "little")


class Clock:
    """time spent inside the calls wrapped with it"""

    def __init__(self):
        self.ms = 0.0

    def __call__(self, fn, *a, **kw):
        t0 = time.perf_counter(); out = fn(*a, **kw); self.ms += (time.perf_counter() - t0) * 1e3
        return out


def assembled(sbn, ol, ctx, Gn, gens_tail, comm_xy, r, ell, C_Zr, proof, calls):
    """PolyEvalProof::verify by a caller of the earlier ABI -> (verdict, transcript state)"""
    ml, mr = ell // 2, ell - ell // 2
    n, lg = 1 << mr, mr
    Qb, H = gens_tail
    Lt, Rt = calls(ctx.eq_evals, r[:32 * ml]), calls(ctx.eq_evals, r[32 * ml:])
    try:
        Lb, Rb = calls(ctx.table_download, Lt), calls(ctx.table_download, Rt)
    finally:
        Lt.free(); Rt.free()
    Cx = calls(ctx.msm, Lb, comm_xy)[0]
    tr = sbn.Transcript(TR)
    tr.append_message(b"protocol-name", b"polynomial evaluation proof")
    tr.append_message(b"protocol-name", b"dot product proof (log)")
    tr.append_message(b"Cx", calls(sbn.g1_compress, Cx)); tr.append_message(b"Cy", calls(sbn.g1_compress, C_Zr))
    for i in range(n):
        tr.append_message(b"a", Rb[32 * i:32 * i + 32])
    rq = ib(tr.challenge_scalar(b"r"))
    pts = [ol.g1_decompress(proof[32 * i:32 * i + 32]) for i in range(2 * lg + 2)]
    if any(p is None for p in pts):
        return False, tr.state()
    us = []
    for j in range(lg):
        tr.append_message(b"L", proof[32 * j:32 * j + 32]); tr.append_message(b"R", proof[32 * (lg + j):32 * (lg + j) + 32])
        us.append(ib(tr.challenge_scalar(b"u")))
    tr.append_message(b"delta", proof[64 * lg:64 * lg + 32]); tr.append_message(b"beta", proof[64 * lg + 32:64 * lg + 64])
    c = ib(tr.challenge_scalar(b"c"))
    z1, z2 = ib(proof[64 * lg + 64:64 * lg + 96]), ib(proof[64 * lg + 96:])
    ui = [pow(u, -1, R) for u in us]
    s = [1]
    for k in range(lg):                                    # bit lg-1-k of the index takes u_k (bullet.rs:183-200): the tensor product, 2n products
        s = [x * f % R for x in s for f in (ui[k], us[k])]
    a_hat = sum(x * ib(Rb[32 * i:32 * i + 32]) for i, x in enumerate(s)) % R
    g_hat = calls(ctx.msm_bases, Gn, b"".join(b32(x) for x in s))[0]
    ac = a_hat * c % R
    lhs_s = [ac * u * u for u in us] + [ac * v * v for v in ui] + [1, a_hat, ac, ac * rq]
    lhs = calls(ctx.msm, b"".join(b32(x) for x in lhs_s), b"".join(pts) + Cx + C_Zr)[0]
    rhs = calls(ctx.msm, b32(z1) + b32(z1 * a_hat * rq) + b32(z2), g_hat + Qb + H)[0]
    return lhs == rhs, tr.state()


def span(xs):
    return [round(min(xs), 3), round(max(xs), 3)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ells", default="20,23,25,26")
    ap.add_argument("--passes", type=int, default=5)
    a = ap.parse_args()
    import __graft_entry__ as ge
    import oracle_lib as ol
    sbn = ge.load_pkg()
    ctx = sbn.Context(0)
    res = {"workload": "polyeval_verify", "passes": a.passes, "reference_snark_verify_ms": 390.0, "openings": {}}
    comp8192 = None
    try:
        for ell in (int(x) for x in a.ells.split(",")):
            ml, mr = ell // 2, ell - ell // 2
            n, N = 1 << mr, 1 << ell
            rng = random.Random(ell)
            bases, xy = ctx.gens_new(n + 1, b"gens_bench_polyeval_verify")
            tail = (xy[64 * n:64 * n + 64], xy[64 * n + 64:64 * n + 128])
            mem = ctx.dev_alloc(32 * N)
            ctx.scalars_synthetic(0xbe7c4 + ell, 0, N, mem)
            Zt = ctx.table_from_dev(mem, N)
            r = b"".join(b32(rng.randrange(R)) for _ in range(ell))
            rnd = b"".join(b32(rng.randrange(R)) for _ in range(3 + 2 * mr))
            Gn, G1 = ctx.bases_split_at(bases, n)
            comm = None
            try:
                Zr = ctx.table_evaluate(Zt, r)
                tp = sbn.Transcript(TR)
                proof, _, Cy = ctx.polyeval_prove(bases, Zt, r, Zr, rnd, tp)
                comm_xy, _ = ctx.commit_table(Gn, Zt, None, 1 << ml, n)
                comm = ctx.bases_upload(comm_xy)
                if (1 << ml) == 8192:
                    comp8192 = sbn.g1_compress(comm_xy)

                def one_call():
                    t = sbn.Transcript(TR)
                    return ctx.polyeval_verify(bases, comm, r, proof, t, C_Zr_xy=Cy), t.state()

                want = (True, tp.state())
                assert one_call() == want, "the one call refuses the prover's proof"          # warm-up of both forms, and the verdicts
                assert assembled(sbn, ol, ctx, Gn, tail, comm_xy, r, ell, Cy, proof, Clock()) == want, "the assembled verifier disagrees"
                one, whole, inside = [], [], []
                for _ in range(a.passes):                  # alternating: other work shares the host
                    ctx.sync()
                    t0 = time.perf_counter(); got = one_call(); one.append((time.perf_counter() - t0) * 1e3)
                    assert got == want
                    ck = Clock()
                    t0 = time.perf_counter(); got = assembled(sbn, ol, ctx, Gn, tail, comm_xy, r, ell, Cy, proof, ck); whole.append((time.perf_counter() - t0) * 1e3)
                    assert got == want
                    inside.append(ck.ms)
                res["openings"][str(ell)] = {"L_size": 1 << ml, "R_size": n, "one_call_ms": span(one), "assembled_ms": span(whole), "assembled_calls_ms": span(inside),
                                             "assembled_host_ms": span([w - i for w, i in zip(whole, inside)])}
            finally:
                for b in (comm, Gn, G1, bases):
                    if b is not None:
                        b.free()
                Zt.free(); ctx.dev_free(mem)
        if comp8192 is not None:
            ctx.g1_decompress(comp8192)
            per = []
            for _ in range(a.passes):
                ctx.prof_reset(); ctx.prof_enable(True)
                _, ok = ctx.g1_decompress(comp8192)
                prof = ctx.prof_get(); ctx.prof_enable(False)
                assert ok == bytes([1] * 8192)
                per.append(prof["k_g1_decompress"][0] * 1e6 / 8192)
            res["decompress_ns_per_point_at_8192"] = span(per)
        print(json.dumps(res))
    finally:
        ctx.prof_enable(False)
        ctx.close()


if __name__ == "__main__":
    main()
