#!/usr/bin/env python3
"""KZG mode on one device: SRS from tau, commitment, opening (division + MSM) and a batched opening, over a resident SRS.

    python tools/bench_kzg.py [--log-n 25] [--batch 4] [--log-batch 23] [--reps 3]

Prints one JSON line: srs_ms (sbn_kzg_srs_from_tau of 2^n + 1 points), commit_ms, open_ms split into div_ms (the three division
kernels, k_kzg_div_*, by HIP events) and msm_ms, open_batched_ms (batch x 2^log_batch), the division's achieved bytes/s
(two reads of the coefficients and one write of the quotient) and identity_ok: the verifier's relation (tau - z) pi + y G == C
checked with the C oracle on the host (no pairing).  The derefs commitment the reference publishes for --features kzg is one MSM of
2^25 scalars over the SRS powers (BENCHMARK_RESULTS.md:46-57: 100.5 s)."""
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
G = (1).to_bytes(32, "little") + (2).to_bytes(32, "little")


def b32(v):
    return int(v).to_bytes(32, "little")


def best(fn, reps):
    t = []
    out = None
    for _ in range(reps):
        t0 = time.perf_counter(); out = fn(); t.append((time.perf_counter() - t0) * 1e3)
    return min(t), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log-n", type=int, default=25)
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--log-batch", type=int, default=23)
    ap.add_argument("--reps", type=int, default=3)
    a = ap.parse_args()
    import __graft_entry__ as ge
    import oracle_lib as ol
    sbn = ge.load_pkg()
    n = 1 << a.log_n
    rng = random.Random(a.log_n)
    tau, z, gamma = rng.randrange(1, R), rng.randrange(R), rng.randrange(R)
    ctx = sbn.Context(0)
    keep, tabs = [], []
    try:
        t0 = time.perf_counter()
        srs = ctx.kzg_srs_from_tau(b32(tau), n + 1)
        srs_ms = (time.perf_counter() - t0) * 1e3

        def synthetic(m, first):
            p = ctx.dev_alloc(32 * m); keep.append(p)
            ctx.scalars_synthetic(0x5BA27A2B4E254, first, m, p)
            t = ctx.table_from_dev(p, m); tabs.append(t)
            return t

        t = synthetic(n, 0)
        ctx.kzg_commit(srs, t, n); ctx.kzg_open(srs, t, n, b32(z))          # warm-up: workspaces, GLV table
        commit_ms, (C, _) = best(lambda: ctx.kzg_commit(srs, t, n), a.reps)
        open_ms, (ev, pi, _) = best(lambda: ctx.kzg_open(srs, t, n, b32(z)), a.reps)
        y = int.from_bytes(ev, "little")
        lhs = ol.g1_add(ol.g1_mul(pi, b32((tau - z) % R)), ol.g1_mul(G, b32(y)))
        identity_ok = lhs == C
        # the division's kernels alone, by HIP events
        div = []
        for _ in range(a.reps):
            ctx.prof_reset(); ctx.prof_enable(True)
            ev2, q = ctx.poly_div_linear(t, n, b32(z))
            prof = ctx.prof_get(); ctx.prof_enable(False)
            q.free()
            div.append(sum(ms for k, (ms, _) in prof.items() if k.startswith("k_kzg_div")))
            identity_ok = identity_ok and ev2 == ev
        div_ms = min(div)
        for x in tabs:
            x.free()
        for p in keep:
            ctx.dev_free(p)
        tabs.clear(); keep.clear()
        m = 1 << a.log_batch
        bt = [synthetic(m, k * m) for k in range(a.batch)]
        ctx.kzg_open_batched(srs, bt, [m] * a.batch, b32(z), b32(gamma))
        ob_ms, _ = best(lambda: ctx.kzg_open_batched(srs, bt, [m] * a.batch, b32(z), b32(gamma)), a.reps)
        srs.free()
        res = {"workload": "kzg", "log_n": a.log_n, "srs_ms": round(srs_ms, 1), "commit_ms": round(commit_ms, 2), "open_ms": round(open_ms, 2),
               "div_ms": round(div_ms, 3), "msm_ms": round(open_ms - div_ms, 2), "div_bytes_per_s": round(3 * 32 * n / (div_ms * 1e-3)),
               "open_batched_ms": round(ob_ms, 2), "batch": f"{a.batch}x2^{a.log_batch}", "identity_ok": bool(identity_ok),
               "reference_derefs_commit_ms": 100500.0}
        print(json.dumps(res))
    finally:
        for x in tabs:
            x.free()
        for p in keep:
            ctx.dev_free(p)
        ctx.close()


if __name__ == "__main__":
    main()
