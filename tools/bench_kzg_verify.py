#!/usr/bin/env python3
"""KZG verification on the device: `sbn_kzg_verify` alone (the three-term G1 sum, then one two-term pairing product) and `sbn_pairing_products`
with two terms a check at 1, 64, 1024 and 4096 checks a launch, as checks per second.  `--passes` passes on one box, each the mean of `--reps`
calls through ctypes; the range over the passes is printed, then the HIP-event kernel totals of one call.  Every verdict is asserted (an honest
opening is accepted, a tampered one refused; the products' verdicts are the fixture's) before anything is timed.  Last, `sbn_sparse_eval_verify_kzg`
at the keyless shape (N = 2^22 operations, 2^21 cells, batch 3, the SRS from the fixture's tau) on the proof of `sbn_sparse_eval_prove_kzg`, beside
the Hyrax build's one call on its own proof of the same instance as context, alternating (--small: 2^12 x 2^12; --no-sparse: skip).

    python tools/bench_kzg_verify.py [--passes 5] [--reps 20] [--checks 1,64,1024,4096] [--small] [--no-sparse]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: F401,E402
from __graft_entry__ import load_pkg  # noqa: E402
import bench  # noqa: E402


def sparse(sbn, ctx, kat, g2, tau_g2, passes, small):
    """-> the result line of the two one-call verifiers at one instance"""
    import numpy as np
    import polyeval_model as pm
    import r1cs_model as rm
    import sparse_eval_loop as loop
    import sparse_eval_model as sem
    TR = b"bench kzg verify"
    if small:
        nx = ny = 12
        mats = loop.random_mats(nx, ny, 1 << 12, 3, 1)
    else:
        nc, nv, mats = rm.keyless_instance(1)
        nx, ny = nc.bit_length() - 1, (2 * nv).bit_length() - 1
    dense = ctx.dense_build(nx, ny, mats)
    N, b = dense.num_ops, dense.batch
    shape = sem.Shape(nx, ny, N, b)
    gens = {k: ctx.gens_new(shape.R(k) + 1, b"gens_r1cs_eval", want_points=False)[0] for k in ("ops", "mem", "derefs")}
    srs = ctx.kzg_srs_from_tau(int(kat["tau"], 16).to_bytes(32, "little"), 1 << shape.ell["derefs"])
    rng = np.random.default_rng(2)
    rx, ry = rm.random_vals(rng, nx).tobytes(), rm.random_vals(rng, ny).tobytes()
    evals = loop.evals_of(sbn, ctx, dense, rx, ry)
    th, tk = sbn.Transcript(TR), sbn.Transcript(TR)
    p_hyrax = ctx.sparse_eval_prove(dense, rx, ry, evals, gens["ops"], gens["mem"], gens["derefs"], rm.random_vals(rng, sbn.sparse_eval_sizes(nx, ny, N, b)[0]).tobytes(), th)
    p_kzg = ctx.sparse_eval_prove_kzg(dense, rx, ry, evals, gens["ops"], gens["mem"], srs, None, rm.random_vals(rng, sbn.sparse_eval_kzg_sizes(nx, ny, N, b)[0]).tobytes(), tk)
    comm_h, splits = [], []
    for kind, tab in (("ops", dense.comb_ops), ("mem", dense.comb_mem)):
        Gn, G1 = ctx.bases_split_at(gens[kind], shape.R(kind))
        splits += [Gn, G1]
        xy, _ = ctx.commit_table(Gn, tab, None, 1 << pm.factored_lens(shape.ell[kind])[0], shape.R(kind))
        comm_h.append(ctx.bases_upload(xy))
    dense.free(); srs.free()

    def hyrax():
        t = sbn.Transcript(TR)
        return ctx.sparse_eval_verify(nx, ny, N, shape.cells, b, comm_h[0], comm_h[1], rx, ry, evals, gens["ops"], gens["mem"], gens["derefs"], p_hyrax, t), t.state()

    def kzg():
        t = sbn.Transcript(TR)
        return ctx.sparse_eval_verify_kzg(nx, ny, N, shape.cells, b, comm_h[0], comm_h[1], rx, ry, evals, gens["ops"], gens["mem"], g2, tau_g2, p_kzg, t), t.state()
    assert hyrax() == (True, th.state()) and kzg() == (True, tk.state()), "a one-call verifier refuses its prover's proof"
    bad = bytearray(p_kzg); bad[-32] ^= 1
    assert not ctx.sparse_eval_verify_kzg(nx, ny, N, shape.cells, b, comm_h[0], comm_h[1], rx, ry, evals, gens["ops"], gens["mem"], g2, tau_g2, bytes(bad), sbn.Transcript(TR))
    hy, kz = [], []
    for _ in range(passes):
        ctx.sync()
        t0 = time.perf_counter(); hyrax(); hy.append((time.perf_counter() - t0) * 1e3)
        t0 = time.perf_counter(); kzg(); kz.append((time.perf_counter() - t0) * 1e3)
    ctx.prof_enable(True); ctx.prof_reset()
    kzg()
    prof = {n: [round(ms, 3), int(l)] for n, (ms, l) in sorted(ctx.prof_get().items(), key=lambda kv: -kv[1][0])}
    ctx.prof_enable(False)
    for h in comm_h + splits + list(gens.values()):
        h.free()
    return {"bench": "sparse_eval_verify_kzg", "num_vars_x": nx, "num_vars_y": ny, "num_ops": N, "batch": b, "proof_bytes": len(p_kzg), "passes": passes,
            "kzg_one_call_ms": [round(min(kz), 3), round(max(kz), 3)], "hyrax_one_call_ms": [round(min(hy), 3), round(max(hy), 3)], "kzg_kernel_ms_launches": prof}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--passes", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--checks", default="1,64,1024,4096")
    ap.add_argument("--small", action="store_true")
    ap.add_argument("--no-sparse", action="store_true")
    a = ap.parse_args()
    sbn = load_pkg(); ctx = sbn.Context(0)
    kat = json.load(open(os.path.join(ROOT, "tests", "golden", "pairing_kat.json")))
    tau = int(kat["tau"], 16).to_bytes(32, "little")
    g2, tau_g2 = ctx.g2_prepare(bytes.fromhex(kat["g2"]["gen"])), ctx.g2_prepare(bytes.fromhex(kat["g2"]["tau"]))
    prep = []
    for _ in range(a.passes):                                         # sbn_g2_prepare: host work and an 11 KiB upload, once per SRS point
        t0 = time.perf_counter(); h = ctx.g2_prepare(bytes.fromhex(kat["g2"]["tau"])); prep.append(round((time.perf_counter() - t0) * 1e6, 1)); h.free()
    n = 1 << 10
    srs = ctx.kzg_srs_from_tau(tau, n)
    t = ctx.table_upload(bench.splitmix_scalars(n, 3))
    z = (123456789).to_bytes(32, "little")
    C, _ = ctx.kzg_commit(srs, t, n)
    ev, pi, _ = ctx.kzg_open(srs, t, n, z)
    bad = ((int.from_bytes(ev, "little") + 1) % (1 << 253)).to_bytes(32, "little")
    assert ctx.kzg_verify(g2, tau_g2, C, z, ev, pi) and not ctx.kzg_verify(g2, tau_g2, C, z, bad, pi), "verdicts"
    cases = {c["name"]: c for c in kat["cases"]}
    two, cancel = cases["two"], cases["cancel"]
    lines = {k: ctx.g2_prepare(bytes.fromhex(v)) for k, v in kat["g2"].items()}

    def products(nchecks):
        p, q, want = b"", [], []
        for i in range(nchecks):
            c = cancel if i % 7 == 3 else two
            p += b"".join(bytes.fromhex(x[0]) for x in c["terms"]); q += [lines[x[1]] for x in c["terms"]]; want.append(1 if c["is_one"] else 0)
        return p, q, [2] * nchecks, bytes(want)

    def timed(fn, reps):
        fn(); t0 = time.perf_counter()
        for _ in range(reps):
            fn()
        return (time.perf_counter() - t0) / reps * 1e6
    checks = [int(x) for x in a.checks.split(",")]
    args = {k: products(k) for k in checks}
    for k in checks:
        assert ctx.pairing_products(*args[k][:3], want_gt=False)[0] == args[k][3], "product verdicts"
    rows = []
    for p in range(a.passes):
        row = {"pass": p, "kzg_verify_us": round(timed(lambda: ctx.kzg_verify(g2, tau_g2, C, z, ev, pi), a.reps), 1)}
        for k in checks:
            us = timed(lambda: ctx.pairing_products(*args[k][:3], want_gt=False), max(2, a.reps // (1 + k // 256)))
            row["products_%d_us" % k] = round(us, 1); row["products_%d_checks_per_s" % k] = round(k / us * 1e6)
        rows.append(row); print(row, flush=True)
    kern = {}
    ctx.prof_enable(True)
    for name, fn in (("kzg_verify", lambda: ctx.kzg_verify(g2, tau_g2, C, z, ev, pi)), ("products_1", lambda: ctx.pairing_products(*args[checks[0]][:3], want_gt=False))):
        fn(); ctx.prof_reset(); fn()
        kern[name] = {k: {"us": round(ms * 1e3, 1), "launches": cnt} for k, (ms, cnt) in ctx.prof_get().items()}
    ctx.prof_enable(False)
    rng = lambda key: [min(r[key] for r in rows), max(r[key] for r in rows)]      # noqa: E731
    print(json.dumps({"bench": "kzg_verify", "reps": a.reps, "passes": rows, "range": {k: rng(k) for k in rows[0] if k != "pass"}, "g2_prepare_us": [min(prep), max(prep)],
                      "kernels_one_call": kern}))
    if not a.no_sparse:
        print(json.dumps(sparse(sbn, ctx, kat, g2, tau_g2, a.passes, a.small)), flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
