#!/usr/bin/env python3
"""sbn_sparse_eval_prove_kzg — the KZG build's SparseMatPolyEvalProof::prove in one call, with and without a derefs key — against the same
proof assembled through the entry points that existed before it (tests/sparse_eval_kzg_loop.py: sbn_kzg_commit and sbn_kzg_open on the full
padded derefs table), and the key on its own: its build, its length, and sbn_derefs_key_commit against sbn_kzg_commit of the gathered table.

Shape: the keyless synthetic instance of tools/bench_sparse_eval.py (N = 2^22 operations, 2^21 cells), batch 3, an SRS of 2^25 + 1 points from
a known tau; rx and ry uniform (every eq value non-zero, as under a verifier's challenges).  The three proof legs run on one context, alternating, `--pairs` times; each pass is the median of `--reps` proofs; all legs must
end with the same bytes and the same transcript.  Wall time from the host around a stream synchronisation.  Raw lines go to
profiles/r13_sparse_eval_kzg.jsonl.

Usage: python tools/bench_sparse_eval_kzg.py [--small] [--pairs 5] [--reps 5] [--skip-loop]
       (--small: 2^12 constraints and variables, a functional check)"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402

import r1cs_model as rm  # noqa: E402
import sparse_eval_kzg_loop as loop  # noqa: E402

TAU = (0x1f2e3d4c5b6a79881726354453627180 << 64 | 0x0123456789abcdef).to_bytes(32, "little")


def timed(ctx, fn):
    ctx.sync(); t0 = time.perf_counter(); out = fn(); ctx.sync()
    return (time.perf_counter() - t0) * 1e3, out


def uniform_vals(rng, n):
    """n scalars uniform below 2^253, as bytes.  NOT r1cs_model.random_vals: a quarter of its values are 1 and a quarter r - 1, and a coordinate of
    rx or ry equal to 1 (or 0) zeroes half of its eq table — with 20 coordinates drawn that way 31 of 32 derefs are zero and every derefs MSM
    skips them, which no verifier challenge does"""
    limbs = rng.integers(0, 2**64, size=(n, 4), dtype=np.uint64)
    limbs[:, 3] &= np.uint64((1 << 61) - 1)
    return limbs.view(np.uint8).reshape(n, 32).tobytes()


def rng_of(passes, name):
    return [min(p[name] for p in passes), max(p[name] for p in passes)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=5)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--small", action="store_true")
    ap.add_argument("--skip-loop", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r13_sparse_eval_kzg.jsonl"))
    a = ap.parse_args()
    import __graft_entry__ as ge
    sbn = ge.load_pkg()
    ctx = sbn.Context(0)

    def emit(res):
        line = json.dumps(res)
        print(line, flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(line + "\n")
    if a.small:
        nx = ny = 12
        mats = loop.random_mats(nx, ny, 1 << 12, 3, a.seed)
    else:
        nc, nv, mats = rm.keyless_instance(a.seed)
        nx, ny = nc.bit_length() - 1, (2 * nv).bit_length() - 1
    dense = ctx.dense_build(nx, ny, mats)
    N, b = dense.num_ops, dense.batch
    n_rnd, n_proof = sbn.sparse_eval_kzg_sizes(nx, ny, N, b)
    n, m = N.bit_length() - 1, max(nx, ny)
    ell = {"ops": n + loop.npo2(5 * b).bit_length() - 1, "mem": m + 1}
    n_d, n_prefix = loop.npo2(2 * b) * N, 2 * b * N
    gens = {k: ctx.gens_new((1 << (e - e // 2)) + 1, b"gens_r1cs_eval", want_points=False)[0] for k, e in ell.items()}
    ms_srs, srs = timed(ctx, lambda: ctx.kzg_srs_from_tau(TAU, n_d + 1))
    rng = np.random.default_rng(a.seed + 1)
    rx, ry = uniform_vals(rng, nx), uniform_vals(rng, ny)
    rnd = rm.random_vals(rng, n_rnd).tobytes()
    lg = loop.LoopGens(ctx, None, 0, N)
    key = None
    held = []
    try:
        # ---- the key on its own
        builds = []
        for _ in range(3):
            if key is not None:
                key.free()
            ms, key = timed(ctx, lambda: ctx.derefs_key_build(dense, srs))
            builds.append(round(ms, 3))
        acc = ctx.prof_last_acc()
        mem_rx, mem_ry, derefs = loop._derefs(ctx, dense, rx, ry); held += [mem_rx, mem_ry, derefs]
        same_point = ctx.derefs_key_commit(key, mem_rx, mem_ry) == ctx.kzg_commit(srs, derefs, n_d)      # warm-up of both
        passes = []
        for _ in range(a.pairs):
            row = {}
            for name, fn in (("key_commit_ms", lambda: ctx.derefs_key_commit(key, mem_rx, mem_ry)), ("kzg_commit_n_d_ms", lambda: ctx.kzg_commit(srs, derefs, n_d)),
                             ("kzg_commit_n_prefix_ms", lambda: ctx.kzg_commit(srs, derefs, n_prefix))):
                row[name] = round(statistics.median(timed(ctx, fn)[0] for _ in range(a.reps)), 3)
            passes.append(row)
        emit({"workload": "derefs_key", "num_ops": N, "cells": dense.num_cells, "batch": b, "n_d": n_d, "n_prefix": n_prefix, "key_len": len(key),
              "srs_from_tau_ms": round(ms_srs, 1), "key_build_ms": builds, "key_build_acc": acc, "same_point": bool(same_point), "passes": passes,
              "key_commit_ms_range": rng_of(passes, "key_commit_ms"), "kzg_commit_n_d_ms_range": rng_of(passes, "kzg_commit_n_d_ms"),
              "kzg_commit_n_prefix_ms_range": rng_of(passes, "kzg_commit_n_prefix_ms"),
              "note": "one run on one MI355X; wall time from the host around a stream synchronisation, medians per pass, legs alternating; key_build_ms: three builds in a row, the first one cold"})
        for t in held:
            t.free()
        held = []
        # ---- the proof
        evals = loop.evals_of(sbn, ctx, dense, rx, ry)

        def call(k):
            def f():
                tr = sbn.Transcript(b"bench sparse eval kzg")
                return ctx.sparse_eval_prove_kzg(dense, rx, ry, evals, gens["ops"], gens["mem"], srs, k, rnd, tr), tr.state()
            return f

        def many():
            tr = sbn.Transcript(b"bench sparse eval kzg")
            return loop.prove_loop(sbn, ctx, dense, rx, ry, evals, gens["ops"], gens["mem"], srs, lg, rnd, tr), tr.state()
        legs = [("one_call_key_ms", call(key)), ("one_call_no_key_ms", call(None))] + ([] if a.skip_loop else [("loop_ms", many)])
        ref = legs[0][1]()                                          # warm-up of every leg: workspace, table cache, derived generator sets
        same = all(fn() == ref for _, fn in legs[1:])
        passes = []
        for _ in range(a.pairs):
            row = {}
            for name, fn in legs:
                ts = []
                for _ in range(a.reps):
                    ms, out = timed(ctx, fn)
                    same = same and out == ref
                    ts.append(ms)
                row[name] = round(statistics.median(ts), 3)
            passes.append(row)
        res = {"workload": "sparse_eval_prove_kzg", "num_vars_x": nx, "num_vars_y": ny, "num_ops": N, "batch": b, "proof_bytes": n_proof, "rnd_scalars": n_rnd,
               "srs_points": n_d + 1, "key_len": len(key), "pairs": a.pairs, "reps_per_pass": a.reps, "passes": passes, "same_bytes_and_transcript": bool(same),
               "note": "one run on one MI355X; wall time from the host around a stream synchronisation, medians per pass, legs alternating"}
        for name, _ in legs:
            res[name + "_range"] = rng_of(passes, name)
        emit(res)
        if not (same and same_point):
            raise SystemExit("the legs do not give the same bytes")
    finally:
        for t in held:
            t.free()
        if key is not None:
            key.free()
        lg.free(); dense.free(); srs.free()
        for g in gens.values():
            g.free()
        ctx.close()


if __name__ == "__main__":
    main()
