#!/usr/bin/env python3
"""sbn_sparse_eval_prove — SparseMatPolyEvalProof::prove in one call — against the same proof assembled through the entry points that existed
before it (tests/sparse_eval_loop.py), and the fused hashing pass sbn_hash_layer_pair_product against sbn_hash_layer_pair + sbn_product_layer.

Shape: the keyless synthetic instance of tools/bench_dense.py (2^20 constraints, 2^20 variables: N = 2^22 operations, 2^21 cells), batch 3.
Both legs run on one context, alternating, `--pairs` times; each pass is the median of `--reps` proofs; both legs must end with the same bytes
and the same transcript.  The construction comparison runs at n = 2^22 for both pair kinds, alternating passes, each the median of `--reps`
runs timed from the host around a stream synchronisation (call wall time, launch overhead included), plus one pass under the HIP-event
profiler for the kernels' own times.  Raw lines go to profiles/r12_sparse_eval.jsonl.

Usage: python tools/bench_sparse_eval.py [--small] [--pairs 5] [--reps 5] [--skip-proof] [--skip-construction]
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
import sparse_eval_loop as loop  # noqa: E402


def timed(ctx, fn):
    ctx.sync(); t0 = time.perf_counter(); out = fn(); ctx.sync()
    return (time.perf_counter() - t0) * 1e3, out


def bench_proof(sbn, ctx, a, emit):
    if a.small:
        nx = ny = 12
        mats = loop.random_mats(nx, ny, 1 << 12, 3, a.seed)
    else:
        nc, nv, mats = rm.keyless_instance(a.seed)
        nx, ny = nc.bit_length() - 1, (2 * nv).bit_length() - 1
    dense = ctx.dense_build(nx, ny, mats)
    N, b = dense.num_ops, dense.batch
    n_rnd, n_proof = sbn.sparse_eval_sizes(nx, ny, N, b)
    n, m = N.bit_length() - 1, max(nx, ny)
    ell = {"ops": n + loop.npo2(5 * b).bit_length() - 1, "mem": m + 1, "derefs": n + loop.npo2(2 * b).bit_length() - 1}
    gens = {k: ctx.gens_new((1 << (e - e // 2)) + 1, b"gens_r1cs_eval", want_points=False)[0] for k, e in ell.items()}
    rng = np.random.default_rng(a.seed + 1)
    rx, ry = rm.random_vals(rng, nx).tobytes(), rm.random_vals(rng, ny).tobytes()
    rnd = rm.random_vals(rng, n_rnd).tobytes()
    lg = loop.LoopGens(ctx, gens["derefs"], 1 << (ell["derefs"] - ell["derefs"] // 2), N)
    try:
        evals = loop.evals_of(sbn, ctx, dense, rx, ry)

        def one():
            tr = sbn.Transcript(b"bench sparse eval")
            return ctx.sparse_eval_prove(dense, rx, ry, evals, gens["ops"], gens["mem"], gens["derefs"], rnd, tr), tr.state()

        def many():
            tr = sbn.Transcript(b"bench sparse eval")
            return loop.prove_loop(sbn, ctx, dense, rx, ry, evals, gens["ops"], gens["mem"], gens["derefs"], lg, rnd, tr), tr.state()
        ref = one()                                             # warm-up of both legs: workspace, table cache, derived generator sets
        same = many() == ref
        passes = []
        for _ in range(a.pairs):
            row = {}
            for name, fn in (("one_call_ms", one), ("loop_ms", many)):
                ts = []
                for _ in range(a.reps):
                    ms, out = timed(ctx, fn)
                    same = same and out == ref
                    ts.append(ms)
                row[name] = round(statistics.median(ts), 3)
            passes.append(row)
        emit({"workload": "sparse_eval_prove", "num_vars_x": nx, "num_vars_y": ny, "num_ops": N, "batch": b, "proof_bytes": n_proof, "rnd_scalars": n_rnd,
              "pairs": a.pairs, "reps_per_pass": a.reps, "passes": passes, "same_bytes_and_transcript": bool(same),
              "one_call_ms_range": [min(p["one_call_ms"] for p in passes), max(p["one_call_ms"] for p in passes)],
              "loop_ms_range": [min(p["loop_ms"] for p in passes), max(p["loop_ms"] for p in passes)],
              "note": "one run on one MI355X; wall time from the host around a stream synchronisation, medians per pass, legs alternating"})
        if not same:
            raise SystemExit("the two legs do not give the same bytes")
    finally:
        lg.free(); dense.free()
        for g in gens.values():
            g.free()


def bench_construction(sbn, ctx, a, emit):
    """one pair of hashed sets and their first product layer at n entries: sbn_hash_layer_pair + 2 x sbn_product_layer against the fused call"""
    n = 1 << (12 if a.small else 22)
    rng = np.random.default_rng(a.seed + 2)
    val = ctx.table_upload(rm.random_vals(rng, n).tobytes())
    addr = rng.integers(0, n, n, dtype=np.uint64).astype(np.uint32)
    ts = rng.integers(0, 64, n, dtype=np.uint64).astype(np.uint32)
    d_addr, d_ts = ctx.dev_alloc(4 * n), ctx.dev_alloc(4 * n)
    ctx.dev_upload(d_addr, addr.tobytes()); ctx.dev_upload(d_ts, ts.tobytes())
    g, tau = rm.random_vals(rng, 1).tobytes(), rm.random_vals(rng, 1).tobytes()
    try:
        for kind, args in (("read / write", (d_addr, val, d_ts, 0, d_ts, 1)), ("init / audit", (None, val, None, 0, d_ts, 0))):
            def unfused():
                x, y = ctx.hash_layer_pair(*args, g, tau)
                px, py = ctx.product_layer(x), ctx.product_layer(y)
                return [x, y, px, py]

            def fused():
                return list(ctx.hash_layer_pair_product(*args, g, tau))
            passes = []
            for fn in (unfused, fused):                         # warm-up: the table cache holds the four buffers
                for t in fn():
                    t.free()
            for _ in range(a.pairs):
                row = {}
                for name, fn in (("pair_then_product_layers_ms", unfused), ("fused_ms", fused)):
                    ts_ = []
                    for _ in range(a.reps):
                        ms, tabs = timed(ctx, fn)
                        for t in tabs:
                            t.free()
                        ts_.append(ms)
                    row[name] = round(statistics.median(ts_), 4)
                passes.append(row)
            # the kernels alone, from the HIP-event profiler (it synchronises behind every call, so this is a pass of its own)
            kern = {}
            for name, fn in (("pair_then_product_layers", unfused), ("fused", fused)):
                ctx.sync(); ctx.prof_reset(); ctx.prof_enable(True)
                try:
                    for _ in range(a.reps * a.pairs):
                        for t in fn():
                            t.free()
                    kern[name] = {k: round(ms / cnt, 4) for k, (ms, cnt) in ctx.prof_get().items()}
                finally:
                    ctx.prof_enable(False)
            emit({"workload": "hash_pair_first_product_layer", "kind": kind, "n": n, "pairs": a.pairs, "reps_per_pass": a.reps, "passes": passes,
                  "kernel_event_ms_per_launch": kern,
                  "fused_over_unfused": round(statistics.median(p["fused_ms"] for p in passes) / statistics.median(p["pair_then_product_layers_ms"] for p in passes), 4),
                  "note": "one run on one MI355X; host wall time around a stream synchronisation (includes the calls' launch overhead), alternating passes"})
    finally:
        val.free(); ctx.dev_free(d_addr); ctx.dev_free(d_ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=5)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--small", action="store_true")
    ap.add_argument("--skip-proof", action="store_true")
    ap.add_argument("--skip-construction", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r12_sparse_eval.jsonl"))
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
    try:
        if not a.skip_construction:
            bench_construction(sbn, ctx, a, emit)
        if not a.skip_proof:
            bench_proof(sbn, ctx, a, emit)
    finally:
        ctx.close()


if __name__ == "__main__":
    main()
