#!/usr/bin/env python3
"""MultiSparseMatPolynomialAsDense on one device at the keyless shape: sbn_dense_build, the two encode-time commitments on its tables,
and the route a caller had before the call existed.

    python tools/bench_dense.py [--reps 3] [--seed 1] [--out profiles/r07_dense_bench.jsonl] [--no-host-route]

The instance is tests/r1cs_model.py's synthetic keyless-shaped one (num_vars_x = 20, num_vars_y = 21, nnz 3,151,183 / 1,040,083 /
2,940,867): N = 2^22 ops per matrix, 2^21 cells, comb_ops 2^26 entries (2 GiB), comb_mem 2^22.
Writes one JSON line (also appended to --out):
  build_device_ms / build_kernels_ms   device time of one sbn_dense_build by HIP events, total and per kernel name (best total of --reps)
  build_wall_ms                        the same call by the wall clock: validation, upload of the triplets, kernels
  tables_bytes_per_s                   (comb_ops + comb_mem bytes written + the u32 arrays and values read) / time of k_dense_tables
  sort_pass_bytes_per_s                bytes one radix pass moves (keys read twice, keys + indices written, indices read) / (time of the
                                       hist + scan + scatter kernels / passes)
  commit_ops_ms / commit_mem_ms        sbn_commit_table of the real comb_ops (8192 x 8192) and comb_mem (2048 x 2048), wall clock, best of --reps,
                                       bucket method (no lookup table)
  host_route_ms                        numpy ranks (stable argsort), expansion to 32-byte scalars and sbn_table_upload / sbn_dev_upload of the
                                       same data: {ranks, expand, upload, total}
Yardsticks: the reference publishes 60.7 s for encode; the two commitments were measured at 41.2 + 4.8 ms on uniform scalars."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402

import dense_model as dm  # noqa: E402
import r1cs_model as rm  # noqa: E402


def ints_as_scalars(a):
    out = np.zeros((len(a), 8), np.uint32)
    out[:, 0] = a
    return out.view(np.uint8).reshape(-1)


def host_route(ctx, nx, ny, mats):
    """what a caller did before sbn_dense_build: ranks on the host, 32-byte scalars, uploads -> times in ms"""
    t0 = time.perf_counter()
    N, cells, addr, read_ts, audit = dm.numpy_expectation(nx, ny, mats)
    t1 = time.perf_counter()
    ops = np.zeros((16 * N, 32), np.uint8)
    for g, grp in enumerate((addr[0], read_ts[0], addr[1], read_ts[1])):
        for k in range(3):
            ops[(3 * g + k) * N:(3 * g + k + 1) * N] = ints_as_scalars(grp[k]).reshape(N, 32)
    for k in range(3):
        v = mats[k][2]; ops[(12 + k) * N:(12 + k) * N + len(v)] = v
    mem = ints_as_scalars(np.concatenate(audit))
    t2 = time.perf_counter()
    t_ops = ctx.table_upload(ops.reshape(-1)); t_mem = ctx.table_upload(mem)
    d = ctx.dev_alloc(4 * (12 * N + 2 * cells))
    off = 0
    for arr in (addr[0], read_ts[0], addr[1], read_ts[1]):
        ctx.dev_upload(d + off, np.ascontiguousarray(arr).reshape(-1)); off += 4 * 3 * N
    ctx.dev_upload(d + off, np.concatenate(audit))
    ctx.sync()
    t3 = time.perf_counter()
    t_ops.free(); t_mem.free(); ctx.dev_free(d)
    return {"ranks": round((t1 - t0) * 1e3, 1), "expand": round((t2 - t1) * 1e3, 1), "upload": round((t3 - t2) * 1e3, 1), "total": round((t3 - t0) * 1e3, 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r07_dense_bench.jsonl"))
    ap.add_argument("--no-host-route", action="store_true")
    a = ap.parse_args()
    import __graft_entry__ as ge
    sbn = ge.load_pkg()
    nc, nv, mats = rm.keyless_instance(a.seed)
    nx, ny = nc.bit_length() - 1, (2 * nv).bit_length() - 1
    nnz = sum(len(m[0]) for m in mats)
    ctx = sbn.Context(0)
    try:
        ctx.dense_build(nx, ny, mats).free()                                   # warm-up: workspace, table cache
        best = None
        for _ in range(a.reps):
            ctx.prof_reset(); ctx.prof_enable(True)
            t0 = time.perf_counter(); h = ctx.dense_build(nx, ny, mats); wall = (time.perf_counter() - t0) * 1e3
            prof = {k: v for k, v in ctx.prof_get().items() if k.startswith("k_dense")}; ctx.prof_enable(False)
            dev = sum(ms for ms, _ in prof.values())
            if best is None or dev < best[0]:
                best = (dev, prof, wall)
            else:
                best = (best[0], best[1], min(best[2], wall))
            h.free()
        dev, prof, wall = best
        h = ctx.dense_build(nx, ny, mats)
        N, cells, M = h.num_ops, h.num_cells, h.batch * h.num_ops
        passes = prof["k_dense_scatter"][1] // 2
        tables_bytes = 32 * (len(h.comb_ops) + len(h.comb_mem)) + 4 * (4 * M + 2 * cells) + 32 * nnz
        pass_bytes = 4 * M * 5
        sort_ms = sum(prof[k][0] for k in ("k_dense_hist", "k_dense_scan", "k_dense_scan_top", "k_dense_scatter")) / (2 * passes)
        commits = {}
        for name, t, lg in (("commit_ops_ms", h.comb_ops, 26), ("commit_mem_ms", h.comb_mem, 22)):
            lv, rv = sbn.factored_lens(lg)
            bases, _ = ctx.gens_new(1 << rv, b"gens_r1cs_eval", want_points=False)
            ts = []
            for _ in range(a.reps + 1):
                t0 = time.perf_counter(); ctx.commit_table(bases, t, None, 1 << lv, 1 << rv); ts.append((time.perf_counter() - t0) * 1e3)
            commits[name] = round(min(ts[1:]), 2)
            bases.free()
        h.free()
        res = {"workload": "dense", "num_vars_x": nx, "num_vars_y": ny, "nnz": nnz, "num_ops": N, "num_cells": cells, "sort_passes_per_side": passes,
               "build_device_ms": round(dev, 3), "build_wall_ms": round(wall, 1),
               "build_kernels_ms": {k: [round(ms, 3), int(n)] for k, (ms, n) in sorted(prof.items())},
               "tables_bytes_per_s": round(tables_bytes / (prof["k_dense_tables"][0] * 1e-3)),
               "sort_pass_ms": round(sort_ms, 3), "sort_pass_bytes_per_s": round(pass_bytes / (sort_ms * 1e-3)),
               **commits, "reference_encode_ms": 60700.0, "commits_on_uniform_scalars_ms": [41.2, 4.8]}
        if not a.no_host_route:
            res["host_route_ms"] = host_route(ctx, nx, ny, mats)
        line = json.dumps(res)
        print(line)
        if a.out:
            with open(a.out, "a") as f:
                f.write(line + "\n")
    finally:
        ctx.close()


if __name__ == "__main__":
    main()
