#!/usr/bin/env python3
"""The R1CS matrices on one device at the keyless shape: upload, multiply (Az, Bz, Cz), the phase-2 table and evaluate.

    python tools/bench_r1cs.py [--reps 5] [--seed 1]

The instance is tests/r1cs_model.py's synthetic keyless-shaped one: num_cons = num_vars = 2^20, nnz A / B / C = 3,151,183 / 1,040,083 /
2,940,867, half of A's real rows in the constant column, one row of 2^16 entries, rows from 1,040,083 on empty.
Prints one JSON line: upload_ms (host sort + copies + conversion, wall clock), per call the device time of its kernels by HIP events
(best of --reps; eval_table and evaluate include building their eq tables) and the wall time, the SpMV kernels' achieved bytes/s over
the streamed arrays (column indices and values, 36 B per non-zero, plus 4 B per row end), and identities_ok: the phase-2 claim
identities <ABC, z> = sum_M r_M <eq(rx), Mz> (r1csproof.rs:373) and <ABC, eq(ry)> = sum_M r_M M(rx, ry), checked on the device.
The reference publishes 0.36 s for "Instance evaluations" (BENCHMARK_RESULTS.md); its multiply_vec and eval-table loops are not
published separately."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402

import r1cs_model as rm  # noqa: E402

R = rm.R


def b32(v):
    return int(v).to_bytes(32, "little")


def timed(ctx, fn, reps, prefix="k_r1cs_spmv"):
    """-> (best device ms of all kernels, best device ms of the SpMV kernels, best wall ms, last result)"""
    dev, spmv, wall, out = [], [], [], None
    for _ in range(reps):
        ctx.prof_reset(); ctx.prof_enable(True)
        t0 = time.perf_counter(); res = fn(); ctx.sync(); wall.append((time.perf_counter() - t0) * 1e3)
        prof = ctx.prof_get(); ctx.prof_enable(False)
        dev.append(sum(ms for ms, _ in prof.values()))
        spmv.append(sum(ms for k, (ms, _) in prof.items() if k.startswith(prefix)))
        if out is not None:
            for t in (out if isinstance(out, list) else [out]):
                if hasattr(t, "free"):
                    t.free()
        out = list(res) if isinstance(res, tuple) and hasattr(res[0], "free") else res
    return min(dev), min(spmv), min(wall), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--seed", type=int, default=1)
    a = ap.parse_args()
    import __graft_entry__ as ge
    sbn = ge.load_pkg()
    nc, nv, mats = rm.keyless_instance(a.seed)
    nnz = sum(len(m[0]) for m in mats)
    rng = np.random.default_rng(a.seed + 1)
    zb = rm.random_vals(rng, 2 * nv).tobytes()
    rx = [int(x) % R for x in rm.vals_as_ints(rm.random_vals(rng, 20))]
    ry = [int(x) % R for x in rm.vals_as_ints(rm.random_vals(rng, 21))]
    rABC = [int(x) % R for x in rm.vals_as_ints(rm.random_vals(rng, 3))]
    rxb, ryb = b"".join(b32(v) for v in rx), b"".join(b32(v) for v in ry)
    ctx = sbn.Context(0)
    tabs = []
    try:
        t0 = time.perf_counter()
        h = ctx.r1cs_upload(nc, nv, mats)
        ctx.sync()
        upload_ms = (time.perf_counter() - t0) * 1e3
        tz = ctx.table_upload(zb); tabs.append(tz)
        mul = ctx.r1cs_multiply(h, tz)                                          # warm-up: workspaces, table cache
        for t in mul:
            t.free()
        mul_dev, mul_spmv, mul_wall, mul = timed(ctx, lambda: ctx.r1cs_multiply(h, tz), a.reps)
        tabs += mul
        et_dev, et_spmv, et_wall, abc = timed(ctx, lambda: ctx.r1cs_eval_table(h, rxb, *(b32(v) for v in rABC)), a.reps)
        tabs.append(abc)
        ev_dev, ev_spmv, ev_wall, ev = timed(ctx, lambda: ctx.r1cs_evaluate(h, rxb, ryb), a.reps)
        ex = ctx.eq_evals(rxb); ey = ctx.eq_evals(ryb); tabs += [ex, ey]
        dots = [int.from_bytes(ctx.table_dot(ex, t), "little") for t in mul]
        ok1 = int.from_bytes(ctx.table_dot(abc, tz), "little") == sum(r * d for r, d in zip(rABC, dots)) % R
        evi = [int.from_bytes(x, "little") for x in ev]
        ok2 = int.from_bytes(ctx.table_dot(abc, ey), "little") == sum(r * e for r, e in zip(rABC, evi)) % R
        h.free()
        streamed_rows = 36 * nnz + 4 * 3 * nc           # row-major copy: multiply and evaluate
        streamed_cols = 36 * nnz + 4 * 2 * nv           # column-major copy: eval_table
        res = {"workload": "r1cs", "num_cons": nc, "num_vars": nv, "nnz": nnz, "upload_ms": round(upload_ms, 1),
               "multiply_ms": round(mul_dev, 3), "eval_table_ms": round(et_dev, 3), "evaluate_ms": round(ev_dev, 3),
               "multiply_wall_ms": round(mul_wall, 3), "eval_table_wall_ms": round(et_wall, 3), "evaluate_wall_ms": round(ev_wall, 3),
               "spmv_ms": {"multiply": round(mul_spmv, 3), "eval_table": round(et_spmv, 3), "evaluate": round(ev_spmv, 3)},
               "streamed_bytes_per_s": {"multiply": round(streamed_rows / (mul_spmv * 1e-3)), "eval_table": round(streamed_cols / (et_spmv * 1e-3)),
                                        "evaluate": round(streamed_rows / (ev_spmv * 1e-3))},
               "identities_ok": bool(ok1 and ok2), "reference_instance_evaluations_ms": 360.0}
        print(json.dumps(res))
    finally:
        for t in tabs:
            t.free()
        ctx.close()


if __name__ == "__main__":
    main()
