#!/usr/bin/env python3
"""The verifier's short sums: ONE `sbn_g1_small_sums` call over `--sums` sums of `--terms` fresh points (one upload, one k_window_sums launch,
one hand-over, the fold on the host) against the same sums as one `sbn_msm` each (a bucket pipeline per sum: DESIGN §4.5 item 3).
`--passes` alternating passes on one box, each the mean of `--reps` calls from host pointers; then the HIP-event kernel totals of one call of
each route.  Every result is compared with the oracle's MSM before anything is timed.

    python tools/bench_small_sums.py [--sums 3] [--terms 30] [--passes 5] [--reps 50]
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
import oracle_lib as ol  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sums", type=int, default=3)
    ap.add_argument("--terms", type=int, default=30)
    ap.add_argument("--passes", type=int, default=5)
    ap.add_argument("--reps", type=int, default=50)
    a = ap.parse_args()
    sbn = load_pkg(); ctx = sbn.Context(0)
    n = a.sums * a.terms
    pts = ol.g1_mul_gen_batch(bench.splitmix_scalars(n, 5), 8)
    sc = bench.splitmix_scalars(n, 6)
    cut = lambda b, w, i: b[w * a.terms * i:w * a.terms * (i + 1)]      # noqa: E731
    want = [ol.msm_pippenger(cut(sc, 32, i), cut(pts, 64, i), 1) for i in range(a.sums)]

    def one_call():
        xy, _ = ctx.g1_small_sums(pts, sc, [a.terms] * a.sums)
        return [xy[64 * i:64 * i + 64] for i in range(a.sums)]

    def msms():
        return [ctx.msm(cut(sc, 32, i), cut(pts, 64, i))[0] for i in range(a.sums)]
    assert one_call() == want and msms() == want, "results differ from the oracle"

    def timed(fn):
        fn(); t0 = time.perf_counter()
        for _ in range(a.reps):
            fn()
        return (time.perf_counter() - t0) / a.reps * 1e6
    rows = []
    for p in range(a.passes):
        rows.append({"pass": p, "small_sums_us": round(timed(one_call), 1), "msm_each_us": round(timed(msms), 1)})
        print(rows[-1], flush=True)
    kern = {}
    ctx.prof_enable(True)
    for name, fn in (("small_sums", one_call), ("msm_each", msms)):
        fn(); ctx.prof_reset(); fn()
        kern[name] = {k: {"us": round(ms * 1e3, 1), "launches": cnt} for k, (ms, cnt) in ctx.prof_get().items()}
    ctx.prof_enable(False)
    med = lambda k: sorted(r[k] for r in rows)[len(rows) // 2]           # noqa: E731
    print(json.dumps({"bench": "small_sums", "sums": a.sums, "terms": a.terms, "reps": a.reps, "passes": rows,
                      "median_us": {"small_sums": med("small_sums_us"), "msm_each": med("msm_each_us")}, "kernels_one_call": kern}))
    ctx.close()


if __name__ == "__main__":
    main()
