#!/usr/bin/env python3
"""One Hyrax opening (PolyEvalProof::prove), Merlin transcript included: the loop through the piecewise calls (sbn_eq_evals, sbn_table_bound,
sbn_commit_table, sbn_msm, sbn_bullet_*, sbn_g1_compress, sbn_transcript_*; the caller's own Fr arithmetic) against sbn_polyeval_prove, both
driven from compiled code (harness/polyeval_bench.cpp -> libsbn_polyeval_bench.so).  The two legs alternate, `--pairs` times, `--reps` openings
each; handles, tables and derived generator sets are made outside the timed region.  One JSON line per size.

    python tools/bench_polyeval.py [--ells 25,20] [--pairs 3] [--reps 10]

ell = the polynomial's variables: R_size = 2^(ell - ell // 2) (25 -> 8192 with a 1 GiB table, 20 -> 1024)."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from __graft_entry__ import load_pkg  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ells", default="25,20")
    ap.add_argument("--pairs", type=int, default=3)
    ap.add_argument("--reps", type=int, default=10)
    args = ap.parse_args()
    sbn = load_pkg()
    sbn.lib()
    B = C.CDLL(os.path.join(os.path.dirname(sbn.lib_path()), "libsbn_polyeval_bench.so"))
    B.sbn_bench_polyeval.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_uint64)]
    ctx = sbn.Context(0)
    try:
        for ell in (int(x) for x in args.ells.split(",")):
            reps = args.reps

            def run(mode):
                us, host, dig = (C.c_double * reps)(), (C.c_double * (3 * reps))(), C.c_uint64()
                rc = B.sbn_bench_polyeval(ctx.h, ell, mode, reps, us, host, C.byref(dig))
                if rc:
                    raise SystemExit(f"bench driver rc={rc}: {sbn.lib().sbn_last_error(ctx.h).decode()}")
                return list(us), [list(host[3 * i:3 * i + 3]) for i in range(reps)], dig.value
            loop, one, digs, host = [], [], set(), []
            for _ in range(args.pairs):
                for mode, dst in ((0, loop), (1, one)):
                    us, h, d = run(mode)
                    dst.append(statistics.median(us)); digs.add(d)
                    if mode == 1:
                        host += h
            med = lambda k: round(statistics.median(x[k] for x in host), 1)      # noqa: E731
            out = {"bench": "polyeval_prove", "ell": ell, "R_size": 1 << (ell - ell // 2), "pairs": args.pairs, "reps": reps,
                   "loop_us": [round(x, 1) for x in loop], "one_call_us": [round(x, 1) for x in one],
                   "loop_us_median": round(statistics.median(loop), 1), "one_call_us_median": round(statistics.median(one), 1),
                   "loop_spread_us": round(max(loop) - min(loop), 1), "one_call_spread_us": round(max(one) - min(one), 1),
                   "host_R_us": med(0), "wait_first_commit_after_R_us": med(1), "absorb_Cx_Cy_a_vec_us": med(2), "same_bytes": len(digs) == 1}
            print(json.dumps(out), flush=True)
    finally:
        ctx.close()


if __name__ == "__main__":
    main()
