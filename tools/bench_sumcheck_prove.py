#!/usr/bin/env python3
"""One batched cubic sumcheck, transcript included: the round-by-round loop (sbn_sumcheck_round + the transcript on the host) against
sbn_sumcheck_prove (all rounds queued, transcript step on the device), both driven from compiled code
(harness/sumcheck_prove_bench.cpp -> libsbn_prove_bench.so).  The two modes alternate, `--pairs` times, `--reps` sumchecks each;
sbn_sumcheck_begin (round 0, identical in both) is timed apart.  One JSON line per shape.

    python tools/bench_sumcheck_prove.py [--shapes a,b] [--pairs 3] [--reps 20] [--prof]

shapes: a = 12 + 6 instances of 2^21 (21 rounds), b = 12 + 6 of 2^10 (10 rounds), or n_par:n_seq:logn.
--prof adds the library's per-kernel event times of one prove call per shape (coarse for kernels of a few microseconds)."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from __graft_entry__ import load_pkg  # noqa: E402

SHAPES = {"a": (12, 6, 21), "b": (12, 6, 10)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="a,b")
    ap.add_argument("--pairs", type=int, default=3)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--prof", action="store_true")
    args = ap.parse_args()
    sbn = load_pkg()
    sbn.lib()
    B = C.CDLL(os.path.join(os.path.dirname(sbn.lib_path()), "libsbn_prove_bench.so"))
    B.sbn_bench_sumcheck_prove.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_uint64)]
    ctx = sbn.Context(0)
    try:
        for name in args.shapes.split(","):
            n_par, n_seq, logn = SHAPES[name] if name in SHAPES else tuple(int(x) for x in name.split(":"))
            reps = args.reps if logn < 18 else max(3, args.reps // 4)

            def run(mode, reps=reps):
                us, bus, dig = (C.c_double * reps)(), (C.c_double * reps)(), C.c_uint64()
                rc = B.sbn_bench_sumcheck_prove(ctx.h, n_par, n_seq, logn, mode, reps, us, bus, C.byref(dig))
                if rc:
                    raise SystemExit(f"bench driver rc={rc}")
                return list(us), list(bus), dig.value
            run(0, 2); run(1, 2)                                     # warm-up: allocations, code objects
            loop, prove, begin, digs = [], [], [], set()
            for _ in range(args.pairs):
                for mode, dst in ((0, loop), (1, prove)):
                    us, bus, d = run(mode)
                    dst.append(statistics.median(us)); begin.append(statistics.median(bus)); digs.add(d)
            out = {"bench": "sumcheck_prove", "shape": {"n_par": n_par, "n_seq": n_seq, "log2_len": logn}, "pairs": args.pairs, "reps": reps,
                   "loop_us": [round(x, 1) for x in loop], "prove_us": [round(x, 1) for x in prove], "begin_us_median": round(statistics.median(begin), 1),
                   "loop_us_per_round": round(statistics.median(loop) / logn, 2), "prove_us_per_round": round(statistics.median(prove) / logn, 2),
                   "same_bytes": len(digs) == 1}
            if args.prof:
                ctx.prof_enable(True); ctx.prof_reset()
                run(1, 1)
                out["prove_kernels"] = {k: {"ms": round(ms, 4), "launches": n} for k, (ms, n) in ctx.prof_get().items()}
                ctx.prof_enable(False)
            print(json.dumps(out), flush=True)
    finally:
        ctx.close()


if __name__ == "__main__":
    main()
