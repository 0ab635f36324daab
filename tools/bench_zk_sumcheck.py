#!/usr/bin/env python3
"""One ZK sumcheck of R1CSProof::prove (prove_cubic_with_additive_term or prove_quad), Merlin transcript included: the round loop through the
piecewise calls (sbn_sc_eval_*, sbn_sc_bind_eval_*, sbn_bind_top_many, sbn_unipoly_from_evals, one-row sbn_commit_rows, sbn_g1_compress,
sbn_transcript_*; the caller's own Fr arithmetic) against sbn_zk_sumcheck_prove_r1cs / _quad, both driven from compiled code
(harness/zk_sumcheck_bench.cpp -> libsbn_zk_sumcheck_bench.so).  The loop runs twice: over the generator handles as sbn_gens_new gives them
(`loop_plain`) and with sbn_bases_precompute's lookup table on both (`loop`, 64 MiB each, what the one call gives its derived set) — the
second is the leg the one call is compared with.  The three legs alternate, `--pairs` times, `--reps` proofs each; handles, tables, lookup
tables and derived generator sets are made outside the timed region.  One JSON line per shape.

    python tools/bench_zk_sumcheck.py [--shapes r1cs:20,quad:21] [--pairs 3] [--reps 5]

A shape is kind:log2(table length): r1cs:20 is phase 1 of the keyless prove (4 x 2^20, 20 rounds), quad:21 its phase 2 (2 x 2^21, 21 rounds)."""
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
    ap.add_argument("--shapes", default="r1cs:20,quad:21")
    ap.add_argument("--pairs", type=int, default=3)
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    sbn = load_pkg()
    sbn.lib()
    B = C.CDLL(os.path.join(os.path.dirname(sbn.lib_path()), "libsbn_zk_sumcheck_bench.so"))
    B.sbn_bench_zk_sumcheck.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_uint64)]
    ctx = sbn.Context(0)
    try:
        for shape in args.shapes.split(","):
            kind, log_len = shape.split(":")
            log_len = int(log_len)
            reps = args.reps

            def run(mode):
                us, dig = (C.c_double * reps)(), C.c_uint64()
                rc = B.sbn_bench_zk_sumcheck(ctx.h, {"r1cs": 0, "quad": 1}[kind], log_len, mode, reps, us, C.byref(dig))
                if rc:
                    raise SystemExit(f"bench driver rc={rc}: {sbn.lib().sbn_last_error(ctx.h).decode()}")
                return list(us), dig.value
            plain, loop, one, digs = [], [], [], set()
            for _ in range(args.pairs):
                for mode, dst in ((0, plain), (2, loop), (1, one)):
                    us, d = run(mode)
                    dst.append(statistics.median(us)); digs.add(d)
            out = {"bench": "zk_sumcheck_prove", "kind": kind, "tables": 4 if kind == "r1cs" else 2, "log_len": log_len, "rounds": log_len,
                   "pairs": args.pairs, "reps": reps}
            for name, xs in (("loop_plain", plain), ("loop", loop), ("one_call", one)):
                out[name + "_us"] = [round(x, 1) for x in xs]
                out[name + "_us_median"] = round(statistics.median(xs), 1)
                out[name + "_spread_us"] = round(max(xs) - min(xs), 1)
            out["same_bytes"] = len(digs) == 1
            print(json.dumps(out), flush=True)
    finally:
        ctx.close()


if __name__ == "__main__":
    main()
