#!/usr/bin/env python3
"""ProductCircuitEvalProofBatched::prove from a compiled caller (harness/product_proof_bench.cpp -> libsbn_product_bench.so), three ways
over the same inputs and the same Merlin transcript:
    base_loop   the layer loop over the older entry points, linked against ANOTHER build of the library (--base-lib, e.g. the parent commit's)
    loop        the same loop on this build
    call        sbn_product_proof_prove on this build
The three alternate, `--rounds` times; every measurement is a fresh process (its own copy of the chosen library next to the driver, so that
exactly one build is loaded), one warm-up prove and `--reps` timed ones.  One JSON line per shape; medians in microseconds.

    python tools/bench_product_proof.py [--shapes ops,mem,small] [--rounds 3] [--reps 5] [--base-lib path/to/libsbn254_hip.so]

shapes: ops = 12 circuits of 2^22 + 6 dot-product circuits, mem = 4 circuits of 2^21, small = 12 + 6 with 11 layers, or n_circ:n_dotp:n_layers.
Without --base-lib only loop and call are run.  A kernel trace of one mode: put the profiler in front of
    python tools/bench_product_proof.py --child <lib> <mode> <n_circ> <n_dotp> <n_layers> <reps>"""
import argparse
import ctypes as C
import json
import os
import shutil
import statistics
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "spartan-bn254_amd")
SHAPES = {"ops": (12, 6, 22), "mem": (4, 0, 21), "small": (12, 6, 11)}


def child(lib, mode, n_circ, n_dotp, n_layers, reps):
    tmp = tempfile.mkdtemp(prefix="ppbench_")
    try:
        shutil.copy(lib, os.path.join(tmp, "libsbn254_hip.so"))
        shutil.copy(os.path.join(PKG, "libsbn_product_bench.so"), os.path.join(tmp, "libsbn_product_bench.so"))
        L = C.CDLL(os.path.join(tmp, "libsbn254_hip.so"), mode=C.RTLD_GLOBAL)
        B = C.CDLL(os.path.join(tmp, "libsbn_product_bench.so"))
        B.sbn_bench_product_proof.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_uint64)]
        L.sbn_last_error.restype = C.c_char_p
        ctx = C.c_void_p()
        if L.sbn_ctx_create(0, C.byref(ctx)):
            raise SystemExit("no context")
        out = {}
        for name, k in (("warm", 1), ("timed", reps)):
            us, dig = (C.c_double * k)(), C.c_uint64()
            rc = B.sbn_bench_product_proof(ctx, n_circ, n_dotp, n_layers, mode, k, us, C.byref(dig))
            if rc:
                raise SystemExit(f"bench driver rc={rc}: {L.sbn_last_error(ctx)}")
            out = {"us": list(us), "digest": f"{dig.value:016x}"}
        L.sbn_ctx_destroy.restype = None
        L.sbn_ctx_destroy(ctx)
        print(json.dumps(out), flush=True)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "--child":
        child(sys.argv[2], *[int(x) for x in sys.argv[3:8]])
        return
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="ops,mem,small")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--base-lib", default=None)
    args = ap.parse_args()
    this = os.path.join(PKG, "libsbn254_hip.so")
    variants = ([("base_loop", args.base_lib, 0)] if args.base_lib else []) + [("loop", this, 0), ("call", this, 1)]
    for name in args.shapes.split(","):
        shape = SHAPES[name] if name in SHAPES else tuple(int(x) for x in name.split(":"))
        med = {v[0]: [] for v in variants}; digs = set()
        for _ in range(args.rounds):
            for vname, lib, mode in variants:
                p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", lib, str(mode), *[str(x) for x in shape], str(args.reps)],
                                   capture_output=True, text=True, timeout=600)
                if p.returncode:
                    raise SystemExit(f"{vname} failed: {p.stdout[-400:]} {p.stderr[-400:]}")
                r = json.loads(p.stdout.strip().splitlines()[-1])
                med[vname].append(round(statistics.median(r["us"]), 1)); digs.add(r["digest"])
        out = {"bench": "product_proof", "shape": {"n_circ": shape[0], "n_dotp": shape[1], "n_layers": shape[2]}, "rounds": args.rounds, "reps": args.reps,
               "same_bytes": len(digs) == 1}
        for vname in med:
            out[vname + "_us"] = med[vname]; out[vname + "_us_median"] = statistics.median(med[vname])
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
