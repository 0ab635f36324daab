#!/usr/bin/env python3
"""A circuit from the bytes of a circom .r1cs file to resident handles on one MI355X at the keyless shape, two ways each:

    NIZK instance   today      the caller's parse into (rows, cols, vals) arrays (timed on its own, reported, not part of the comparison) + sbn_nizk_instance_new
                    from file  sbn_circom_r1cs_load + sbn_nizk_instance_from_circom
    SNARK encode    today      the same parse + sbn_snark_encode
                    from file  sbn_circom_r1cs_load + sbn_snark_encode_circom

    python tools/bench_circom.py [--log 20] [--passes 5] [--out profiles/r25_circom.jsonl]

The circuit is the synthetic raw circuit of tools/bench_snark.py (tests/r1cs_model.keyless_instance: 2^20 x 2^20, nnz 3,151,183 / 1,040,083 / 2,940,867) with
10 inputs, written as .r1cs bytes in memory: every matrix in constraint order, as a file holds it.  `--passes` alternating passes; both routes must give the
same matrices (A, B, C at one random point) and the same commitment bytes.  Then the kernels and launches of one call of each new entry point.
No time is gated: whatever the comparison shows is written down, a route that does not pay included."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from __graft_entry__ import load_pkg  # noqa: E402

R = 0x30644e72e131a029b85045b68181585d2833e84879b9709143e1f593f0000001
NUM_INPUTS = 10
DIGEST = bytes(range(32))


def span(xs):
    return [round(min(xs), 3), round(max(xs), 3)]


def timed(fn):
    t0 = time.perf_counter(); out = fn()
    return out, (time.perf_counter() - t0) * 1e3


def write_r1cs(np, num_cons, num_vars, num_inputs, mats):
    """raw matrices (columns vars | 1 | inputs, any entry order) -> the bytes of a .r1cs file as a numpy uint8 array, each matrix stably sorted by constraint"""
    srt = []
    for rows, cols, vals in mats:
        o = np.argsort(rows, kind="stable")
        c = cols[o].astype(np.int64)
        wire = np.where(c < num_vars, c + num_inputs + 1, c - num_vars).astype(np.uint32)      # the constant is wire 0, the inputs 1 .. num_inputs
        srt.append((rows[o].astype(np.int64), wire, np.ascontiguousarray(vals.reshape(-1, 32)[o])))
    counts = np.stack([np.bincount(r, minlength=num_cons) for r, _, _ in srt], axis=1).astype(np.int64)      # [constraint, matrix]
    flat = counts.reshape(-1)
    run_first = np.concatenate([[0], np.cumsum(flat)])
    total = int(run_first[-1])
    payload = np.zeros(4 * len(flat) + 36 * total, dtype=np.uint8)
    k = np.arange(len(flat), dtype=np.int64)
    at = 4 * k + 36 * run_first[:-1]
    payload[at[:, None] + np.arange(4)] = flat.astype("<u4").view(np.uint8).reshape(-1, 4)
    for m, (rows, wire, vals) in enumerate(srt):
        mat_first = np.concatenate([[0], np.cumsum(counts[:, m])])[:-1]
        e = np.arange(len(rows), dtype=np.int64) - mat_first[rows]
        pos = 4 * (3 * rows + m + 1) + 36 * (run_first[3 * rows + m] + e)
        rec = np.concatenate([wire.astype("<u4").view(np.uint8).reshape(-1, 4), vals], axis=1)
        for lo in range(0, len(rows), 1 << 20):
            payload[pos[lo:lo + (1 << 20), None] + np.arange(36)] = rec[lo:lo + (1 << 20)]
    le = lambda x, n: np.frombuffer(int(x).to_bytes(n, "little"), dtype=np.uint8)      # noqa: E731
    nw = 1 + num_inputs + num_vars
    head = np.concatenate([le(32, 4), le(R, 32), le(nw, 4), le(0, 4), le(num_inputs, 4), le(0, 4), le(nw, 8), le(num_cons, 4)])
    return np.concatenate([np.frombuffer(b"r1cs", dtype=np.uint8), le(1, 4), le(2, 4), le(1, 4), le(len(head), 8), head, le(2, 4), le(len(payload), 8), payload])


def parse_r1cs(np, data):
    """what a caller does today: the file's bytes -> (num_cons, num_vars, num_inputs, three (rows, raw cols, vals) arrays).  The walk over the counts is a
    Python loop; the records are gathered with numpy"""
    b = data.tobytes()
    off = 12
    secs = {}
    for _ in range(int.from_bytes(b[8:12], "little")):
        t, size = int.from_bytes(b[off:off + 4], "little"), int.from_bytes(b[off + 4:off + 12], "little")
        secs.setdefault(t, (off + 12, size)); off += 12 + size
    h = secs[1][0] + 36
    nw, npo, npi = (int.from_bytes(b[h + 4 * i:h + 4 * i + 4], "little") for i in range(3))
    nc = int.from_bytes(b[h + 24:h + 28], "little")
    ni = npo + npi
    nv = nw - 1 - ni
    p0 = secs[2][0]
    pos, starts, cnts = p0, [], []
    for _ in range(3 * nc):
        n = int.from_bytes(b[pos:pos + 4], "little")
        starts.append(pos + 4); cnts.append(n); pos += 4 + 36 * n
    starts, cnts = np.array(starts, dtype=np.int64), np.array(cnts, dtype=np.int64)
    out = []
    for m in range(3):
        c, s = cnts[m::3], starts[m::3]
        rows = np.repeat(np.arange(nc, dtype=np.uint32), c)
        first = np.concatenate([[0], np.cumsum(c)])[:-1]
        at = np.repeat(s, c) + 36 * (np.arange(len(rows), dtype=np.int64) - np.repeat(first, c))
        rec = np.empty((len(rows), 36), dtype=np.uint8)
        for lo in range(0, len(rows), 1 << 20):
            rec[lo:lo + (1 << 20)] = data[at[lo:lo + (1 << 20), None] + np.arange(36)]
        wire = np.ascontiguousarray(rec[:, :4]).view("<u4").reshape(-1).astype(np.int64)
        cols = np.where(wire == 0, nv, np.where(wire <= ni, nv + wire, wire - ni - 1)).astype(np.uint32)      # raw: vars | 1 | inputs
        out.append((rows, cols, np.ascontiguousarray(rec[:, 4:])))
    return nc, nv, ni, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log", type=int, default=20, help="20: the keyless shape as it is; smaller: the same recipe scaled down (a quick look, not a figure)")
    ap.add_argument("--passes", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import numpy as np
    import r1cs_model as rm
    sbn = load_pkg()
    rng = np.random.default_rng(25)
    if a.log == rm.KEYLESS_LOG:
        n, _, mats = rm.keyless_instance()
        real = rm.KEYLESS_REAL_ROWS
    else:
        n = 1 << a.log; real = n - n // 128
        mats = [(rng.integers(0, real, k * n, dtype=np.uint32), rng.integers(0, 2 * n, k * n, dtype=np.uint32), rm.random_vals(rng, k * n)) for k in (3, 1, 2)]
    live = n + 1 + NUM_INPUTS
    mats = [(r, np.where(c >= live, c - live, c).astype(np.uint32), v) for r, c, v in mats]      # raw columns: vars | 1 | inputs
    data, write_ms = timed(lambda: write_r1cs(np, real, n, NUM_INPUTS, mats))
    (nc, nv, ni, parsed), parse_ms = timed(lambda: parse_r1cs(np, data))
    assert (nc, nv, ni) == (real, n, NUM_INPUTS)
    nnz = [len(m[0]) for m in parsed]
    ctx = sbn.Context(0)
    lines = []
    try:
        gens = ctx.snark_gens_new(nc, nv, ni, max(nnz))
        point = rm.random_vals(rng, 2 * a.log + 1).tobytes()
        rx, ry = point[:32 * a.log], point[32 * a.log:]

        def nizk_today():
            return ctx.nizk_instance_new(nc, nv, ni, parsed, DIGEST)

        def nizk_file():
            f = ctx.circom_r1cs_load(data)
            try:
                return ctx.nizk_instance_from_circom(f, DIGEST)
            finally:
                f.free()

        def enc_today():
            return ctx.snark_encode(nc, nv, ni, parsed, gens)

        def enc_file():
            f = ctx.circom_r1cs_load(data)
            try:
                return ctx.snark_encode_circom(f, gens)
            finally:
                f.free()

        # warm-up of all four (workspaces, derived generator sets), and that the two routes agree
        ia, ib, ka, kb = nizk_today(), nizk_file(), enc_today(), enc_file()
        assert ctx.r1cs_evaluate(ia.r1cs, rx, ry) == ctx.r1cs_evaluate(ib.r1cs, rx, ry), "the two routes give other matrices"
        assert ka.comm() == kb.comm(), "the two routes give other commitments"
        for h in (ia, ib, ka, kb):
            h.free()
        t = {k: [] for k in ("nizk_today", "nizk_file", "enc_today", "enc_file", "load")}
        for _ in range(a.passes):                                     # alternating: other work shares the host
            for name, fn in (("nizk_today", nizk_today), ("nizk_file", nizk_file), ("enc_today", enc_today), ("enc_file", enc_file)):
                ctx.sync()
                h, ms = timed(fn)
                h.free()
                t[name].append(ms)
            ctx.sync()
            f, ms = timed(lambda: ctx.circom_r1cs_load(data))
            f.free()
            t["load"].append(ms)
        out = {"bench": "circom", "log": a.log, "num_cons": nc, "num_vars": nv, "num_inputs": ni, "nnz": nnz, "file_bytes": int(len(data)), "passes": a.passes,
               "caller_parse_ms_not_compared": round(parse_ms, 1), "file_write_ms": round(write_ms, 1),
               "nizk_instance_new_ms": span(t["nizk_today"]), "load_plus_nizk_instance_from_circom_ms": span(t["nizk_file"]),
               "snark_encode_ms": span(t["enc_today"]), "load_plus_snark_encode_circom_ms": span(t["enc_file"]), "circom_r1cs_load_alone_ms": span(t["load"]),
               "same_matrices_and_commitment": True}
        lines.append(out)
        print(json.dumps(out), flush=True)
        f = ctx.circom_r1cs_load(data)
        for name, fn in (("circom_r1cs_load_kernels", lambda: ctx.circom_r1cs_load(data)), ("nizk_instance_from_circom_kernels", lambda: ctx.nizk_instance_from_circom(f, DIGEST)),
                         ("snark_encode_circom_kernels", lambda: ctx.snark_encode_circom(f, gens))):
            ctx.prof_enable(True); ctx.prof_reset()
            try:
                fn().free()
                prof = ctx.prof_get()
            finally:
                ctx.prof_enable(False)
            st = {"bench": name, "launches": int(sum(l for _, l in prof.values())), "kernel_ms_launches": {k: [round(ms, 3), int(l)] for k, (ms, l) in sorted(prof.items(), key=lambda kv: -kv[1][0])}}
            lines.append(st)
            print(json.dumps(st), flush=True)
        f.free(); gens.free()
    finally:
        ctx.close()
    if a.out:
        with open(a.out, "w") as f:
            for ln in lines:
                f.write(json.dumps(ln) + "\n")


if __name__ == "__main__":
    main()
