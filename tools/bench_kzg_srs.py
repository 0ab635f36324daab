#!/usr/bin/env python3
"""The KZG SRS as a file buffer on one MI355X, through ctypes:

    load        sbn_kzg_srs_load of the file's bytes               beside   sbn_kzg_srs_upload of the same points uncompressed (what a caller does
                                                                            today, AFTER arkworks has done the square roots on the CPU)
    save        sbn_kzg_srs_save
    check       sbn_kzg_srs_check                                  beside   one sbn_kzg_commit at the same n
    load+check  sbn_kzg_srs_load with SBN_SRS_CHECK
    kernels     k_srs_decompress per point at n and at 2^20, and k_g1_decompress through sbn_bases_from_compressed at 2^20 (HIP events around
                each launch; `--kernels-only` runs just these calls once each, for a kernel trace of their own)
    sweep       the load alone in fresh contexts over SBN_SRS_CHUNK

    python tools/bench_kzg_srs.py [--log 25] [--passes 5] [--sweep 14,16,18,20,22] [--out profiles/rNN_kzg_srs.jsonl] [--kernels-only]

n = 2^log + 1.  The file is made by sbn_kzg_srs_from_tau + sbn_kzg_srs_save, so the save runs at full size, and the loaded handle is compared with
the generated one by download before anything is timed: a loader that is fast and different is not faster.  `--passes` alternating passes.  No time
is gated here; the one condition (k_srs_decompress not slower per point than k_g1_decompress at 2^20) is reported as a boolean with both ranges."""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from __graft_entry__ import load_pkg  # noqa: E402

R = 0x30644e72e131a029b85045b68181585d2833e84879b9709143e1f593f0000001
TAU = (0x1d2c3b4a5968778695a4b3c2d1e0f1021324354657687980a9bacbdcedfe0f1 % R).to_bytes(32, "little")
RHO = (0x0123456789abcdef00112233445566778899aabbccddeeff1032547698badcf % R).to_bytes(32, "little")
BLOCK = 1 << 22      # points a download in the comparison


def span(xs, nd=3):
    return [round(min(xs), nd), round(max(xs), nd)]


def timed(fn):
    t0 = time.perf_counter(); out = fn()
    return out, (time.perf_counter() - t0) * 1e3


def download(np, sbn, ctx, h, first, count):
    out = np.empty(64 * count, dtype=np.uint8)
    rc = sbn.lib().sbn_bases_download(ctx.h, h.h, C.c_size_t(first), C.c_size_t(count), out.ctypes.data_as(C.c_void_p))
    assert rc == 0, rc
    return out


def same_points(np, sbn, ctx, a, b, n):
    return all(np.array_equal(download(np, sbn, ctx, a, f, min(BLOCK, n - f)), download(np, sbn, ctx, b, f, min(BLOCK, n - f))) for f in range(0, n, BLOCK))


def kernel_ns(ctx, fn, name, points):
    ctx.prof_enable(True); ctx.prof_reset()
    try:
        fn()
        ms, launches = ctx.prof_get()[name]
    finally:
        ctx.prof_enable(False)
    return ms * 1e6 / points, launches


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log", type=int, default=25)
    ap.add_argument("--passes", type=int, default=5)
    ap.add_argument("--sweep", default="14,16,18,20,22")
    ap.add_argument("--out", default=None)
    ap.add_argument("--kernels-only", action="store_true")
    a = ap.parse_args()
    import numpy as np
    sbn = load_pkg()
    n, n20 = (1 << a.log) + 1, 1 << 20
    g2_xy, tau_xy = sbn.kzg_srs_g2_from_tau(TAU)
    ctx = sbn.Context(0)
    lines = []

    def emit(o):
        lines.append(o); print(json.dumps(o), flush=True)

    try:
        ref = ctx.kzg_srs_from_tau(TAU, n)
        data = np.zeros(8 + 32 * n + 128, dtype=np.uint8)
        assert ctx.kzg_srs_save(ref, g2_xy, tau_xy, out=data) == len(data)
        file20 = np.concatenate([np.frombuffer(n20.to_bytes(8, "little"), dtype=np.uint8), data[8:8 + 32 * n20], data[-128:]])
        comp20 = np.ascontiguousarray(data[8:8 + 32 * n20])

        def load(d=data, flags=0, want_lines=True):
            hs = ctx.kzg_srs_load(d, flags=flags, want_lines=want_lines)
            for h in hs[1:3]:
                if h is not None:
                    h.free()
            return hs[0]

        if a.kernels_only:
            load().free(); load(file20).free(); ctx.bases_from_compressed(comp20).free()
            return
        srs = load()
        assert same_points(np, sbn, ctx, srs, ref, n), "the loaded handle differs from the generated one"
        srs.free()
        emit({"bench": "kzg_srs", "n": n, "file_bytes": int(len(data)), "loaded_equals_generated": True, "default_chunk_points": 1 << 18})

        xy = download(np, sbn, ctx, ref, 0, n)                              # what a caller hands sbn_kzg_srs_upload today
        rng = np.random.default_rng(28)
        coeffs = rng.integers(0, 256, size=32 * n, dtype=np.uint8); coeffs[31::32] &= 0x1f
        table = ctx.table_upload(coeffs)
        l_g2, l_tau = ctx.g2_prepare(g2_xy), ctx.g2_prepare(tau_xy)
        out_buf = np.zeros(len(data), dtype=np.uint8)
        assert ctx.kzg_srs_check(ref, l_g2, l_tau, RHO), "the generated SRS fails its own check"
        ctx.kzg_commit(ref, table, n); ctx.kzg_srs_upload(xy).free(); load(flags=sbn.SBN_SRS_CHECK).free()      # warm-up
        t = {k: [] for k in ("load", "load_no_g2", "upload", "save", "check", "commit", "load_check")}
        for _ in range(a.passes):                                           # alternating: other work shares the host
            for name, fn in (("load", lambda: load().free()), ("load_no_g2", lambda: load(want_lines=False).free()), ("upload", lambda: ctx.kzg_srs_upload(xy).free()),
                             ("save", lambda: ctx.kzg_srs_save(ref, g2_xy, tau_xy, out=out_buf)), ("check", lambda: ctx.kzg_srs_check(ref, l_g2, l_tau, RHO)),
                             ("commit", lambda: ctx.kzg_commit(ref, table, n)), ("load_check", lambda: load(flags=sbn.SBN_SRS_CHECK).free())):
                ctx.sync()
                _, ms = timed(fn)
                t[name].append(ms)
        assert np.array_equal(out_buf, data)
        emit({"bench": "kzg_srs_wall_ms", "n": n, "passes": a.passes, "srs_load_ms": span(t["load"]), "srs_load_without_g2_handles_ms": span(t["load_no_g2"]),
              "srs_upload_uncompressed_ms": span(t["upload"]), "srs_save_ms": span(t["save"]), "srs_check_ms": span(t["check"]), "kzg_commit_same_n_ms": span(t["commit"]),
              "srs_load_with_check_ms": span(t["load_check"])})
        table.free(); l_g2.free(); l_tau.free()
        del xy, coeffs

        k = {"srs_n": [], "srs_20": [], "g1_20": []}
        for _ in range(a.passes):
            k["srs_n"].append(kernel_ns(ctx, lambda: load(want_lines=False).free(), "k_srs_decompress", n)[0])
            k["srs_20"].append(kernel_ns(ctx, lambda: load(file20, want_lines=False).free(), "k_srs_decompress", n20)[0])
            k["g1_20"].append(kernel_ns(ctx, lambda: ctx.bases_from_compressed(comp20).free(), "k_g1_decompress", n20)[0])
        sv = kernel_ns(ctx, lambda: ctx.kzg_srs_save(ref, g2_xy, tau_xy, out=out_buf), "k_srs_compress", n)
        emit({"bench": "kzg_srs_kernel_ns_per_point", "timer": "HIP events around each launch", "passes": a.passes, "k_srs_decompress_at_n": span(k["srs_n"], 2),
              "k_srs_decompress_at_2p20": span(k["srs_20"], 2), "k_g1_decompress_at_2p20": span(k["g1_20"], 2), "k_srs_compress_at_n": round(sv[0], 2),
              "srs_not_slower_than_g1_beyond_spread": min(k["srs_20"]) <= max(k["g1_20"])})
        ref.free()
    finally:
        ctx.close()
    if a.kernels_only:
        return
    sweep = {}
    for lg in [int(x) for x in a.sweep.split(",") if x]:
        os.environ["SBN_SRS_CHUNK"] = str(1 << lg)
        c2 = sbn.Context(0)
        try:
            def one():
                hs = c2.kzg_srs_load(data, want_lines=False)
                hs[0].free()
            one()
            ts = []
            for _ in range(3):
                c2.sync(); ts.append(timed(one)[1])
            sweep[f"2^{lg}"] = span(ts)
        finally:
            c2.close(); del os.environ["SBN_SRS_CHUNK"]
    emit({"bench": "kzg_srs_chunk_sweep_load_ms", "n": n, "passes": 3, "chunk_points": sweep})
    if a.out:
        with open(a.out, "w") as f:
            for ln in lines:
                f.write(json.dumps(ln) + "\n")


if __name__ == "__main__":
    main()
