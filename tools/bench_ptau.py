#!/usr/bin/env python3
"""A powers-of-tau ceremony file (.ptau) as the KZG SRS on one MI355X, through ctypes, at each n of --ns (default 2^20 and 2^25 + 1):

    ptau_load   sbn_kzg_srs_load_ptau of the first n powers of a .ptau file (64 B a point, k_ptau_points: no square root)
    srs_load    sbn_kzg_srs_load of the same powers in the reference's file format (32 B a point, k_srs_decompress: one square root a point)
    upload      sbn_kzg_srs_upload of the same powers as canonical x | y (what a caller with a parser of their own does today; nothing is checked)
    kernels     k_ptau_points beside k_srs_decompress per point (HIP events around each launch)

    python tools/bench_ptau.py [--ns 1048576,33554433] [--passes 5] [--out profiles/rNN_ptau.txt]

The powers are made by sbn_kzg_srs_from_tau and downloaded; the reference-format file is sbn_kzg_srs_save's, the .ptau file is the model's framing
(tests/ptau_model.py) around the downloaded points taken into the file's Montgomery form on the host.  The .ptau file is of the smallest power that holds
n powers; the powers behind the first n and all of section 3 behind its first two points are zero pages that are never read, so the file costs its
prefix.  Both loaded handles are compared with the generated one by download before anything is timed.  `--passes` alternating passes; medians.  The
one condition: the .ptau load is not slower than sbn_kzg_srs_load of the same powers, with a margin of 5 % (boxes and passes differ by about that
much); it is reported as a boolean with both medians and ranges, and gates nothing."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from __graft_entry__ import load_pkg  # noqa: E402

Q = 0x30644e72e131a029b85045b68181585d97816a916871ca8d3c208c16d87cfd47
R = 0x30644e72e131a029b85045b68181585d2833e84879b9709143e1f593f0000001
TAU = (0x1d2c3b4a5968778695a4b3c2d1e0f1021324354657687980a9bacbdcedfe0f1 % R).to_bytes(32, "little")
BLOCK = 1 << 22      # points a download in the comparison


def span(xs, nd=3):
    return {"median": round(statistics.median(xs), nd), "range": [round(min(xs), nd), round(max(xs), nd)]}


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


def to_file_form(np, xy):
    """canonical residues (32 B each) -> v 2^256 mod q, on the host: plain integers, a residue at a time"""
    mont = (1 << 256) % Q
    out = bytearray(len(xy))
    raw = xy.tobytes()
    for o in range(0, len(raw), 32):
        out[o:o + 32] = (int.from_bytes(raw[o:o + 32], "little") * mont % Q).to_bytes(32, "little")
    return np.frombuffer(out, dtype=np.uint8)


def kernel_ns(ctx, fn, name, points):
    ctx.prof_enable(True); ctx.prof_reset()
    try:
        fn()
        ms, _ = ctx.prof_get()[name]
    finally:
        ctx.prof_enable(False)
    return ms * 1e6 / points


def bench_one(np, sbn, ptm, ctx, n, passes, emit):
    g2_xy, tau_xy = sbn.kzg_srs_g2_from_tau(TAU)
    ref = ctx.kzg_srs_from_tau(TAU, n)
    srs_file = np.zeros(8 + 32 * n + 128, dtype=np.uint8)
    assert ctx.kzg_srs_save(ref, g2_xy, tau_xy, out=srs_file) == len(srs_file)
    xy = download(np, sbn, ctx, ref, 0, n)
    power = 1
    while ptm.counts(power)[0] < n:
        power += 1
    n_g1, n_g2 = ptm.counts(power)
    # the model's framing, section by section, into one buffer of untouched zero pages
    head = [(1, ptm.header_section(power)), (2, None), (3, None)]
    size = {1: 44, 2: 64 * n_g1, 3: 128 * n_g2}
    ptau = np.zeros(12 + sum(12 + size[s] for s, _ in head), dtype=np.uint8)
    ptau[:12] = np.frombuffer(b"ptau" + (1).to_bytes(4, "little") + (3).to_bytes(4, "little"), dtype=np.uint8)
    pos, off = 12, {}
    for s, payload in head:
        ptau[pos:pos + 12] = np.frombuffer(s.to_bytes(4, "little") + size[s].to_bytes(8, "little"), dtype=np.uint8)
        pos += 12; off[s] = pos
        if payload is not None:
            ptau[pos:pos + len(payload)] = np.frombuffer(payload, dtype=np.uint8)
        pos += size[s]
    _, conv_ms = timed(lambda: ptau.__setitem__(slice(off[2], off[2] + 64 * n), to_file_form(np, xy)))
    ptau[off[3]:off[3] + 256] = to_file_form(np, np.frombuffer(g2_xy + tau_xy, dtype=np.uint8))
    info = sbn.ptau_scan(ptau)
    assert (info.power, info.n_g1, info.off_g1, info.off_g2) == (power, n_g1, off[2], off[3])

    def drop(hs):
        for h in hs[:3]:
            if h is not None:
                h.free()

    calls = {"ptau_load": lambda: drop(ctx.kzg_srs_load_ptau(ptau, n)), "srs_load": lambda: drop(ctx.kzg_srs_load(srs_file)),
             "upload": lambda: ctx.kzg_srs_upload(xy).free()}
    for name, load in (("ptau", lambda: ctx.kzg_srs_load_ptau(ptau, n)), ("srs", lambda: ctx.kzg_srs_load(srs_file))):
        hs = load()
        assert same_points(np, sbn, ctx, hs[0], ref, n), f"the handle of the {name} load differs from the generated one"
        assert (hs[3], hs[4]) == (g2_xy, tau_xy)
        drop(hs)
    emit({"bench": "ptau", "n": n, "power": power, "ptau_bytes_read": 64 * n + 256 + 44 + 48, "ptau_file_bytes": int(len(ptau)), "srs_file_bytes": int(len(srs_file)),
          "both_loads_equal_generated": True, "host_conversion_of_the_test_file_ms": round(conv_ms)})
    for fn in calls.values():                                               # warm-up: staging buffers, pinned memory
        fn()
    t = {k: [] for k in calls}
    for _ in range(passes):                                                 # alternating: other work shares the host
        for name, fn in calls.items():
            ctx.sync()
            t[name].append(timed(fn)[1])
    med = {k: statistics.median(v) for k, v in t.items()}
    emit({"bench": "ptau_wall_ms", "n": n, "passes": passes, "ptau_load_ms": span(t["ptau_load"]), "srs_load_ms": span(t["srs_load"]), "srs_upload_unchecked_ms": span(t["upload"]),
          "ptau_over_srs_load": round(med["ptau_load"] / med["srs_load"], 3), "ptau_load_not_slower_than_srs_load_within_5_percent": med["ptau_load"] <= 1.05 * med["srs_load"]})
    k = {"ptau": [], "srs": []}
    for _ in range(passes):
        k["ptau"].append(kernel_ns(ctx, lambda: drop(ctx.kzg_srs_load_ptau(ptau, n, want_lines=False)), "k_ptau_points", n))
        k["srs"].append(kernel_ns(ctx, lambda: drop(ctx.kzg_srs_load(srs_file, want_lines=False)), "k_srs_decompress", n))
    emit({"bench": "ptau_kernel_ns_per_point", "n": n, "timer": "HIP events around each launch", "passes": passes, "k_ptau_points": span(k["ptau"], 2),
          "k_srs_decompress": span(k["srs"], 2)})
    ref.free()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ns", default=f"{1 << 20},{(1 << 25) + 1}")
    ap.add_argument("--passes", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import numpy as np
    import ptau_model as ptm
    sbn = load_pkg()
    ctx = sbn.Context(0)
    lines = []

    def emit(o):
        lines.append(o); print(json.dumps(o), flush=True)

    try:
        for n in [int(x) for x in a.ns.split(",") if x]:
            bench_one(np, sbn, ptm, ctx, n, a.passes, emit)
    finally:
        ctx.close()
    if a.out:
        with open(a.out, "w") as f:
            for ln in lines:
                f.write(json.dumps(ln) + "\n")


if __name__ == "__main__":
    main()
