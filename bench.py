#!/usr/bin/env python3
"""bench.py — throughput of the MI355X MSM hot path (BASELINE.json metric: BN254 G1 MSM points/s) and, in the same JSON line,
the other workloads SURVEY 8(d) names.

    python bench.py [--gpus N] [--steps K] [--warmup W] [--log-n 20] [--dump-outputs DIR]
    python bench.py --full [--blocks all|none|hyrax,sweep,sumcheck,prove_stages] [--group-devices 0,0] ...
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port P bench.py --gpus N ...
    (python bench.py --gpus N without a launcher starts the N ranks itself, before anything touches the GPU)

Headline (`value`, `ms_per_step`; BASELINE configs[1] / SURVEY 8d config 2): one MSM of 2^log_n points per GPU per step —
uniform full-width scalars (SplitMix64, reduced mod r), distinct bases with known discrete logs, inputs resident in HBM.  With
N > 1 the MSM of N*2^log_n points is sharded by base-point range; each rank's 64-byte partial sum goes through ONE all-gather
over RCCL and a local fold (weak scaling: per-GPU work fixed).

A plain run does only what the headline needs: set-up, warm-up, the K timed steps, the outputs (--dump-outputs) and the line.
--dump-outputs DIR writes the result of the last timed step, as a caller of the timed path receives it, to DIR/*.npy: every
affine point (64 B: x, y little-endian) as float32 16-bit limbs of shape (..., 2, 16), exact, and its infinity flag.

--full adds everything else, as before: the parity gate of the headline (discrete-log identity / CPU oracle, checked before
timing), the one-step-in-flight pass behind `serial_reference` and `roofline`, `cpu_baseline` (16 threads and 1 thread), and
the blocks below (--blocks, default all; --group-devices).  Each block is parity-gated before it is timed, one step in flight:
  hyrax      config 3: the derefs commitment shape, 4096 x 8192 uniform Fr scalars (rows 3072.. zero, hyrax.rs:245) against the
             reference's own generator set MultiCommitGens::new(8192, "gens_r1cs_eval"); fixed-base lookup table and bucket method;
             sampled rows checked against the CPU oracle; roofline with 32.02 B / pair.  With N > 1: ONE matrix, interleaved rows
             per rank (sharding.shard_rows), joined with gather_rows and checked.
  msm_sweep  2^22, 2^24, 2^26 points on one GPU (checked against the discrete-log identity).  With N > 1: config 4, the FIXED
             2^26-point MSM cut into N base-point ranges (strong scaling), folded over RCCL and checked.
  sumcheck   config 5's dominant sumcheck: prove_cubic_batched layer 0 of the ops product circuits, 12 "par" + 6 "seq" instances
             over 2^21-entry tables (2.7 GiB touched in round 0), 21 rounds; GB/s of algorithmic bytes against the 8 TB/s HBM peak.
Prints ONE JSON line on rank 0.
"""
import argparse
import hashlib
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

R_MOD = 0x30644e72e131a029b85045b68181585d2833e84879b9709143e1f593f0000001
MADD_PEAK = 1.64e10            # xyzz mixed additions/s with operands in registers, whole chip (tools/micro/ecbench.hip on MI355X, round 3: Y3 with one reduction; 1.46e10 in round 2)
HBM_PEAK_GBS = 8000.0          # MI355X_MICROARCH.md: 8 TB/s spec (6.3 TB/s achievable streaming)
S0 = 0x1234567890abcdef1234567890abcdef
DSTEP = 0x0fedcba987654321
SEED = 0x5BA27A2B4E254
G_XY = bytes([1]) + bytes(31) + bytes([2]) + bytes(31)


def splitmix_scalars(n, seed, first=0):
    """n uniform canonical Fr scalars (32 B LE each) from SplitMix64, numpy: the host twin of
    sbn_scalars_synthetic (tests compare the two)"""
    import numpy as np
    with np.errstate(over="ignore"):
        idx = np.arange(4 * n, dtype=np.uint64) + np.uint64(4 * first + 1)
        z = np.uint64(seed) + idx * np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        z = z ^ (z >> np.uint64(31))
    limbs = z.reshape(n, 4).copy()
    limbs[:, 3] &= np.uint64((1 << 62) - 1)                      # < 2^254
    r = [np.uint64((R_MOD >> (64 * i)) & 0xFFFFFFFFFFFFFFFF) for i in range(4)]
    ge = np.zeros(n, dtype=bool); decided = np.zeros(n, dtype=bool)
    for i in (3, 2, 1, 0):
        gt = (limbs[:, i] > r[i]) & ~decided; lt = (limbs[:, i] < r[i]) & ~decided
        ge |= gt; decided |= gt | lt
    ge |= ~decided
    borrow = np.zeros(n, dtype=np.uint64)
    with np.errstate(over="ignore"):
        for i in range(4):                                        # subtract r where value >= r  (value < 2^254 < 2r)
            sub = np.where(ge, r[i], np.uint64(0))
            t = limbs[:, i] - sub
            b1 = (limbs[:, i] < sub).astype(np.uint64)
            t2 = t - borrow
            b2 = (t < borrow).astype(np.uint64)
            limbs[:, i] = t2; borrow = b1 | b2
    return limbs.tobytes()


def dlog_expect(d_scal, first, n):
    """sum_i k_i * (S0 + (first+i)*DSTEP) mod r  =  S0*sum(k_i) + DSTEP*sum((first+i)*k_i), exact: the scalars (a CUDA uint8
    tensor of n x 32 B) are split into 16-bit digits so that every int64 partial sum stays below 2^63; chunked on the device."""
    import torch
    sum_k = 0; sum_ik = 0
    CH = 1 << 22
    for c0 in range(0, n, CH):
        m = min(CH, n - c0)
        k16 = d_scal[32 * c0:32 * (c0 + m)].view(torch.int16).view(m, 16).to(torch.int64) & 0xFFFF
        idx = torch.arange(c0, c0 + m, dtype=torch.int64, device=d_scal.device)
        ilo, ihi = (idx & 0xFFFF).unsqueeze(1), (idx >> 16).unsqueeze(1)            # n <= 2^31
        sj = k16.sum(0).tolist()                                                    # < 2^16 * 2^22
        lo = (k16 * ilo).sum(0).tolist()                                            # < 2^32 * 2^22
        hi = (k16 * ihi).sum(0).tolist()
        for j in range(16):
            sum_k += sj[j] << (16 * j)
            sum_ik += (lo[j] + (hi[j] << 16)) << (16 * j)
    tot = (S0 * sum_k + DSTEP * (sum_ik + first * sum_k)) % R_MOD
    return tot.to_bytes(32, "little")


def self_launch(ngpus):
    """python bench.py --gpus N without a launcher: start the N ranks as children (nothing here has touched the GPU yet)"""
    port = 29500 + (os.getpid() % 2000)
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={ngpus}", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    return subprocess.call(cmd)


def kernel_avgs(prof):
    return {k: round(ms / max(cnt, 1), 4) for k, (ms, cnt) in prof.items()}


def g1_limbs(xy):
    """affine points as the C ABI returns them (64 B each: x, y little-endian) -> float32 array (points, 2, 16) of their
    16-bit limbs: exact in float32, so two builds compare bit for bit"""
    import numpy as np
    return np.frombuffer(bytes(xy), dtype="<u2").reshape(-1, 2, 16).astype(np.float32)


def dump_outputs(out_dir, arrays):
    """--dump-outputs: DIR/<name>.npy per array (float32 / float64 only, 64 MB at most in all)"""
    import numpy as np
    assert all(a.dtype in (np.float32, np.float64) for a in arrays.values())
    assert sum(a.nbytes for a in arrays.values()) <= 64 << 20
    os.makedirs(out_dir, exist_ok=True)
    for name, a in arrays.items():
        np.save(os.path.join(out_dir, name + ".npy"), a)


def hbm_roofline(alg_bytes, kernel, kernel_ms, traffic=None, extra=None):
    """traffic: None or (HBM bytes per launch, source) from stored_traffic()"""
    achieved = alg_bytes / (kernel_ms * 1e-3) / 1e9 if kernel_ms else None
    r = {"bound": "hbm", "kernel": kernel, "achieved": round(achieved, 2) if achieved else None, "peak": HBM_PEAK_GBS, "unit": "GB/s",
         "frac": round(achieved / HBM_PEAK_GBS, 5) if achieved else None, "traffic": traffic[0] if traffic else None,
         "kernel_avg_ms": round(kernel_ms, 4) if kernel_ms else None, "algorithmic_bytes_per_launch": int(alg_bytes)}
    if traffic:
        r["traffic_source"] = traffic[1] + " (stored rocprofv3 --pmc passes of this workload at this size: FETCH_SIZE x 2 + WRITE_SIZE per the gfx950 correction; not measured by this run)"
    if extra:
        r.update(extra)
    return r


def stored_traffic(workload, size_key, kernel):
    """HBM bytes per launch of `kernel` from the committed rocprofv3 --pmc passes (profiles/pmc_traffic.json), only when the
    stored entry was measured at exactly this workload size; otherwise None (never a number from another size)."""
    path = os.path.join(ROOT, "profiles", "pmc_traffic.json")
    try:
        for e in json.load(open(path)).get("entries", []):
            if e.get("workload") == workload and e.get("size") == size_key and e.get("kernel") == kernel:
                return (e["hbm_bytes_per_launch"], e.get("source", "profiles/pmc_traffic.json"))
    except Exception:
        pass
    return None


def summarize(line):
    """the round's figures in one compact object (<= ~1.5 kB), emitted as the LAST key of the JSON line so that it survives a stored tail"""
    def g(d, *path):
        for k in path:
            if not isinstance(d, dict) or k not in d:
                return None
            d = d[k]
        return d
    s = {"msm_2^20": {"points_per_s": line.get("value"), "ms_per_step": line.get("ms_per_step"), "one_msm_alone_ms": g(line, "serial_reference", "ms_per_step"),
                      "k_acc_first_ms": g(line, "roofline", "kernel_avg_ms"), "hbm_frac": g(line, "roofline", "frac"), "alu_frac": g(line, "roofline", "alu", "frac"),
                      "traffic_bytes": g(line, "roofline", "traffic")}}
    hy = line.get("hyrax")
    if isinstance(hy, dict):
        h = {k: g(hy, k, "ms_per_step") for k in ("lookup", "bucket") if isinstance(hy.get(k), dict)}
        for k in ("lookup", "bucket"):
            if g(hy, k, "roofline", "frac") is not None:
                h[k + "_hbm_frac"] = g(hy, k, "roofline", "frac")
        if g(hy, "lookup", "lookup_table", "window_bits"):
            h["lookup_window_bits"] = g(hy, "lookup", "lookup_table", "window_bits")
        for k, v in (hy.get("variants") or {}).items():
            h[k] = v.get("ms_per_step", "skipped")
        if "error" in hy:
            h["error"] = hy["error"][:80]
        s["hyrax_ms"] = h
    sw = line.get("msm_sweep")
    if isinstance(sw, dict):
        s["msm_sweep"] = {k: {"ms": v.get("ms_per_step"), "points_per_s": v.get("points_per_s"), "alu_frac": g(v, "roofline", "alu", "frac")} for k, v in sw.items() if isinstance(v, dict)}
    sc = line.get("sumcheck")
    if isinstance(sc, dict):
        s["sumcheck"] = {"stateful_ms": g(sc, "stateful", "ms_per_sumcheck"), "fused_ms": g(sc, "fused", "ms_per_sumcheck"), "hbm_frac": g(sc, "roofline", "frac"),
                         "first_launch_frac": g(sc, "roofline", "largest_launch", "frac"), "round0_ms": g(sc, "stateful", "kernels_ms_total", "k_sc_eval_mixed"),
                         "traffic_bytes": g(sc, "roofline", "traffic")}
    ps = line.get("prove_stages")
    if isinstance(ps, dict):
        s["prove"] = {"total_device_side_ms": ps.get("total_device_side_ms"), "stage_ms": {x["stage"]: x["ms"] for x in ps.get("stages", [])},
                      "detail_ms": ps.get("detail_ms"), "digest": ps.get("transcript_digest")}
        if "error" in ps:
            s["prove"] = {"error": ps["error"][:80]}
    gr = line.get("group")
    if isinstance(gr, dict):
        s["group"] = {k: (v.get("ms_per_commit") or v.get("ms_per_commit_incl_pcie") or v.get("ms_per_msm")) for k, v in gr.items() if isinstance(v, dict)}
    if isinstance(line.get("collective"), dict):
        s["collective"] = {k: line["collective"].get(k) for k in ("backend", "world_size", "rccl_version", "all_gather_calls", "device_tensors")}
    cb = line.get("cpu_baseline")
    if isinstance(cb, dict):
        s["cpu_points_per_s"] = {"cores_%d" % cb.get("cores", 0): cb.get("value"), "cores_1": g(cb, "one_thread", "value")}
    return s


class Timer:
    def __init__(self, barrier):
        self.barrier = barrier

    def run(self, fn, steps):
        self.barrier(); t0 = time.perf_counter()
        for _ in range(steps):
            fn()
        self.barrier()
        return time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--workload", choices=["msm", "hyrax"], default="msm", help="which workload is the HEADLINE value (msm = BASELINE configs[1])")
    ap.add_argument("--log-n", type=int, default=20, help="msm headline: log2 of the points per GPU")
    ap.add_argument("--rows", type=int, default=4096, help="hyrax: matrix rows")
    ap.add_argument("--cols", type=int, default=8192, help="hyrax: matrix columns")
    ap.add_argument("--inflight", type=int, default=6, help="headline: independent steps kept in flight on separate HIP streams (contexts); 1 = strictly serial")
    ap.add_argument("--full", action="store_true", help="also run the parity gates, the one-step-in-flight pass (serial_reference, roofline), the CPU "
                    "baseline and the extra blocks; a plain run times the headline only")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None, help="write the last timed step's result to DIR/<name>.npy (float32)")
    ap.add_argument("--blocks", default=None, help="with --full: extra blocks, all (default) | none | comma list of hyrax,sweep,sumcheck,prove_stages")
    ap.add_argument("--sweep", default="22,24,26", help="msm_sweep sizes (log2) on one GPU")
    ap.add_argument("--strong-log-n", type=int, default=26, help="N > 1: log2 of the FIXED total size of the strong-scaling MSM (config 4)")
    ap.add_argument("--sc-log-n", type=int, default=21, help="sumcheck block: log2 of the table length")
    ap.add_argument("--const-tail", type=float, default=0.0, help="hyrax: fraction of each 512-row block whose rows repeat one constant "
                    "(the padded tail of every derefs matrix repeats mem[0], sparse_mlpoly_full.rs:89-101; ~0.43 at keyless size)")
    ap.add_argument("--precompute-gb", type=float, default=200.0, help="hyrax: HBM budget (GiB) of the fixed-base lookup table of the generator set "
                    "(sbn_bases_precompute; built once before the timed region like any commitment-key setup); 0 = bucket method only")
    ap.add_argument("--group-devices", default="", help="comma list of device indices (repeats allowed): adds a `group` block — ONE Hyrax matrix and ONE 2^26 MSM over "
                    "those devices from THIS process through the C ABI's device groups (sbn_group_*: host threads per device, no launcher, no collective); needs --gpus 1")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--force-collective", action="store_true", help="world size 1 only: still initialise the process group (backend nccl = RCCL, device_id = this GPU) and send every "
                    "partial sum / row commitment through the same all-gathers the N > 1 run uses (sharding.allgather_fold / gather_rows on device uint8 tensors) — "
                    "the collective code path exercised on a one-GPU box")
    args = ap.parse_args()
    if not args.full:
        if args.blocks not in (None, "none"):
            ap.error("--blocks needs --full")
        if args.group_devices:
            ap.error("--group-devices needs --full")
    if args.blocks is None:
        args.blocks = "all" if args.full else "none"

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus:
        if world == 1 and args.gpus > 1 and "RANK" not in os.environ:
            raise SystemExit(self_launch(args.gpus))
        raise SystemExit(f"--gpus {args.gpus} but WORLD_SIZE={world}")

    import numpy as np  # noqa: F401
    import torch
    import torch.distributed as dist
    from __graft_entry__ import load_pkg

    # BENCH_BACKEND=gloo rehearses the N > 1 path on a box with fewer GPUs than ranks (ranks then share devices and the
    # 64-byte partials travel as CPU tensors); the driver's runs use the default: "nccl", which is RCCL on ROCm.
    backend = os.environ.get("BENCH_BACKEND", "nccl")
    ndev = torch.cuda.device_count()
    dev_index = local_rank if backend == "nccl" else local_rank % max(ndev, 1)
    torch.cuda.set_device(dev_index)
    dev = torch.device("cuda", dev_index)
    coll_dev = dev if backend == "nccl" else torch.device("cpu")
    use_coll = world > 1 or args.force_collective          # partial sums / row commitments travel through torch.distributed
    if use_coll:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", str(29500 + (os.getpid() % 2000)))
        if backend == "nccl":
            dist.init_process_group("nccl", rank=rank, world_size=world, device_id=dev)
        else:
            dist.init_process_group(backend, rank=rank, world_size=world)

    sbn = load_pkg()
    from spartan_bn254_amd import sharding
    import oracle_lib as ol          # the checker and the cpu_baseline leg only
    ctx = sbn.Context(dev_index)    # raises if the HIP library / device is missing: no fallback
    M = max(1, args.inflight)
    ctxs = [ctx] + [sbn.Context(dev_index) for _ in range(M - 1)]     # one HIP stream + workspace per step in flight
    blocks = set() if args.blocks == "none" else ({"hyrax", "sweep", "sumcheck", "prove_stages"} if args.blocks == "all" else set(args.blocks.split(",")))

    def barrier():
        if use_coll:
            dist.barrier()
        torch.cuda.synchronize()
        for cx in ctxs:
            cx.sync()

    def max_over_ranks(dt):
        if not use_coll:
            return dt
        t = torch.tensor([dt], dtype=torch.float64, device=coll_dev)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        return float(t.item())

    timer = Timer(barrier)

    def synth_scalars(n, first):
        t = torch.empty(32 * n, dtype=torch.uint8, device=dev)
        ctx.scalars_synthetic(SEED, first, n, t.data_ptr())
        return t

    def fold_partials(parts):
        """one all-gather for the partial sums of the steps that just completed, then the local folds"""
        if not use_coll:
            return parts
        if len(parts) == 1:
            return [sharding.allgather_fold(parts[0][0], device=coll_dev)]
        xy, _ = zip(*parts)
        allb = sharding.allgather_bytes(b"".join(xy), device=coll_dev)
        return [sbn.g1_sum(b"".join(a[64 * j:64 * j + 64] for a in allb)) for j in range(len(parts))]

    # ------------------------------------------------------------------------------------------------ one MSM problem
    def msm_problem(n, first, expect=True):
        """bases P_i = (S0 + (first+i) DSTEP) G, scalars from the SplitMix64 stream at offset `first`, the expected partial sum
        (None unless `expect`)"""
        d_scal = synth_scalars(n, first)
        bases = ctx.bases_synthetic(n, first, S0.to_bytes(32, "little"), DSTEP.to_bytes(32, "little"))
        want = ol.g1_mul(G_XY, dlog_expect(d_scal, first, n)) if expect else None
        return d_scal, bases, want

    def check_sharded(total, want):
        """the folded result must be the sum of all ranks' expectations"""
        if not use_coll:
            return total == want
        wants = [None] * world
        dist.all_gather_object(wants, want)
        return total == sbn.g1_sum(b"".join(wants))[0]

    def timed_msm(cx_list, d_scal, bases, n, steps, warm):
        """`steps` MSMs, one in flight on cx_list[0] when len == 1, else shared out over the streams; returns (seconds, profile,
        the result of the last step as the caller receives it: the folded sum when the partials travel through the collective)"""
        from concurrent.futures import ThreadPoolExecutor
        Mx = len(cx_list)
        pool = ThreadPoolExecutor(max_workers=Mx) if Mx > 1 else None

        def local(cx):
            return cx.msm_bases_dev(bases, d_scal.data_ptr(), n)

        def run(count):
            last = None
            if Mx == 1:
                for _ in range(count):
                    last = fold_partials([local(cx_list[0])])[-1]
                return last
            if not use_coll:
                shares = [count // Mx + (1 if j < count % Mx else 0) for j in range(Mx)]
                futs = [pool.submit(lambda cx=cx, k=k: [local(cx) for _ in range(k)]) for cx, k in zip(cx_list, shares)]
                for f in futs:
                    last = (f.result() or [last])[-1]
                return last
            done = 0
            while done < count:                   # rounds of up to 4 steps per stream, then ONE all-gather carrying all their partials
                g = min(4 * Mx, count - done)
                shares = [g // Mx + (1 if j < g % Mx else 0) for j in range(Mx)]
                futs = [pool.submit(lambda cx=cx, k=k: [local(cx) for _ in range(k)]) for cx, k in zip(cx_list, shares) if k]
                last = fold_partials([p for f in futs for p in f.result()])[-1]
                done += g
            return last

        for cx in cx_list:                        # every stream's workspace is sized before the timed region
            local(cx)
        run(warm)
        for cx in cx_list:
            cx.prof_enable(True); cx.prof_reset()
        barrier(); t0 = time.perf_counter()
        last = run(steps)
        barrier(); dt = time.perf_counter() - t0
        prof = {}
        for cx in cx_list:
            for k, (ms, cnt) in cx.prof_get().items():
                a, b = prof.get(k, (0.0, 0)); prof[k] = (a + ms, b + cnt)
            cx.prof_enable(False)
        if pool:
            pool.shutdown()
        return max_over_ranks(dt), prof, last

    def msm_alu(job, kernel_ms):
        madds = job["slots"]                      # uniform scalars: a digit is zero with probability 2^-c
        return {"unit": "mixed additions/s", "achieved": round(madds / (kernel_ms * 1e-3), 1), "peak": MADD_PEAK, "frac": round(madds / (kernel_ms * 1e-3) / MADD_PEAK, 4),
                "window_bits": job["c"], "windows": job["W"], "mixed_additions_per_launch": int(madds),
                "note": "peak = xyzz_madd in registers, all CUs busy (tools/micro/ecbench.hip); kernel time from the one-step-in-flight pass"}

    # ------------------------------------------------------------------------------------------------ Hyrax matrices
    def hyrax_setup(L, Rc):
        bases, _ = ctx.gens_new(Rc, b"gens_r1cs_eval", want_points=False)    # the reference's gens_derefs set (sparse_mlpoly_full.rs:625-627)
        Z = synth_scalars(L * Rc, 1 << 40)                                   # uniform in Fr, full width
        Zv = Z.view(L, Rc * 32)
        Zv[(3 * L // 4):] = 0                                                # rows 3072.. are zero padding (hyrax.rs:245)
        if args.const_tail > 0:                                              # SURVEY 8d config 3 variant: constant suffix of every 512-row block
            blk = max(1, L // 8)
            for b0 in range(0, 3 * L // 4, blk):
                k0 = b0 + int(blk * (1.0 - args.const_tail))
                Zv[k0:b0 + blk] = Zv[k0:k0 + 1, :32].repeat(1, Rc)
        torch.cuda.synchronize()
        return bases, Z

    def hyrax_check(Z, out, L, Rc, rows, gxy):
        Zv = Z.view(L, Rc * 32)
        for i in rows:
            row = Zv[i].cpu().numpy().tobytes()
            if out[64 * i:64 * i + 64] != ol.commit(row, bytes(32), gxy[:64 * Rc], gxy[64 * Rc:]):
                return i
        return None

    line_extra = {}
    cpu_baseline = None
    serial = roofline = None
    outputs = {}                                                   # --dump-outputs: name -> array, what the last timed step returned
    # ================================================================================================ headline
    if args.workload == "msm":
        n = 1 << args.log_n
        first = rank * n                                           # this rank's base-point range of the N*n-point MSM
        d_scal, bases, want = msm_problem(n, first, expect=args.full)
        if args.full:
            part, _ = ctx.msm_bases_dev(bases, d_scal.data_ptr(), n)   # parity gate: partial == (sum k_i s_i) G, exact
            if part != want:
                raise SystemExit(f"rank {rank}: GPU MSM result differs from the discrete-log oracle")
            total = fold_partials([(part, False)])[0][0]
            if not check_sharded(total, want):
                raise SystemExit("sharded MSM result differs from the folded oracle partials")
        dt, prof, last = timed_msm(ctxs, d_scal, bases, n, args.steps, args.warmup)
        if last is not None:
            outputs = {"msm_point": g1_limbs(last[0]), "msm_infinity": np.array([float(last[1])], dtype=np.float32)}
        units_per_step = n
        dominant = "k_acc_first"
        if args.full:
            ns_ser = max(2, min(16, args.steps))
            ts, sp, _ = timed_msm([ctx], d_scal, bases, n, ns_ser, 1)
            serial = {"steps": ns_ser, "ms_per_step": round(ts / ns_ser * 1e3, 4), "kernels_avg_ms": kernel_avgs(sp)}
            dom_ms = serial["kernels_avg_ms"].get(dominant, 0.0)
            roofline = hbm_roofline(96.0 * n, dominant, dom_ms, stored_traffic("msm", f"2^{args.log_n}", dominant),
                                    {"note": "kernel time from the one-step-in-flight pass (with several streams a launch shares the chip and its event-to-event time "
                                             "stretches); MSM is integer-ALU bound (~170 modular products per point vs 96 B): see roofline.alu and DESIGN.md"})
            if M > 1:
                pm, pc = prof.get(dominant, (0.0, 0))
                roofline["inflight_pass_kernel_avg_ms"] = round(pm / max(pc, 1), 4)
            if dom_ms:
                roofline["alu"] = msm_alu(ctx.prof_last_job(), dom_ms)
        workload = f"synthetic BN254 G1 MSM, 2^{args.log_n} uniform Fr scalars x distinct bases per GPU, inputs resident in HBM"
        sharding_desc = "base-point ranges + one RCCL all-gather of 64-B partial sums"
        if args.full and rank == 0 and not args.no_cpu_baseline:   # rank 0 only, at every N (the other ranks wait at the next barrier, outside any timed region)
            cores = min(len(os.sched_getaffinity(0)), 16)
            ns = min(n, 1 << 20); n1 = min(n, 1 << 18)
            pts = ctx.bases_download(bases, 0, ns)
            sc_host = d_scal[:32 * ns].cpu().numpy().tobytes()
            tb = time.perf_counter(); got = ol.msm_pippenger(sc_host, pts, cores); tcpu = time.perf_counter() - tb
            if ns == n and got != want:
                raise SystemExit("CPU oracle and GPU disagree")
            tb = time.perf_counter(); ol.msm_pippenger(sc_host[:32 * n1], pts[:64 * n1], 1); t1 = time.perf_counter() - tb
            cpu_baseline = {"value": round(ns / tcpu, 1), "unit": "points/s", "cores": cores, "kind": "port",
                            "sample": f"the same MSM on its first 2^{ns.bit_length() - 1} points: oracle/ arkworks-style signed-digit Pippenger (c={ol.window_bits(ns)}), threads over windows",
                            "one_thread": {"value": round(n1 / t1, 1), "unit": "points/s", "cores": 1,
                                           "sample": f"first 2^{n1.bit_length() - 1} points, 1 thread (the published RAYON_NUM_THREADS=1 configuration, reference README.md:29-35); c={ol.window_bits(n1)}"}}
        bases.free(); del d_scal
    else:
        L, Rc = args.rows, args.cols
        bases, Z = hyrax_setup(L, Rc)
        comb_c = 0
        if args.precompute_gb > 0:
            try:
                comb_c = ctx.bases_precompute(bases, int(args.precompute_gb * (1 << 30)))
            except sbn.SbnError as e:                              # e.g. another tenant holds the HBM: keep the bucket method
                print(f"[bench] precompute skipped: {e}", file=sys.stderr)
        # ONE matrix; with N > 1 every rank commits its interleaved rows and the commitments are joined with gather_rows
        my_rows = sharding.shard_rows(L, rank, world)
        Zl = Z.view(L, Rc * 32)[rank::world].contiguous() if world > 1 else Z
        nl = len(my_rows)

        last_rows = [None]

        def hy_step():
            out, _ = ctx.commit_rows_dev(bases, Zl.data_ptr(), 0, nl, Rc)
            last_rows[0] = sharding.gather_rows(out, L, rank, world, device=coll_dev) if use_coll else out
            return last_rows[0]

        out = hy_step()
        if args.full:
            gxy, _ = ol.gens_new(Rc, b"gens_r1cs_eval")
            bad = hyrax_check(Z, out, L, Rc, (0, 1, L // 2, 3 * L // 4 - 1, L - 1), gxy) if rank == 0 else None
            if bad is not None:
                raise SystemExit(f"Hyrax row {bad} differs from the oracle")
        for _ in range(args.warmup):
            hy_step()
        ctx.prof_enable(True); ctx.prof_reset()
        last_rows[0] = None
        dt = max_over_ranks(timer.run(hy_step, args.steps))
        prof = ctx.prof_get(); ctx.prof_enable(False)
        if last_rows[0] is not None:
            outputs = {"hyrax_row_commitments": g1_limbs(last_rows[0])}
        serial = {"steps": args.steps, "ms_per_step": round(dt / args.steps * 1e3, 4), "kernels_avg_ms": kernel_avgs(prof)}
        units_per_step = L * Rc / world
        dominant = "k_comb_rows" if comb_c else "k_acc_first"
        alg = nl * Rc * 32.0 + (Rc + 1) * 64.0 + nl * 64.0
        roofline = hbm_roofline(alg, dominant, serial["kernels_avg_ms"].get(dominant, 0.0), stored_traffic("hyrax-lookup" if comb_c else "hyrax-bucket", f"{nl}x{Rc}", dominant))
        workload = f"Hyrax derefs commitment: ONE {L} x {Rc} matrix of uniform Fr scalars, {Rc}+1 shared reference generators, last quarter of rows zero, inputs resident in HBM" + (
            f", fixed-base lookup table c={comb_c}" if comb_c else ", bucket method")
        sharding_desc = "interleaved rows of one matrix per rank, joined by one all-gather of the row commitments; no data-path reduction"
        M = 1
        bases.free(); del Z, Zl

    value = units_per_step * world * args.steps / dt
    if args.dump_outputs and rank == 0:
        if not outputs:
            raise SystemExit("--dump-outputs: the timed path returned nothing (--steps 0?)")
        dump_outputs(args.dump_outputs, outputs)

    # ================================================================================================ extra blocks (--full)
    torch.cuda.empty_cache()
    if "hyrax" in blocks and args.workload == "msm":
        L, Rc = args.rows, args.cols
        try:
            hb, Z = hyrax_setup(L, Rc)
            gxy, _ = ol.gens_new(Rc, b"gens_r1cs_eval") if rank == 0 else (None, None)
            my_rows = sharding.shard_rows(L, rank, world)
            Zl = Z.view(L, Rc * 32)[rank::world].contiguous() if world > 1 else Z
            nl = len(my_rows)
            res = {"shape": f"{L}x{Rc}", "scalars": "uniform in Fr (SplitMix64 mod r), rows >= 3L/4 zero", "generators": "MultiCommitGens::new(cols, b'gens_r1cs_eval') (commitments.rs:31-62; 2813 unique points + h at 8192 columns)",
                   "rows_per_rank": nl, "sharding": "interleaved rows of ONE matrix, gather_rows" if world > 1 else None,
                   "algorithmic_bytes_per_pair": round((L * Rc * 32.0 + (Rc + 1) * 64.0 + L * 64.0) / (L * Rc), 3)}

            def hy_step():
                out, _ = ctx.commit_rows_dev(hb, Zl.data_ptr(), 0, nl, Rc)
                return sharding.gather_rows(out, L, rank, world, device=coll_dev) if use_coll else out

            variants = [("bucket", 0.0)] + ([("lookup", args.precompute_gb)] if args.precompute_gb > 0 else [])
            for name, gb in variants:                      # bucket first: the lookup table stays attached to the handle once built
                comb_c = 0; tpre = 0.0
                if gb > 0:
                    tpre = time.perf_counter()
                    err = None
                    try:
                        comb_c = ctx.bases_precompute(hb, int(gb * (1 << 30)))
                    except sbn.SbnError as e:
                        err = str(e)
                    if use_coll:                           # the variant's steps hold a collective: every rank runs it or none does
                        flag = torch.tensor([0 if err is None else 1], dtype=torch.int32, device=coll_dev)
                        dist.all_reduce(flag, op=dist.ReduceOp.MAX)
                        if int(flag.item()) and err is None:
                            err = "another rank could not build its lookup table"
                    if err is not None:
                        res[name] = {"skipped": err}; continue
                    tpre = time.perf_counter() - tpre
                out = hy_step()
                bad = hyrax_check(Z, out, L, Rc, (0, 7, L // 2 + 1, 3 * L // 4 - 1, 3 * L // 4, L - 1), gxy) if rank == 0 else None
                if bad is not None:
                    raise SystemExit(f"hyrax[{name}]: row {bad} differs from the oracle")
                hy_step()
                ksteps = max(3, min(10, args.steps))
                ctx.prof_enable(True); ctx.prof_reset()
                hdt = max_over_ranks(timer.run(hy_step, ksteps))
                hp = kernel_avgs(ctx.prof_get()); ctx.prof_enable(False)
                dom = "k_comb_rows" if comb_c else "k_acc_first"
                alg = nl * Rc * 32.0 + (Rc + 1) * 64.0 + nl * 64.0
                job = ctx.prof_last_job()
                r = {"ms_per_step": round(hdt / ksteps * 1e3, 4), "pairs_per_s": round(L * Rc * ksteps / hdt, 1), "steps": ksteps, "window_bits": job["c"],
                     "parity": "6 sampled rows (first, zero-padding, last non-zero) bit-exact vs the CPU oracle",
                     "roofline": hbm_roofline(alg, dom, hp.get(dom, 0.0), stored_traffic("hyrax-" + name, f"{nl}x{Rc}", dom)),
                     "kernels_avg_ms": hp}
                if hp.get(dom):
                    madds = 0.75 * job["slots"] * (1.0 - args.const_tail)          # zero rows add nothing
                    r["roofline"]["alu"] = {"unit": "mixed additions/s", "achieved": round(madds / (hp[dom] * 1e-3), 1), "peak": MADD_PEAK, "frac": round(madds / (hp[dom] * 1e-3) / MADD_PEAK, 4)}
                if comb_c:
                    r["lookup_table"] = {"window_bits": comb_c, "build_s": round(tpre, 2)}
                res[name] = r
            if world == 1:
                # SURVEY 8d config 3's other variants, on the handle as the loop left it (lookup table attached when it fitted), each
                # parity-gated on sampled rows before it is timed
                method = "lookup" if (res.get("lookup") or {}).get("lookup_table") else "bucket"
                var = {}

                def timed_variant(handle, Zt, Lt, gx_bytes, hx_bytes, rows_chk):
                    o, _ = ctx.commit_rows_dev(handle, Zt.data_ptr(), 0, Lt, Rc)
                    Zt2 = Zt.view(Lt, Rc * 32)
                    for i in rows_chk:
                        if o[64 * i:64 * i + 64] != ol.commit(Zt2[i].cpu().numpy().tobytes(), bytes(32), gx_bytes, hx_bytes):
                            raise SystemExit(f"hyrax variant: row {i} differs from the oracle")
                    ks = 3
                    vdt = timer.run(lambda: ctx.commit_rows_dev(handle, Zt.data_ptr(), 0, Lt, Rc), ks)
                    return {"ms_per_step": round(vdt / ks * 1e3, 4), "pairs_per_s": round(Lt * Rc * ks / vdt, 1), "window_bits": ctx.prof_last_job()["c"]}

                # (1) the padded suffix of every derefs matrix repeats one constant (sparse_mlpoly_full.rs:89-101; ~43 % of the non-zero rows at keyless size)
                Zc = Z.clone(); Zv = Zc.view(L, Rc * 32); blk = max(1, L // 8)
                for b0 in range(0, 3 * L // 4, blk):
                    k0 = b0 + int(blk * 0.57)
                    Zv[k0:b0 + blk] = Zv[k0:k0 + 1, :32].repeat(1, Rc)
                torch.cuda.synchronize()
                var["const_tail_0.43"] = dict(timed_variant(hb, Zc, L, gxy[:64 * Rc], gxy[64 * Rc:], (0, int(blk * 0.57), blk - 1, 3 * L // 4 - 1, L - 1)), method=method,
                                              note="the last 43 % of the rows of every 512-row block hold one repeated constant (the mem[0] lookups of padded ops)")
                del Zc, Zv
                # (2) BASELINE.json's "~2^24 points": 2048 x 8192
                L2 = L // 2
                Z2 = Z[:32 * L2 * Rc].clone(); Z2.view(L2, Rc * 32)[(3 * L2 // 4):] = 0; torch.cuda.synchronize()
                var[f"{L2}x{Rc}"] = dict(timed_variant(hb, Z2, L2, gxy[:64 * Rc], gxy[64 * Rc:], (0, L2 // 2, 3 * L2 // 4 - 1, L2 - 1)), method=method, note="2^24 (scalar, base) pairs, rows >= 3L/4 zero")
                del Z2
                # (3) 8192 DISTINCT bases (the reference's derivation makes 66 % of its generators equal: nothing to merge here)
                db = ctx.bases_synthetic(Rc, 0, S0.to_bytes(32, "little"), DSTEP.to_bytes(32, "little"))
                dxy = ctx.bases_download(db, 0, Rc)
                var["distinct_bases"] = dict(timed_variant(db, Z, L, dxy, G_XY, (0, L // 2 + 1, 3 * L // 4 - 1, L - 1)), method="bucket", note=f"{Rc} distinct points, no h, same {L}x{Rc} matrix")
                db.free()
                for v in var.values():
                    v["parity"] = "sampled rows bit-exact vs the CPU oracle"
                res["variants"] = var
            if rank == 0 and world == 1 and not args.no_cpu_baseline:
                cores = min(len(os.sched_getaffinity(0)), 16)
                rows = min(L, 2 * cores)
                Zs = Z[:rows * Rc * 32].cpu().numpy().tobytes()
                tb = time.perf_counter(); got = ol.commit_rows(Zs, None, rows, Rc, gxy[:64 * Rc], gxy[64 * Rc:], cores); tcpu = time.perf_counter() - tb
                if got != out[:64 * rows]:
                    raise SystemExit("CPU oracle and GPU disagree (hyrax rows)")
                tb = time.perf_counter(); ol.commit_rows(Zs[:2 * Rc * 32], None, 2, Rc, gxy[:64 * Rc], gxy[64 * Rc:], 1); t1 = time.perf_counter() - tb
                res["cpu_baseline"] = {"value": round(rows * Rc / tcpu, 1), "unit": "pairs/s", "cores": cores, "kind": "port",
                                       "sample": f"first {rows} rows of the same matrix: oracle/ per-row Pippenger, threads over rows (hyrax.rs:259-261)",
                                       "one_thread": {"value": round(2 * Rc / t1, 1), "unit": "pairs/s", "cores": 1, "sample": "first 2 rows, 1 thread; the reference publishes 166.2 s for the whole commitment on one M2 Max core (BENCHMARK_RESULTS.md:37-39)"}}
            line_extra["hyrax"] = res
            hb.free(); del Zl
            if world == 1 and args.precompute_gb > 0 and "variants" in res:
                # the same 8192 DISTINCT bases with THEIR fixed-base lookup table (the reference's set shares 177 GB among 2814 unique points; 8193 distinct points fit
                # c = 15: 17 windows x 2^14 multiples x 64 B = 146 GB) — what the commitment costs if the reference ever derives distinct generators (group.rs:110-131)
                try:
                    torch.cuda.empty_cache()
                    db = ctx.bases_synthetic(Rc, 0, S0.to_bytes(32, "little"), DSTEP.to_bytes(32, "little"))
                    dxy = ctx.bases_download(db, 0, Rc)
                    tb = time.perf_counter(); cdb = ctx.bases_precompute(db, int(args.precompute_gb * (1 << 30))); tpre = time.perf_counter() - tb
                    o, _ = ctx.commit_rows_dev(db, Z.data_ptr(), 0, L, Rc)
                    for i in (0, L // 2 + 1, 3 * L // 4 - 1, L - 1):
                        if o[64 * i:64 * i + 64] != ol.commit(Z.view(L, Rc * 32)[i].cpu().numpy().tobytes(), bytes(32), dxy, G_XY):
                            raise SystemExit(f"hyrax distinct-bases lookup: row {i} differs from the oracle")
                    vdt = timer.run(lambda: ctx.commit_rows_dev(db, Z.data_ptr(), 0, L, Rc), 3)
                    res["variants"]["distinct_bases_lookup"] = {"ms_per_step": round(vdt / 3 * 1e3, 4), "pairs_per_s": round(L * Rc * 3 / vdt, 1), "window_bits": cdb, "method": "lookup",
                                                                "lookup_table_build_s": round(tpre, 2), "note": f"{Rc} distinct points with their own lookup table", "parity": "sampled rows bit-exact vs the CPU oracle"}
                    db.free()
                except sbn.SbnError as e:
                    res["variants"]["distinct_bases_lookup"] = {"skipped": str(e)}
            del Z
        except (sbn.SbnError, RuntimeError) as e:
            line_extra["hyrax"] = {"error": str(e)}
        torch.cuda.empty_cache()

    if "sweep" in blocks and args.workload == "msm":
        sweep = {}
        if world == 1:
            for ln in [int(x) for x in args.sweep.split(",") if x]:
                try:
                    nn = 1 << ln
                    ds, bs, wt = msm_problem(nn, 0)
                    got, _ = ctx.msm_bases_dev(bs, ds.data_ptr(), nn)
                    if got != wt:
                        raise SystemExit(f"msm_sweep 2^{ln}: GPU result differs from the discrete-log oracle")
                    ksteps = 12 if ln <= 22 else 6 if ln <= 24 else 3
                    sdt, sp, _ = timed_msm([ctx], ds, bs, nn, ksteps, 1)
                    ka = kernel_avgs(sp)
                    e = {"ms_per_step": round(sdt / ksteps * 1e3, 4), "points_per_s": round(nn * ksteps / sdt, 1), "steps": ksteps, "steps_in_flight": 1,
                         "parity": "bit-exact vs the discrete-log identity", "kernels_avg_ms": ka,
                         "roofline": hbm_roofline(96.0 * nn, "k_acc_first", ka.get("k_acc_first", 0.0), stored_traffic("msm", f"2^{ln}", "k_acc_first"))}
                    if ka.get("k_acc_first"):
                        e["roofline"]["alu"] = msm_alu(ctx.prof_last_job(), ka["k_acc_first"])
                    sweep[f"2^{ln}"] = e
                    bs.free(); del ds
                    torch.cuda.empty_cache()
                except sbn.SbnError as e:
                    sweep[f"2^{ln}"] = {"error": str(e)}
        else:
            # config 4: ONE MSM of 2^strong_log_n points, cut into `world` base-point ranges (strong scaling)
            ntot = 1 << args.strong_log_n
            lo, hi = sharding.shard_range(ntot, rank, world)
            nn = hi - lo
            ds, bs, wt = msm_problem(nn, lo)
            part, _ = ctx.msm_bases_dev(bs, ds.data_ptr(), nn)
            if part != wt:
                raise SystemExit(f"rank {rank}: strong-scaling partial differs from the discrete-log oracle")
            total = fold_partials([(part, False)])[0][0]
            if not check_sharded(total, wt):
                raise SystemExit("strong-scaling MSM: folded result differs from the folded oracle partials")
            ksteps = 4
            sdt, sp, _ = timed_msm([ctx], ds, bs, nn, ksteps, 1)
            ka = kernel_avgs(sp)
            size_key = f"2^{nn.bit_length() - 1}" if nn & (nn - 1) == 0 else str(nn)
            strong_roof = hbm_roofline(96.0 * nn, "k_acc_first", ka.get("k_acc_first", 0.0), stored_traffic("msm", size_key, "k_acc_first"),
                                       {"note": "rank 0's share of the fixed-size MSM; traffic only where a stored --pmc pass of exactly this share size exists"})
            if ka.get("k_acc_first"):
                strong_roof["alu"] = msm_alu(ctx.prof_last_job(), ka["k_acc_first"])
            sweep[f"2^{args.strong_log_n}_strong"] = {"roofline": strong_roof,"total_points": ntot, "points_per_rank": nn, "n_gpus": world, "scaling": "strong", "ms_per_step": round(sdt / ksteps * 1e3, 4),
                                                      "points_per_s": round(ntot * ksteps / sdt, 1), "steps": ksteps, "parity": "each partial and the folded sum bit-exact vs the discrete-log identity",
                                                      "collective": f"one all-gather of {world} x 64 B per MSM ({backend})", "kernels_avg_ms": kernel_avgs(sp)}
            bs.free(); del ds
        line_extra["msm_sweep"] = sweep
        torch.cuda.empty_cache()

    if "sumcheck" in blocks and world == 1:
        try:
            line_extra["sumcheck"] = sumcheck_block(ctx, sbn, ol, torch, dev, args.sc_log_n)
        except sbn.SbnError as e:
            line_extra["sumcheck"] = {"error": str(e)}
        torch.cuda.empty_cache()

    if "prove_stages" in blocks and world == 1:
        try:
            line_extra["prove_stages"] = prove_stages_block(ctx, sbn, int(args.precompute_gb * (1 << 30)))
        except sbn.SbnError as e:
            line_extra["prove_stages"] = {"error": str(e)}
        torch.cuda.empty_cache()

    if args.group_devices and world == 1:
        try:
            line_extra["group"] = group_block(sbn, ol, torch, [int(x) for x in args.group_devices.split(",")], args.rows, args.cols, args.strong_log_n)
        except sbn.SbnError as e:
            line_extra["group"] = {"error": str(e)}
        torch.cuda.empty_cache()

    if rank == 0:
        line = {"metric": "msm_points_per_s", "value": round(value, 1), "unit": "points/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
                "ms_per_step": round(dt / args.steps * 1e3, 4), "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
                "dtype": "u32", "data": "synthetic", "full": bool(args.full),
                "config": {"workload": workload, "units_per_step_per_gpu": int(units_per_step), "steps_in_flight": M, "collective_backend": backend if use_coll else None,
                           "sharding": sharding_desc, "parity": "bit-exact vs the discrete-log identity / CPU oracle, checked before timing" if args.full
                           else "not checked by a plain run (--full checks it before timing; --dump-outputs writes the result)"},
                "roofline": roofline, "cpu_baseline": cpu_baseline, "kernels_avg_ms": kernel_avgs(prof), "serial_reference": serial}
        line.update(line_extra)
        if use_coll:
            try:
                ver = ".".join(str(x) for x in torch.cuda.nccl.version()) if backend == "nccl" else None
            except Exception:
                ver = None
            line["collective"] = dict(sharding.STATS, backend=dist.get_backend(), world_size=world, rccl_version=ver, forced_at_world_size_1=bool(args.force_collective),
                                      note="every partial sum / row commitment of this run went through torch.distributed all_gather on uint8 tensors (sharding.py)")
        line["summary"] = summarize(line)          # LAST key: the driver keeps only the tail of a long line
        print(json.dumps(line), flush=True)
    for cx in ctxs:
        cx.close()
    if use_coll:
        dist.destroy_process_group()


def sumcheck_block(ctx, sbn, ol, torch, dev, logn):
    """prove_cubic_batched, layer 0 of the ops product circuits (sumcheck.rs:165-330): 12 "par" instances sharing one C
    table + 6 "seq" instances, tables of 2^logn uniform Fr values.  Three drivers of the same rounds:
      stateful  sbn_sumcheck_begin / round / finish: the coeffs-combined triple per round (what the transcript absorbs, :269-271), "par"
                group on the combined kernels (one reduction per index for all instances, C factored out)   <- the reported path
      fused     one sbn_sc_bind_eval_cubic_batched per round, 18 triples back per round (round 2's path)
      separate  eval + bind launches (the reference's structure)
    Parity: the stateful run's combined values of ALL rounds and its 43 final claims against the oracle's prove_cubic_batched loop on
    the same tables; fused and separate must agree with each other on every final value and with the stateful finals."""
    import numpy as np
    n = 1 << logn
    NPAR, NSEQ = 12, 6
    ntab = 2 * NPAR + 1 + 3 * NSEQ
    coeffs = splitmix_scalars(NPAR + NSEQ, SEED + 77)

    def fresh(keep_host=False):
        ts, host = [], []
        for k in range(ntab):
            x = torch.empty(32 * n, dtype=torch.uint8, device=dev)
            ctx.scalars_synthetic(SEED + 1000 + k, 0, n, x.data_ptr())
            if keep_host:
                torch.cuda.synchronize(); host.append(x.cpu().numpy())
            ts.append(ctx.table_from_dev(x.data_ptr(), n, 0)); del x
        return ts, host

    def split(ts):
        par_a, par_b, c_par = ts[:NPAR], ts[NPAR:2 * NPAR], ts[2 * NPAR]
        rest = ts[2 * NPAR + 1:]
        return par_a, par_b, c_par, rest[:NSEQ], rest[NSEQ:2 * NSEQ], rest[2 * NSEQ:]

    def challenge(ev, rnd):
        return (int.from_bytes(hashlib.sha3_256(ev + bytes([rnd])).digest(), "little") % R_MOD).to_bytes(32, "little")

    res = {"workload": f"batched cubic sumcheck, {NPAR} par + {NSEQ} seq instances, tables of 2^{logn}, {logn} rounds, {round(ntab * n * 32 / 2**30, 2)} GiB in round 0"}
    finals = {}
    chal_used = None
    for mode in ("stateful", "fused", "separate"):
        times = []; prof = {}
        reps = 2 if mode == "separate" else 3
        for rep in range(reps):
            gate = mode == "stateful" and rep == 0
            ts, host = fresh(keep_host=gate)
            pa, pb, pc, sa, sb_, sc_ = split(ts)
            As, Bs, Cs = pa + sa, pb + sb_, [pc] * NPAR + sc_
            ctx.prof_enable(True); ctx.prof_reset()
            ctx.sync(); t0 = time.perf_counter()
            if mode == "stateful":
                st, ev = ctx.sumcheck_begin(pa, pb, pc, sa, sb_, sc_, coeffs)
                evs, chs = [ev], []
                for rnd in range(logn):
                    chs.append(challenge(ev, rnd))
                    ev = st.round(chs[-1]); evs.append(ev)
                fin = st.finish()
                ctx.sync(); dtm = time.perf_counter() - t0
                st.free()
                if gate:                                           # the whole sumcheck against the oracle's loop on the same tables
                    hp = split(host)
                    _, want_comb, want_fin = ol.sc_prove_cubic_batched(hp[0], hp[1], hp[2], hp[3], hp[4], hp[5], coeffs, b"".join(chs), min(len(os.sched_getaffinity(0)), 16))
                    for j in range(logn):
                        if evs[j] != want_comb[j]:
                            raise SystemExit(f"sumcheck block: combined sums of round {j} differ from the oracle")
                    if fin != want_fin:
                        raise SystemExit("sumcheck block: final claims differ from the oracle")
                    del host, hp
                finals[mode] = fin; chal_used = chs
            else:
                ev = ctx.sc_eval_cubic_batched(As, Bs, Cs)
                for rnd in range(logn):
                    r = chal_used[rnd]                               # the same challenges: the three drivers must end in the same claims
                    if mode == "fused" and len(ts[0]) >= 4:
                        ev = ctx.sc_bind_eval_cubic_batched(As, Bs, Cs, r)
                    else:
                        ctx.bind_top_many(ts, r)
                        if len(ts[0]) >= 2:
                            ev = ctx.sc_eval_cubic_batched(As, Bs, Cs)
                ctx.sync(); dtm = time.perf_counter() - t0
                finals[mode] = [ctx.table_read0(t) for t in ts]
            prof = ctx.prof_get(); ctx.prof_enable(False)
            for t in ts:
                t.free()
            if rep:
                times.append(dtm)
        res[mode] = {"ms_per_sumcheck": round(1e3 * sum(times) / len(times), 3), "kernels_ms_total": {k: round(v[0], 3) for k, v in prof.items()},
                     "kernels_launches": {k: v[1] for k, v in prof.items()}}
    if not (finals["separate"] == finals["fused"] == finals["stateful"]):
        raise SystemExit("sumcheck block: the three drivers disagree on the final table values")
    table_bytes = ntab * n * 32
    par_bytes = (2 * NPAR) * n * 32
    # eval reads every live table once, a bind reads it once and writes half; live bytes halve per round (sum over rounds = 2 x round 0)
    alg_sep = 2 * table_bytes * (1 + 1 + 0.5)
    alg_first = table_bytes
    alg_fused_rounds = 2 * table_bytes * (1 + 0.5)
    for mode, alg in (("separate", alg_sep), ("fused", alg_first + alg_fused_rounds), ("stateful", alg_first + alg_fused_rounds)):
        ms = res[mode]["ms_per_sumcheck"]
        res[mode]["algorithmic_GB"] = round(alg / 1e9, 3)
        res[mode]["GBps_end_to_end"] = round(alg / (ms * 1e-3) / 1e9, 1)
    # the streaming rounds: ONE launch per round (k_sc_round_mixed: the "par" groups and the "seq" instances interleaved in one grid) + the
    # out-of-place bind of the shared C ahead of it; the first launch (tables of 2^logn entries) is timed under its own name
    ks = res["stateful"]["kernels_ms_total"]; kl = res["stateful"]["kernels_launches"]
    first_ms = ks.get("k_sc_round_mixed_first", 0.0)
    mix_ms, mix_n = ks.get("k_sc_round_mixed", 0.0) + first_ms, kl.get("k_sc_round_mixed", 0) + kl.get("k_sc_round_mixed_first", 0)
    rest_comb_ms = ks.get("k_sc_comb_bind_eval", 0.0) + ks.get("k_sc_comb_bind_eval_first", 0.0) + ks.get("k_sc_bind_eval_cubic_stream", 0.0)
    small_ms = ks.get("k_sc_bind_eval_cubic", 0.0) + ks.get("k_bind_top", 0.0)
    if mix_ms and mix_n:
        unit = n * 32                                                  # one table of the first round
        per_round0 = ((2 * NPAR + 3 * NSEQ) * 1.5 + 0.5) * unit         # 42 tables read once, their bound halves written once, the bound shared C read once
        geo = sum(0.5 ** j for j in range(mix_n))
        # from the second streaming round on the kernel binds the shared C itself (reads it unbound: 1 unit, writes the bound half: 0.5) instead of reading a pre-bound copy (0.5)
        fused_c = kl.get("k_bind_oop", 0) < mix_n
        alg_mix = per_round0 * geo + (unit * sum(0.5 ** j for j in range(1, mix_n)) if fused_c else 0.0)
        ach = alg_mix / (mix_ms * 1e-3) / 1e9
        bind_c_ms = ks.get("k_bind_oop", 0.0)
        alg_stream = table_bytes * 1.5 * geo                            # + the shared C's own bind (read 1, write 1/2)
        res["roofline"] = {"bound": "hbm", "kernel": "k_sc_round_mixed (ONE launch per streaming round: 12 'par' instances on the combined code path + 6 'seq' instances, interleaved blocks)",
                           "achieved": round(ach, 1), "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": round(ach / HBM_PEAK_GBS, 4), "traffic": None, "launches": mix_n,
                           "kernel_avg_ms": round(mix_ms / mix_n, 4), "algorithmic_bytes_per_launch": int(alg_mix / mix_n), "kernel_ms_total": round(mix_ms, 3),
                           "note": "kernel-only (HIP events on the context's stream), per launch averaged over its %d launches of one sumcheck (table bytes halve per round)" % mix_n,
                           "largest_launch": {"what": "the first bind: 42 tables of 2^%d entries (+ the bound shared C)" % logn, "kernel_ms": round(first_ms, 4), "algorithmic_bytes": int(per_round0),
                                              "GBps": round(per_round0 / (first_ms * 1e-3) / 1e9, 1) if first_ms else None, "frac": round(per_round0 / (first_ms * 1e-3) / 1e9 / HBM_PEAK_GBS, 4) if first_ms else None},
                           "streaming_rounds_all_kernels": {"kernels": "k_sc_round_mixed + k_bind_oop (the shared C's own bind: only ahead of the first round, the later rounds bind it in the kernel)", "kernel_ms": round(mix_ms + bind_c_ms, 3), "algorithmic_bytes": int(alg_stream),
                                                            "GBps": round(alg_stream / ((mix_ms + bind_c_ms) * 1e-3) / 1e9, 1), "frac": round(alg_stream / ((mix_ms + bind_c_ms) * 1e-3) / 1e9 / HBM_PEAK_GBS, 4)},
                           "all_fused_rounds": {"kernel_ms": round(mix_ms + bind_c_ms + rest_comb_ms + small_ms, 3), "algorithmic_bytes": int(alg_fused_rounds),
                                                "GBps": round(alg_fused_rounds / ((mix_ms + bind_c_ms + rest_comb_ms + small_ms) * 1e-3) / 1e9, 1),
                                                "note": "incl. the rounds below 2^14 index pairs (combined / per-instance single-launch kernels, launch-latency bound)"}}
        st = stored_traffic("sumcheck", "18x2^%d" % logn, "k_sc_round_mixed<*>") or stored_traffic("sumcheck", "18x2^%d" % logn, "k_sc_round_mixed")
        if st:
            res["roofline"]["traffic"] = int(st[0])
            st1 = stored_traffic("sumcheck", "18x2^%d" % logn, "k_sc_round_mixed<true>")
            if st1:
                res["roofline"]["largest_launch"]["traffic"] = int(st1[0])
            res["roofline"]["traffic_source"] = st[1] + " (stored rocprofv3 --pmc passes of tools/bench_sumcheck.py at this size: average per launch; not measured by this run)"
    ke = res["separate"]["kernels_ms_total"]
    if ke.get("k_sc_eval_cubic") and ke.get("k_bind_top"):
        res["separate"]["eval_GBps"] = round(2 * table_bytes / (ke["k_sc_eval_cubic"] * 1e-3) / 1e9, 1)
        res["separate"]["bind_GBps"] = round(2 * table_bytes * 1.5 / (ke["k_bind_top"] * 1e-3) / 1e9, 1)
    res["parity"] = "stateful driver: the combined sums of all %d rounds and the 43 final claims bit-exact vs the CPU oracle's prove_cubic_batched loop on the same tables; fused and separate drivers agree with it on all 43 final values" % logn
    return res


def group_block(sbn, ol, torch, devices, L, Rc, log_n):
    """SURVEY 8e from ONE process: the C ABI's device groups (sbn_group_*, csrc/abi_group.inc).  ONE L x Rc matrix committed by
    interleaved rows (host matrix: the figure includes PCIe) and ONE 2^log_n MSM by base-point ranges with resident points and
    device-resident scalar slices; both parity-gated (sampled rows vs the oracle; the discrete-log identity)."""
    g = sbn.Group(devices)
    N = len(devices)
    res = {"devices": devices, "driver": "one process, one host thread per device inside the library; no collective"}
    try:
        gb, gxy = g.gens_new(Rc, b"gens_r1cs_eval")
        c0 = g.ctx(0)
        Z = torch.empty(32 * L * Rc, dtype=torch.uint8, device=f"cuda:{devices[0]}")
        c0.scalars_synthetic(SEED, 1 << 40, L * Rc, Z.data_ptr())
        Z.view(L, Rc * 32)[(3 * L // 4):] = 0
        torch.cuda.synchronize()
        Zh = Z.cpu().numpy(); del Z
        out, _ = g.commit_rows(gb, Zh, None, L, Rc)
        for i in (0, 1, N, L // 2 + 1, 3 * L // 4 - 1, L - 1):
            row = Zh[32 * Rc * i:32 * Rc * (i + 1)].tobytes()
            if out[64 * i:64 * i + 64] != ol.commit(row, bytes(32), gxy[:64 * Rc], gxy[64 * Rc:]):
                raise SystemExit(f"group: row {i} differs from the oracle")
        t0 = time.perf_counter(); reps = 3
        for _ in range(reps):
            g.commit_rows(gb, Zh, None, L, Rc)
        dt = (time.perf_counter() - t0) / reps
        res["hyrax_rows"] = {"shape": f"{L}x{Rc}", "ms_per_commit_incl_pcie": round(dt * 1e3, 2), "pairs_per_s": round(L * Rc / dt, 1), "sharding": f"row i on device i mod {N}, no reduction",
                             "parity": "6 sampled rows bit-exact vs the CPU oracle", "note": "host-pointer entry point: the 1 GiB matrix crosses PCIe inside the timed call"}
        # the same commitment from DEVICE-resident rows (sbn_group_commit_rows_dev): device d holds rows d, d + N, ... — nothing but L x 64 B crosses PCIe
        import numpy as np
        Zr = Zh.reshape(L, Rc * 32)
        zs = [torch.from_numpy(np.ascontiguousarray(Zr[d::N])).to(f"cuda:{devices[d]}") for d in range(N)]
        torch.cuda.synchronize()
        out_dev, _ = g.commit_rows_dev(gb, [t.data_ptr() for t in zs], None, L, Rc)
        if out_dev != out:
            raise SystemExit("group: device-resident row commit differs from the host-matrix one")
        t0 = time.perf_counter()
        for _ in range(reps):
            g.commit_rows_dev(gb, [t.data_ptr() for t in zs], None, L, Rc)
        dt = (time.perf_counter() - t0) / reps
        res["hyrax_rows_dev"] = {"shape": f"{L}x{Rc}", "ms_per_commit": round(dt * 1e3, 2), "pairs_per_s": round(L * Rc / dt, 1), "sharding": f"device d holds rows d, d + {N}, ...; no reduction",
                                 "parity": "all rows equal to the host-matrix commit (itself checked on sampled rows against the oracle)"}
        del zs
        # Derefs::commit over the group from device-resident inputs (sbn_group_gather_commit): replicated eq tables + per-circuit address arrays,
        # each device gathers and commits only its rows; against ONE context's sbn_gather_merge + sbn_commit_table
        if L * Rc == 1 << 25:
            nops, lm = 1 << 22, 21
            rx, ry = splitmix_scalars(lm, SEED + 5), splitmix_scalars(lm, SEED + 6)
            rng = np.random.default_rng(7)
            addrs = [rng.integers(0, 1 << (lm - 1), size=nops, dtype=np.uint32) for _ in range(6)]
            mem, aptr, keep = [], [], []
            for d in range(N):
                cx = g.ctx(d)
                tx, ty = cx.eq_evals(rx), cx.eq_evals(ry)
                at = [torch.from_numpy(a.view(np.int32)).to(f"cuda:{devices[d]}") for a in addrs]
                keep.append((tx, ty, at)); mem.append([tx] * 3 + [ty] * 3); aptr.append([t.data_ptr() for t in at])
            torch.cuda.synchronize()
            comb = c0.gather_merge(mem[0], aptr[0], nops)
            want, _ = g.gather_commit(gb, mem, aptr, nops, L, Rc)
            t0 = time.perf_counter()
            for _ in range(reps):
                g.gather_commit(gb, mem, aptr, nops, L, Rc)
            dt = (time.perf_counter() - t0) / reps
            # parity: sampled rows of the merged polynomial against the oracle
            combh = c0.table_download(comb)
            for i in (0, 1, N, L // 2 + 1, 3 * L // 4 - 1, L - 1):
                if want[64 * i:64 * i + 64] != ol.commit(combh[32 * Rc * i:32 * Rc * (i + 1)], bytes(32), gxy[:64 * Rc], gxy[64 * Rc:]):
                    raise SystemExit(f"group gather_commit: row {i} differs from the oracle")
            res["derefs_gather_commit"] = {"shape": f"{L}x{Rc}", "ms_per_commit": round(dt * 1e3, 2), "what": "deref_mem + merge + commit_inner from device-resident eq tables and address arrays, rows dealt i mod N",
                                           "parity": "6 sampled rows bit-exact vs the CPU oracle's commitment of the gathered polynomial"}
            comb.free()
            for tx, ty, _ in keep:
                tx.free(); ty.free()
        gb.free(); del Zh
        n = 1 << log_n
        gr = g.bases_synthetic_ranges(n, S0.to_bytes(32, "little"), DSTEP.to_bytes(32, "little"))
        slices, want_sum = [], 0
        for d in range(N):
            lo, hi = gr.range(d)
            t = torch.empty(32 * (hi - lo), dtype=torch.uint8, device=f"cuda:{devices[d]}")
            g.ctx(d).scalars_synthetic(SEED, lo, hi - lo, t.data_ptr())
            torch.cuda.synchronize(devices[d])
            want_sum = (want_sum + int.from_bytes(dlog_expect(t, lo, hi - lo), "little")) % R_MOD
            slices.append(t)
        got, inf = g.msm_bases_dev(gr, [t.data_ptr() for t in slices])
        if got != ol.g1_mul(G_XY, want_sum.to_bytes(32, "little")):
            raise SystemExit("group: the folded MSM differs from the discrete-log identity")
        t0 = time.perf_counter(); reps = 3
        for _ in range(reps):
            g.msm_bases_dev(gr, [t.data_ptr() for t in slices])
        dt = (time.perf_counter() - t0) / reps
        res["msm"] = {"total_points": n, "ms_per_msm": round(dt * 1e3, 3), "points_per_s": round(n / dt, 1), "sharding": f"{N} contiguous base-point ranges, {N} x 64 B folded on the host (sbn_g1_sum)",
                      "parity": "bit-exact vs the discrete-log identity"}
        gr.free()
    finally:
        g.close()
    return res


def prove_stages_block(ctx, sbn, lookup_bytes):
    """BASELINE config 5: the device-side stages of one keyless-shaped SNARK::prove (Hyrax mode), issued by COMPILED code through the
    C ABI (spartan-bn254_amd/harness/prove_stages.cpp: the call sequence of the Rust shim in INTEGRATION.md), timed per stage under the
    names of the reference's benchmark (examples/keyless_benchmark.rs:171-238).  Parity gate first: the same harness at 2^-14 of the
    size with its trace on, replayed against the CPU oracle (tests/harness_model.py) — every commitment, round value and final claim."""
    import harness_model
    from spartan_bn254_amd import binding
    t0 = time.perf_counter()
    for stateful in (True, False):
        _, digest, trace, rounds = binding.harness_prove(ctx, 8, 7, 6, stateful=stateful, seed=11, trace_cap=8 << 20)
        got = harness_model.replay(trace, 8, 7, 6, seed=11)
        if got["digest"] != digest:
            raise SystemExit("prove_stages: the small harness run does not replay against the oracle")
    gate_s = time.perf_counter() - t0
    LO, LM, LC = 22, 21, 20
    out = {}
    for name, stateful in (("stateful_sumcheck", True), ("per_instance_sumcheck", False)):
        # three proves back to back on one setup (generator sets, their lookup tables, address arrays: per-circuit); the fastest is reported
        stages, digest, _, rounds = binding.harness_prove(ctx, LO, LM, LC, stateful=stateful, lookup_bytes_sat=16 << 30, lookup_bytes_eval=lookup_bytes, seed=11, passes=3)
        tot = sum(stages[k] for k in binding.HARNESS_STAGES[:6])
        out[name] = {"total_device_side_ms": round(tot, 2), "stage_ms": {k: round(stages[k], 3) for k in binding.HARNESS_STAGES[:6]},
                     "detail_ms": {k[4:]: round(stages[k], 3) for k in binding.HARNESS_STAGES[6:]}, "rounds": rounds, "transcript_digest": digest.hex()[:16]}
    if out["stateful_sumcheck"]["transcript_digest"] != out["per_instance_sumcheck"]["transcript_digest"]:
        raise SystemExit("prove_stages: the two sumcheck drivers absorbed different values at full size")
    st = out["stateful_sumcheck"]
    names = {"r1cs_sat_proof": "R1CS sat proof", "eq_evals": "EqPolynomial evaluation", "derefs_computation": "Derefs computation", "derefs_commitment": "Derefs commitment",
             "network_construction": "Network construction", "network_proof": "Network proof"}
    pub = {"r1cs_sat_proof": 3.45, "eq_evals": 0.10, "derefs_computation": 0.14, "derefs_commitment": 166.2, "network_construction": 4.07, "network_proof": 34.5}
    return {"workload": "keyless-shaped SNARK::prove (Hyrax): num_cons = num_vars = 2^20, 6 sparse polynomials of 2^22 ops over 2^21 memory cells (SURVEY App. C); synthetic tables, "
                        "uniform Fr; SHA3 chain in place of the Merlin transcript; fastest of three proves on one setup (generator sets, window / lookup tables, address arrays: per-circuit setup, outside the timed stages)",
            "driver": "compiled C++ caller of the C ABI (libsbn_prove_harness.so), one ABI call per sumcheck round",
            "stages": [{"stage": names[k], "ms": st["stage_ms"][k], "reference_published_s_M2Max_1thread": pub[k]} for k in binding.HARNESS_STAGES[:6]],
            "total_device_side_ms": st["total_device_side_ms"], "transcript_digest": st["transcript_digest"], "reference_published_total_prove_s": 208.8,
            "detail_ms": st["detail_ms"], "rounds": st["rounds"], "per_instance_sumcheck_calls": out["per_instance_sumcheck"],
            "not_included": "host-side Rust control flow: Instance evaluations (sparse, keyless_benchmark.rs:185-188), SpMV Az/Bz/Cz, the Sigma-protocol steps of the ZK sumchecks "
                            "(3-5 point commitments per round), Merlin hashing — they stay in Rust; the published figures include them",
            "parity": "the same harness at 2^-14 of the size, both sumcheck drivers: every absorbed value (commitments, %d+ round values, final claims, bullet L/R) replayed against the CPU oracle (%.1f s); "
                      "at full size both drivers end in the same transcript digest" % (got["records_checked"], gate_s)}


if __name__ == "__main__":
    main()
