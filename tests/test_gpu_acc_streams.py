"""GPU: a context's bucket jobs in a row, beside other contexts, on a caller's stream and after a refused call, with the MSM's helper kernels at raised
wave priority (fp.cuh: wave_prio_helper) and k_acc_extra's grid sized from the plan (msm_host.hpp: launch_accumulate).  Neither changes what a kernel
computes, so every case compares bit for bit with the oracle.  What the cases drive is what a change of WHO RUNS WHEN around the accumulate could
break: workspace reused by back-to-back calls with other contents, k_acc_extra's segments (a grid of 37 and 55 blocks here, not 2048) feeding k_acc_merge on
both of its paths, several contexts on one device, the row commit that shares launch_accumulate, a caller's stream, the call after a refused one.
They were written for the accumulate on a low-priority stream of its own (measured and dropped) and pass with and without it.

The derefs key build (abi_derefs_key.inc) goes through the same launch_accumulate; tests/test_gpu_sparse_eval_kzg.py holds it against its model and
needs that model's whole instance to do so, which is not repeated here.
"""
import random
import threading

import pytest

import acc_model as am
import window_model as wm
from conftest import rand_scalars
from test_gpu_acc_geometry import check_acc, set_env
from test_gpu_window_widths import _context_with, expect_from_dlogs, profiled, tiled_bases, to_bytes

pytestmark = pytest.mark.gpu

N_SMALL = 3008                    # c = 7, segments of 8, two lanes per bucket, one-level sort
N_TWO_LEVEL = 1 << 13             # with SBN_SORT2_MIN=8192 and SBN_MSM_GLV=1: GLV halves through the two-level sort, the headline's code path at its smallest
DISTINCT = 7


@pytest.fixture(scope="module")
def ctx_headline(sbn):
    c = _context_with(sbn, SBN_SORT2_MIN=N_TWO_LEVEL, SBN_MSM_GLV=1)
    yield c
    c.close()


@pytest.fixture(scope="module")
def shared(ol):
    """the bases of every single MSM here (7 distinct points, tiled) with their discrete logs"""
    return tiled_bases(ol, N_TWO_LEVEL, DISTINCT)


def want_msm(ol, pr, sc, shared):
    pts, dl = shared
    n = len(sc) // 32
    want = expect_from_dlogs(ol, pr, sc, dl[:32 * n])
    assert want == ol.msm_pippenger(sc, pts[:64 * n], 8)
    return want


def test_back_to_back_calls_reuse_the_workspace(ctx_headline, ol, pr, monkeypatch, shared):
    """eight MSMs on one context, the size and the scalars changing from call to call: `sorted`, `hist` and `buckets` of a call hold other contents
    than the call before left there, and nothing but stream order keeps a call's accumulate off them until its sort is done"""
    set_env(monkeypatch)
    cx = ctx_headline
    sets = {(n, s): rand_scalars(n, 9100 + s + n) for n in (N_SMALL, N_TWO_LEVEL) for s in (0, 1)}
    want = {k: want_msm(ol, pr, sc, shared) for k, sc in sets.items()}
    b = cx.bases_upload(shared[0])
    try:
        for i in range(8):
            n, s = (N_SMALL, N_TWO_LEVEL)[i % 2], (i // 2) % 2
            out, inf = cx.msm_bases(b, sets[(n, s)])
            job = cx.prof_last_job()
            if n == N_SMALL:
                assert (job["c"], job["slots"]) == (7, wm.make_shape(7).W * n) and cx.prof_last_acc()["LPB"] == 2
            else:
                assert job["slots"] == 2 * n * job["W"] and job["W"] == wm.make_shape(job["c"], 127).W          # GLV: 2 n half-scalars of 127 bits
            assert out == want[(n, s)] and not inf, i
    finally:
        b.free()


@pytest.mark.parametrize("n,LPB", [(2000, 1), (N_SMALL, 2)])
def test_skewed_loads_through_extra_and_merge(ctx, ol, pr, monkeypatch, n, LPB):
    """loads of SEG + 1, 13 SEG and 13 SEG + 1 in one bucket each at SEG = 8 (the rule for 512 .. 4096 terms): k_acc_extra's segments (thousands of
    items over a grid sized from the plan's capacity: 37 and 55 blocks) are folded by k_acc_merge, by one lane (k = 1, 12) and by a wave (k = 13)"""
    env = set_env(monkeypatch)
    c, SEG = 7, 8
    W = wm.make_shape(c).W
    windows = {W // 2: [SEG + 1, 13 * SEG, 13 * SEG + 1]}
    n_edge = len(am.edge_scalars(c, W, SEG, windows))
    fill = am.masked_uniform(n - n_edge, n, c, list(windows))
    edge, plan = am.edge_plan(c, W, SEG, windows, am.loads_of(fill, c, W))
    sc = edge + fill
    assert len(sc) == n and sorted(plan[W // 2]) == sorted(windows[W // 2])
    random.Random(n).shuffle(sc)
    loads = am.loads_of(sc, c, W)
    assert all(loads.get((W // 2, bk), 0) == t for t, bk in plan[W // 2].items())
    lane, wave = am.merge_paths(loads, SEG)
    assert lane >= 2 and wave >= 1
    blob = to_bytes(sc)
    pts, dl = tiled_bases(ol, n, DISTINCT)
    with profiled(ctx) as ran:
        out, inf = ctx.msm(blob, pts)
        ran = ran()
    assert ran["k_acc_first"][1] == 1 and ran["k_acc_extra"][1] == 1 and ran["k_acc_merge"][1] == 1, ran
    acc = check_acc(ctx, am.SINGLE, n, W, n, c, env, loads)          # extra_count and big_count are the ones these loads give
    assert (acc["SEG"], acc["LPB"]) == (SEG, LPB) and acc["extra_count"] >= 1 + 12 + 13 and acc["big_count"] >= 3
    assert out == expect_from_dlogs(ol, pr, blob, dl) and not inf
    assert out == ol.msm_pippenger(blob, pts, 8)


def test_three_contexts_on_three_host_threads(sbn, ol, pr, monkeypatch, shared):
    """three contexts on one device, four MSMs each with scalars of their own over ONE handle: each context's raised-priority helper waves run beside
    the other contexts' accumulate"""
    set_env(monkeypatch)
    cxs = [_context_with(sbn, SBN_SORT2_MIN=N_TWO_LEVEL, SBN_MSM_GLV=1) for _ in range(3)]
    b = cxs[0].bases_upload(shared[0])
    ks = [[rand_scalars(N_TWO_LEVEL, 9300 + 10 * t + i) for i in range(4)] for t in range(3)]
    want = [[expect_from_dlogs(ol, pr, k, shared[1]) for k in row] for row in ks]
    got = [[None] * 4 for _ in range(3)]

    def work(t):
        for i in range(4):
            got[t][i] = cxs[t].msm_bases(b, ks[t][i])
    try:
        th = [threading.Thread(target=work, args=(t,)) for t in range(3)]
        for t in th:
            t.start()
        for t in th:
            t.join()
        assert [[g[0] for g in row] for row in got] == want and not any(g[1] for row in got for g in row)
        assert want[0][0] == ol.msm_pippenger(ks[0][0], shared[0], 8)
    finally:
        b.free()
        for cx in cxs:
            cx.close()


def test_small_row_commit_on_the_bucket_path(ctx, ol, monkeypatch):
    """8 rows x 64 columns, no lookup table: run_bucket_job in row mode over the same launch_accumulate, the sums fetched through the host mailbox"""
    set_env(monkeypatch)
    L, R = 8, 64
    bases, gxy = ctx.gens_new(R, b"gens_acc_streams")
    try:
        G, h = gxy[:64 * R], gxy[64 * R:]
        for seed, blinds in ((1, None), (2, rand_scalars(L, 9402))):
            Z = rand_scalars(L * R, 9400 + seed)
            with profiled(ctx) as ran:
                out, infs = ctx.commit_rows(bases, Z, blinds, L, R)
                ran = ran()
            assert "k_acc_first" in ran and "k_comb_rows" not in ran, sorted(ran)
            assert out == ol.commit_rows(Z, blinds, L, R, G, h, 4) and not any(infs)
    finally:
        bases.free()


def test_a_callers_stream_gives_the_same_results(ctx_headline, ol, pr, monkeypatch, shared):
    """sbn_ctx_set_stream with a torch stream (the caller owns the ordering), then back to null (the context's own stream), twice"""
    import torch
    set_env(monkeypatch)
    cx = ctx_headline
    sets = [rand_scalars(n, 9500 + n) for n in (N_SMALL, N_TWO_LEVEL)]
    want = [want_msm(ol, pr, sc, shared) for sc in sets]
    b = cx.bases_upload(shared[0])
    s = torch.cuda.Stream()
    try:
        for stream in (s.cuda_stream, 0, s.cuda_stream, 0):
            cx.set_stream(stream)
            assert [cx.msm_bases(b, sc) for sc in sets] == [(w, False) for w in want], stream
    finally:
        cx.set_stream(0)
        b.free()


def test_the_call_after_a_refused_one(sbn, ol, pr, monkeypatch, shared):
    """one scalar >= r: the kernels count it, the call returns SBN_EINVAL after its stream has drained; the next MSM on the context gives the right
    point, and so does a larger one that frees and regrows the workspace"""
    set_env(monkeypatch)
    cx = _context_with(sbn, SBN_SORT2_MIN=N_TWO_LEVEL, SBN_MSM_GLV=1)
    pts, dl = shared
    good = rand_scalars(N_SMALL, 9600)
    bad = bytearray(good); bad[32 * 1000:32 * 1001] = wm.R.to_bytes(32, "little")
    large = rand_scalars(N_TWO_LEVEL, 9601)
    b = cx.bases_upload(pts)
    try:
        assert cx.msm_bases(b, good) == (want_msm(ol, pr, good, shared), False)
        with pytest.raises(sbn.SbnError, match="rc=-1.*not canonical"):
            cx.msm_bases(b, bytes(bad))
        assert cx.msm_bases(b, good) == (want_msm(ol, pr, good, shared), False)
        assert cx.msm_bases(b, large) == (want_msm(ol, pr, large, shared), False)
        with pytest.raises(sbn.SbnError, match="rc=-1.*not canonical"):
            cx.msm_bases(b, bytes(bad))
        assert cx.msm_bases(b, large) == (want_msm(ol, pr, large, shared), False)
    finally:
        b.free()
        cx.close()
