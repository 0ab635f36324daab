"""GPU: the segment, lane-split and merge edges of the bucket accumulate (k_size_*, k_acc_first<G>, k_acc_extra, k_acc_merge) and the
shapes of the reduction (k_reduce_l1, k_reduce_combine[_quad]), each driven on purpose and compared bit for bit.

Every case (1) builds scalars whose per-bucket loads are known from the model (tests/acc_model.py: loads derived from the scalars with
the window model's recoding, never assumed), (2) asserts through prof_last_acc that the geometry the host took (SEG, LPB, L, chunks,
combine launches, quad) is the one the model gives, and that the device counters extra_count / big_count are the ones the loads give
— so a case whose input misses its seam fails instead of passing quietly — and (3) compares the result with the discrete-log identity
(fr_dot, then one g1_mul) and, up to 10000 terms, with the oracle's Pippenger.

The load set (acc_model.load_set), each load in a bucket of its own: 0, 1, 2, 3; SEG - 1, SEG, SEG + 1; 2 SEG - 1, 2 SEG, 2 SEG + 1;
13 SEG (k = 12: the last merge by one lane, a full last segment); 13 SEG + 1 (k = 13: the first merge by a wave, a one-entry last
segment); 65 SEG + 1 (k = 65: lane 0 of the wave takes two partials).  The longest goes to bucket 0 of a window, the second longest to
its last bucket (digit -2^(c-1)).  Bases are 7 distinct points tiled, so a segment is made of repeats: P + P in every chain.
"""
import random

import pytest

import acc_model as am
import window_model as wm
from conftest import rand_scalars
from test_glv_cpu import LAM, split
from test_gpu_msm import DSTEP, S0, _dot_arith
from test_gpu_window_widths import _context_with, expect_from_dlogs, pool, profiled, tiled_bases, to_bytes

pytestmark = pytest.mark.gpu

SEGS = [8, 32, 64, 256, 8192]
DISTINCT = 7


@pytest.fixture(scope="module")
def ctx_sort2(sbn):
    c = _context_with(sbn, SBN_SORT2_MIN=1024)
    yield c
    c.close()


@pytest.fixture(scope="module")
def ctx_glv(sbn):
    c = _context_with(sbn, SBN_MSM_GLV=1, SBN_SORT2_MIN=1024)
    yield c
    c.close()


@pytest.fixture(scope="module")
def ctx_plain(sbn):
    c = _context_with(sbn, SBN_MSM_GLV=0)
    yield c
    c.close()


def set_env(monkeypatch, **env):
    """the overrides a job reads when it runs -> the same, as the model takes them"""
    for k in ("SBN_MSM_C", "SBN_MSM_SEG", "SBN_RED_L"):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, str(v))
    return {k: str(v) for k, v in env.items()}


def check_acc(ctx, mode, n, P, estride, c, env, loads):
    """model == host for the six host values, model == device for the two counters"""
    acc = ctx.prof_last_acc()
    assert am.geometry_of(acc) == am.geometry(mode, n, P, estride, c, env), acc
    assert (acc["extra_count"], acc["big_count"]) == am.expected_counters(loads, acc["SEG"]), acc
    return acc


def has_loads(loads, w, want):
    return set(want) <= {loads.get((w, b), 0) for b in range(max(b for _, b in loads) + 2)}


def windows_for(c, W, SEG):
    """first, middle and top window with the whole load set; with segments of ACC_SEG_MAX the set goes to the middle window alone
    (nine segments' worth of entries once) and the small loads to the other two"""
    if SEG < am.ACC_SEG_MAX:
        return [0, W // 2, W - 1]
    return {0: [3, 2, 1, 0], W // 2: am.load_set(SEG), W - 1: [3, 2, 1]}


def seam_job(c, SEG, n_min, seed, bits=254, windows=None):
    """scalars (integers, shuffled) of at least n_min terms: the load set in three windows, uniform scalars that leave those windows
    alone around it -> (scalars, loads, {window: {load: bucket}})"""
    W = wm.make_shape(c, bits).W
    windows = windows_for(c, W, SEG) if windows is None else windows
    n_edge = len(am.edge_scalars(c, W, SEG, windows, None, bits))
    fill = am.masked_uniform(max(600, n_min - n_edge), seed, c, list(windows), bits)
    edge, plan = am.edge_plan(c, W, SEG, windows, am.loads_of(fill, c, W), bits)
    sc = edge + fill
    random.Random(seed).shuffle(sc)
    loads = am.loads_of(sc, c, W)
    for w, placed in plan.items():
        assert all(loads.get((w, b), 0) == t for t, b in placed.items())
    return sc, loads, plan


def run_single(ctx, ol, pr, sc, c, W, env, loads, LPB):
    n = len(sc)
    blob = to_bytes(sc)
    pts, dl = tiled_bases(ol, n, DISTINCT)
    out, inf = ctx.msm(blob, pts)
    job = ctx.prof_last_job()
    assert (job["c"], job["W"], job["slots"], job["buckets"]) == (c, W, W * n, W << (c - 1))
    acc = check_acc(ctx, am.SINGLE, n, W, n, c, env, loads)
    assert acc["LPB"] == LPB
    assert out == expect_from_dlogs(ol, pr, blob, dl) and not inf
    if n <= 10000:
        assert out == ol.msm_pippenger(blob, pts, 8)
    return acc


# ---- a / b: the segment seams with one and with two lanes per bucket ------------------------------------------------------
@pytest.mark.parametrize("SEG", SEGS)
def test_segment_seams_one_lane_per_bucket(ctx, ol, pr, monkeypatch, SEG):
    """c = 12, fewer than 47 x 2048 terms: mean load below 48, k_acc_first<1>"""
    c, W = 12, wm.make_shape(12).W
    env = set_env(monkeypatch, SBN_MSM_C=c, SBN_MSM_SEG=SEG)
    sc, loads, plan = seam_job(c, SEG, 0, 100 + SEG)
    assert len(sc) < 47 * 2048
    assert sorted(plan[W // 2]) == sorted(am.load_set(SEG))
    acc = run_single(ctx, ol, pr, sc, c, W, env, loads, 1)
    assert acc["SEG"] == SEG
    lane, wave = am.merge_paths(loads, SEG)
    assert lane >= 4 and (wave >= 6 or SEG == am.ACC_SEG_MAX)


@pytest.mark.parametrize("SEG", SEGS)
def test_segment_seams_two_lanes_per_bucket(ctx, ol, pr, monkeypatch, SEG):
    """c = 7, at least 3008 terms: mean load 48, k_acc_first<2>.  Loads 1 and 3 leave the second lane an empty and a shorter part, a bucket
    past SEG gets its extras folded into slot 0 while slot 1 keeps the second lane's part: any slot mix-up changes the sum."""
    c, W = 7, wm.make_shape(7).W
    env = set_env(monkeypatch, SBN_MSM_C=c, SBN_MSM_SEG=SEG)
    sc, loads, plan = seam_job(c, SEG, 3008, 200 + SEG)
    assert len(sc) >= 3008
    assert sorted(plan[W // 2]) == sorted(am.load_set(SEG)) and {1, 3} <= set(plan[0 if SEG == am.ACC_SEG_MAX else W // 2])
    acc = run_single(ctx, ol, pr, sc, c, W, env, loads, 2)
    assert acc["SEG"] == SEG


# ---- c: the rule's own edge ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,LPB", [(3007, 1), (3008, 2)])
def test_lanes_per_bucket_flip_at_mean_48(ctx, ol, pr, monkeypatch, n, LPB):
    """no override: 512 .. 4096 terms take c = 7 and segments of 8; 3008 / 64 + 1 = 48 is the first mean that splits a bucket over two lanes"""
    env = set_env(monkeypatch)
    c, W = 7, wm.make_shape(7).W
    assert am.choose_c(n, False, am.MSM_C_MAX, 1) == c
    windows = [0, W // 2, W - 1]
    n_edge = len(am.edge_scalars(c, W, 8, windows))
    fill = am.masked_uniform(n - n_edge, n, c, windows)
    edge, plan = am.edge_plan(c, W, 8, windows, am.loads_of(fill, c, W))
    sc = edge + fill
    assert len(sc) == n                                    # (the filler leaves the three windows alone: no bucket needed less topping up)
    random.Random(n).shuffle(sc)
    loads = am.loads_of(sc, c, W)
    assert has_loads(loads, W // 2, am.load_set(8))
    acc = run_single(ctx, ol, pr, sc, c, W, env, loads, LPB)
    assert acc["SEG"] == 8


# ---- d: the two-level sort and GLV feeding the same kernels -----------------------------------------------------------------
def test_segment_seams_behind_the_two_level_sort(ctx_sort2, ol, pr, monkeypatch):
    c, W, SEG = 13, wm.make_shape(13).W, 8
    env = set_env(monkeypatch, SBN_MSM_C=c, SBN_MSM_SEG=SEG)
    sc, loads, plan = seam_job(c, SEG, 10277, 1313)
    assert len(sc) == 10277 and all(sorted(plan[w]) == sorted(am.load_set(SEG)) for w in (0, W // 2, W - 1))
    with profiled(ctx_sort2) as ran:
        run_single(ctx_sort2, ol, pr, sc, c, W, env, loads, 1)
        ran = ran()
    assert "k_s2_place" in ran and "k_hist_lds" not in ran, sorted(ran)


def test_segment_seams_behind_glv(ctx_glv, ol, pr, monkeypatch):
    """3001 terms = 6002 half-scalars of 127 bits (estride = 2 n).  The load set is built over the HALVES (acc_model.glv_scalars pairs them
    into full scalars); test_glv_cpu.split, the model of the kernel's decomposition, says which halves every scalar gives, the uniform
    ones included, and the loads are counted over those."""
    c, SEG, n = 13, 8, 3001
    W = wm.make_shape(c, 127).W
    env = set_env(monkeypatch, SBN_MSM_C=c, SBN_MSM_SEG=SEG)
    windows = [0, W // 2, W - 1]
    n_edge = len(am.glv_scalars(am.edge_scalars(c, W, SEG, windows, bits=127), c, W, LAM, wm.R))
    rnd = random.Random(127)
    fill = [rnd.randrange(wm.R) for _ in range(n - n_edge - 5)]
    edge, plan = am.edge_plan(c, W, SEG, windows, am.loads_of([h for k in fill for h in split(k)], c, W), bits=127)
    sc = am.glv_scalars(edge, c, W, LAM, wm.R) + fill
    sc += [0] * (n - len(sc))                              # (two halves share a scalar; buckets the uniform halves loaded need less topping up)
    assert len(sc) == n
    random.Random(7).shuffle(sc)
    halves = [split(k) for k in sc]
    assert sum(1 for k1, k2 in halves if k1 and k2 and k2 < 1 << 120) >= 700 and all((k1 + LAM * k2) % wm.R == k for (k1, k2), k in zip(halves, sc))
    loads = am.loads_of([h for pair in halves for h in pair], c, W)
    assert all(loads.get((w, b), 0) == t for w in windows for t, b in plan[w].items())
    assert all(sorted(plan[w]) == sorted(am.load_set(SEG)) for w in windows)
    blob = to_bytes(sc)
    pts, dl = tiled_bases(ol, n, DISTINCT)
    b = ctx_glv.bases_upload(pts)
    try:
        with profiled(ctx_glv) as ran:
            out, inf = ctx_glv.msm_bases(b, blob)
            ran = ran()
        assert "k_glv_split" in ran, sorted(ran)
        job = ctx_glv.prof_last_job()
        assert (job["c"], job["W"], job["slots"]) == (c, W, 2 * n * W)
        check_acc(ctx_glv, am.SINGLE, 2 * n, W, 2 * n, c, env, loads)
        assert out == expect_from_dlogs(ol, pr, blob, dl) and not inf
        assert out == ol.msm_pippenger(blob, pts, 8)
    finally:
        b.free()


# ---- e: row commits (one bucket set per row, shared by its windows) ----------------------------------------------------------
@pytest.mark.parametrize("SEG", [8, 64])
def test_segment_seams_in_row_commits(ctx, ol, monkeypatch, SEG):
    """three rows of 3000 columns at c = 8: all zero; one scalar repeated (every bucket it touches holds 3000 entries or more); the
    load set in buckets 0 .. 12 and 127, columns with digits 65 .. 126 around it (buckets 64 .. 125, some twenty segments each)."""
    c, R, L = 8, 3000, 3
    W = wm.make_shape(c).W
    env = set_env(monkeypatch, SBN_MSM_C=c, SBN_MSM_SEG=SEG)
    n_edge = len(am.row_edge_columns(c, W, SEG, am.load_set(SEG))[0])
    fill = am.digit_range_columns(R - n_edge, 80 + SEG, c, W, 65, 126)
    cols, plan = am.row_edge_columns(c, W, SEG, am.load_set(SEG))
    row = cols + fill
    random.Random(SEG).shuffle(row)
    const = 0x1d3 | (0x7f << 8 * 9) | (1 << 250)
    rows = [[0] * R, [const] * R, row]
    blinds = [5, am.digit_range_columns(1, 1, c, W, 65, 126)[0], am.digit_range_columns(1, 2, c, W, 65, 126)[0]]
    pts, _ = pool(ol)
    G, h = pts[:64 * R], pts[64 * R:64 * R + 64]
    Z = b"".join(to_bytes(r) for r in rows)
    b = ctx.bases_upload(G, h)
    try:
        for bl in (blinds, None):
            full = [r + [bl[i]] for i, r in enumerate(rows)] if bl else rows
            loads = am.loads_of_rows(full, c, W)
            assert all(loads.get((2, bk), 0) == t for t, bk in plan.items()) and sorted(plan) == sorted(am.load_set(SEG))
            ncol = R + (1 if bl else 0)
            with profiled(ctx) as ran:
                out, infs = ctx.commit_rows(b, Z, to_bytes(bl) if bl else None, L, R)
                ran = ran()
            assert "k_acc_first" in ran and "k_comb_rows" not in ran and "k_merge_scalars" not in ran, sorted(ran)
            job = ctx.prof_last_job()
            assert (job["c"], job["W"], job["slots"], job["buckets"]) == (c, W, L * ncol * W, L << (c - 1))
            acc = check_acc(ctx, am.ROWS, ncol, L, ncol * W, c, env, loads)
            assert (acc["SEG"], acc["LPB"]) == (SEG, 1)
            assert out == ol.commit_rows(Z, to_bytes(bl) if bl else None, L, R, G, h, 16), bl is not None
            assert infs[0] == (0 if bl else 1)
    finally:
        b.free()


# ---- f: the shipped geometry under the automatic rule -----------------------------------------------------------------------
def synthetic_job(torch, ctx, n, seed, c, W, SEG, glv):
    """n uniform scalars from sbn_scalars_synthetic, the first block replaced by scalars that top chosen buckets of the first, a middle
    and the top window up to the load set, from SEG - 1 on: under a uniform fill of mean 2 SEG / 4 .. 2 SEG / 2 per bucket no bucket a
    scalar can reach holds 0 .. 3 entries (those loads are cases a - e's).  -> (device tensor, bytes, loads [W, 2^(c-1)])"""
    x = torch.empty((n, 8), dtype=torch.int32, device="cuda")
    ctx.scalars_synthetic(0xACC0 + seed, 0, n, x.data_ptr())
    torch.cuda.synchronize()
    raw = bytearray(x.cpu().numpy().tobytes())
    want = [t for t in am.load_set(SEG) if t >= SEG - 1]
    windows = {w: want for w in (0, W // 2, W - 1)}
    block = 3 * sum(want)                                  # no bucket needs more than its whole load
    bits = 127 if glv else 254

    def loads_of_blob(blob):
        if not glv:
            return am.loads_of_bytes(blob, c, W)
        halves = b"".join(h.to_bytes(16, "little") for i in range(0, len(blob), 32) for h in split(int.from_bytes(blob[i:i + 32], "little")))
        return am.loads_of_bytes(halves, c, W, 16)
    back = loads_of_blob(bytes(raw[32 * block:]))
    background = {(w, b): int(back[w, b]) for w in windows for b in list(range(64)) + [(1 << (c - 1)) - 1]}
    edge, plan = am.edge_plan(c, W, SEG, windows, background, bits)
    assert len(edge) <= block and all(b < 64 or b == (1 << (c - 1)) - 1 for p in plan.values() for b in p.values())
    if glv:
        assert all(split(k) == (k, 0) for k in set(edge))
    raw[:32 * block] = to_bytes(edge) + bytes(32 * (block - len(edge)))
    raw = bytes(raw)
    loads = back + loads_of_blob(raw[:32 * block])
    assert all(loads[w, b] == t for w in windows for t, b in plan[w].items())
    x.copy_(torch.frombuffer(bytearray(raw), dtype=torch.int32).reshape(n, 8))
    torch.cuda.synchronize()
    return x, raw, loads


@pytest.mark.parametrize("which,log_n", [("glv", 20), ("plain", 20), ("auto", 21)])
def test_shipped_geometry_with_the_load_set(ctx, ctx_plain, ol, pr, monkeypatch, which, log_n):
    import torch
    env = set_env(monkeypatch)
    cx = ctx_plain if which == "plain" else ctx
    n, first = 1 << log_n, 3
    glv = which == "glv"
    if glv:
        c = am.glv_c(n); W = wm.make_shape(c, 127).W
        geo = am.geometry(am.SINGLE, 2 * n, W, 2 * n, c)
        assert (c, W, geo) == (16, 8, (256, 2, 4, 128, 2, 1))
    else:
        c = am.choose_c(n, False, am.S2_C_MAX, 1, am.S2_C_MAX); W = wm.make_shape(c).W
        geo = am.geometry(am.SINGLE, n, W, n, c)
        assert (c, geo[:2]) == ((15, (256, 2)) if log_n == 20 else (17, (128, 1)))
    k, raw, loads = synthetic_job(torch, cx, n, log_n, c, W, geo[0], glv)
    b = cx.bases_synthetic(n, first, S0.to_bytes(32, "little"), DSTEP.to_bytes(32, "little"))
    try:
        out, inf = cx.msm_bases_dev(b, k.data_ptr(), n)
        job = cx.prof_last_job()
        rec = 2 * n if glv else n
        assert (job["c"], job["W"], job["slots"], job["buckets"]) == (c, W, rec * W, W << (c - 1))
        acc = check_acc(cx, am.SINGLE, rec, W, rec, c, env, loads)
        assert am.geometry_of(acc) == geo
        assert acc["big_count"] >= 3 * 6 and am.merge_paths(loads, geo[0])[1] >= 3 * 2
        assert out == ol.g1_mul(pr.point_to_xy(pr.G), _dot_arith(pr, raw, first, n)) and not inf
    finally:
        b.free()


# ---- g: the grid-stride loops -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c,log_n,seam", [(7, 17, "extra"), (9, 15, "wave"), (16, 19, "lane")])
def test_grid_stride_loops_of_extra_and_merge(ctx, ol, pr, monkeypatch, c, log_n, seam):
    """uniform scalars cut into segments of 8, at the smallest sizes that take k_acc_extra past its 2048 x 256 work items, k_acc_merge's
    wave loop past its 4096 blocks and its lane loop past its 4096 x 64 lanes"""
    import torch
    env = set_env(monkeypatch, SBN_MSM_C=c, SBN_MSM_SEG=8)
    n, first, W = 1 << log_n, 11, wm.make_shape(c).W
    x = torch.empty((n, 8), dtype=torch.int32, device="cuda")
    ctx.scalars_synthetic(0x6121D + c, 0, n, x.data_ptr())
    torch.cuda.synchronize()
    raw = x.cpu().numpy().tobytes()
    loads = am.loads_of_bytes(raw, c, W)
    lane, wave = am.merge_paths(loads, 8)
    b = ctx.bases_synthetic(n, first, S0.to_bytes(32, "little"), DSTEP.to_bytes(32, "little"))
    try:
        out, inf = ctx.msm_bases_dev(b, x.data_ptr(), n)
        assert ctx.prof_last_job()["c"] == c
        acc = check_acc(ctx, am.SINGLE, n, W, n, c, env, loads)
        assert acc["SEG"] == 8
        if seam == "extra":
            assert acc["extra_count"] > am.ACC_EXTRA_GRID
        elif seam == "wave":
            assert wave > am.MERGE_WAVE_GRID and acc["big_count"] == lane + wave
        else:
            assert lane > am.MERGE_LANE_GRID and acc["big_count"] == lane + wave > am.MERGE_LANE_GRID
        assert out == ol.g1_mul(pr.point_to_xy(pr.G), _dot_arith(pr, raw, first, n)) and not inf
    finally:
        b.free()


# ---- h: three combine levels, and the quad kernel on two ----------------------------------------------------------------------
@pytest.mark.parametrize("L,chunks,levels,quad", [(1, 8192, 3, 0), (64, 128, 2, 1)])
def test_combine_levels(ctx_sort2, ol, pr, monkeypatch, L, chunks, levels, quad):
    c, W, n = 20, wm.make_shape(20).W, 10277
    env = set_env(monkeypatch, SBN_MSM_C=c, SBN_RED_L=L)
    SEG = am.geometry(am.SINGLE, n, W, n, c, env)[0]
    sc, loads, _ = seam_job(c, SEG, 0, 2020)
    fill = am.masked_uniform(n - len(sc), 2021, c, [])
    sc += fill
    loads = am.loads_of(sc, c, W)
    assert len(sc) == n
    with profiled(ctx_sort2) as ran:
        acc = run_single(ctx_sort2, ol, pr, sc, c, W, env, loads, 1)
        ran = ran()
    assert (acc["L"], acc["chunks"], acc["levels"], acc["quad"]) == (L, chunks, levels, quad)
    assert ran["k_reduce_combine"][1] == levels and ran["k_reduce_l1"][1] == 1, ran


# ---- the getter itself ----------------------------------------------------------------------------------------------------------
def test_prof_last_acc_arguments_and_lookup_jobs(ctx, sbn, ol, monkeypatch):
    """a null out is refused; a commit through the lookup table runs no bucket job and leaves the values of the last one"""
    set_env(monkeypatch)
    assert sbn.lib().sbn_prof_last_acc(ctx.h, None) == -1
    sc = rand_scalars(700, 1)
    pts, _ = tiled_bases(ol, 700, 64)
    ctx.msm(sc, pts)
    before = ctx.prof_last_acc()
    assert (before["SEG"], before["LPB"]) == (8, 1)
    R = 16
    G, _ = pool(ol)
    b = ctx.bases_upload(G[:64 * R], G[64 * R:64 * R + 64])
    try:
        ctx.bases_precompute(b, 8 << 20)
        ctx.commit_rows(b, rand_scalars(2 * R, 2), None, 2, R)
        assert ctx.prof_last_job()["buckets"] == 0
        assert ctx.prof_last_acc() == before
    finally:
        b.free()
    fresh = sbn.Context(0)
    try:
        assert set(fresh.prof_last_acc().values()) == {0}
    finally:
        fresh.close()
