"""GPU: every window width of every MSM / commitment path, pinned by name and compared bit for bit with the oracle.

The window width c fixes where the signed digits are cut out of a scalar, the width of the top window, the bucket count 2^(c-1), the
template instance of the two-level sort and the index arithmetic of the lookup table.  Each case below sets ONE width, asserts through
prof_last_job that this width (and its window count) is what ran, asserts through the profile which kernels ran, and feeds the path
the seam scalars of that width (tests/window_model.py; tests/test_window_digits_cpu.py shows that they land on every seam) mixed with
uniform ones, over bases whose discrete logarithms are known.

  single MSM, one-level sort      c = 7 .. 16   (SBN_MSM_C)
  single MSM, two-level sort      c = 13 .. 22  (SBN_SORT2_MIN=1024, both SBN_SORT2_SPT)
  GLV single MSM (127-bit halves) c = 13 .. 17  (SBN_MSM_GLV=1)
  row commits, bucket method      c = 7 .. 16   (SBN_MSM_C), fused and generic row sort
  row commits, lookup table       c = 7 .. 17   (the budget of sbn_bases_precompute), k_comb_rows / _flat / _const
"""
import contextlib
import os

import pytest

import window_model as wm
from conftest import rand_scalars
from test_glv_cpu import LAM, split

pytestmark = pytest.mark.gpu

POOL = 13200                     # distinct points with known discrete logs (the widest generic-sort row needs 13108 + h)
_cache = {}


def pool(ol):
    if "pool" not in _cache:
        dl = rand_scalars(POOL, 20261)
        _cache["pool"] = (ol.g1_mul_gen_batch(dl, 16), dl)
    return _cache["pool"]


def tiled_bases(ol, n, distinct):
    """n bases made of `distinct` pool points, tiled (duplicates exercise P + P in the buckets)"""
    pts, dl = pool(ol)
    reps = (n + distinct - 1) // distinct
    return (pts[:64 * distinct] * reps)[:64 * n], (dl[:32 * distinct] * reps)[:32 * n]


def to_bytes(vals):
    return b"".join(v.to_bytes(32, "little") for v in vals)


def mixed_scalars(seams, n, seed):
    """the seam scalars repeated to length at the even positions, uniform scalars at the odd ones"""
    uni = rand_scalars((n + 1) // 2, seed)
    out = bytearray()
    for i in range(n):
        out += seams[(i // 2) % len(seams)].to_bytes(32, "little") if i % 2 == 0 else uni[32 * (i // 2):32 * (i // 2) + 32]
    return bytes(out)


def expect_from_dlogs(ol, pr, scalars, dlogs):
    return ol.g1_mul(pr.point_to_xy(pr.G), ol.fr_dot(scalars, dlogs))


@contextlib.contextmanager
def profiled(ctx):
    """profiling on for the block; the yielded function returns {label: (ms, launches)} of what ran inside it"""
    ctx.prof_enable(True); ctx.prof_reset()
    try:
        yield ctx.prof_get
    finally:
        ctx.prof_enable(False)


def _context_with(sbn, **env):
    old = {k: os.environ.get(k) for k in env}
    os.environ.update({k: str(v) for k, v in env.items()})
    try:
        return sbn.Context(0)              # SBN_SORT2_MIN / SBN_MSM_GLV are read when a context is created
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


@pytest.fixture(scope="module")
def ctx_sort2(sbn):
    """single MSMs take the two-level sort (sort2_kernels.cuh) from 1024 terms on instead of from 2^20"""
    c = _context_with(sbn, SBN_SORT2_MIN=1024)
    yield c
    c.close()


@pytest.fixture(scope="module")
def glv_pair(sbn):
    """(GLV forced, GLV off), both with the two-level sort from 1024 terms on, which the GLV path needs"""
    on, off = _context_with(sbn, SBN_MSM_GLV=1, SBN_SORT2_MIN=1024), _context_with(sbn, SBN_MSM_GLV=0, SBN_SORT2_MIN=1024)
    yield on, off
    on.close(); off.close()


# ---- single MSM, one-level sort ---------------------------------------------------------------------------------------------
# run_bucket_job: a sort block owns (window, bucket range r of R, entry chunk k of K).  R = 2^(c-1) / min(2^(c-1), sort_rs_max), and a
# context on gfx950 is granted 128 KiB of LDS per sort block, sort_rs_max = 32768 = 2^(MSM_C_MAX - 1): NO width the one-level sort accepts
# has more than one bucket range there (R > 1 needs the 64 KiB fallback of a device that refuses the grant), so no size reaches the
# r > 0 passes of k_hist_lds / k_scatter_lds on this hardware.  What the size does switch is K = min(ceil(1024 / W), n / 4096): one
# chunk per window below 8192 terms, two from 8192 on (the k > 0 prefix of k_block_prefix), and the segment rule (SEG = 8 up to 4096
# terms, 32 above).  The two sizes are the ragged neighbours of those edges: 3001 (K = 1, SEG = 8) and 8192 + 37 (K = 2, SEG = 32).
@pytest.mark.parametrize("n", [3001, 8229])
@pytest.mark.parametrize("c", range(7, 17))
def test_single_msm_one_level_sort(ctx, ol, pr, monkeypatch, c, n):
    monkeypatch.setenv("SBN_MSM_C", str(c))
    W = wm.make_shape(c).W
    sc = mixed_scalars(wm.seam_scalars(c), n, 1000 * c + n)
    pts, dl = tiled_bases(ol, n, 2048)
    with profiled(ctx) as ran:
        out, inf = ctx.msm(sc, pts)
        ran = ran()
    job = ctx.prof_last_job()
    assert (job["c"], job["W"], job["slots"], job["buckets"]) == (c, W, W * n, W << (c - 1))
    assert "k_hist_lds" in ran and "k_scatter_lds" in ran and "k_s2_count" not in ran and "k_sort_rows" not in ran, sorted(ran)
    assert out == expect_from_dlogs(ol, pr, sc, dl) and not inf
    assert out == ol.msm_pippenger(sc, pts, 8)


# ---- single MSM, two-level sort ---------------------------------------------------------------------------------------------
# one template instance of k_s2_count / k_s2_scatter per (c, scalars per block); 10277 = 8192 + 2048 + 37 terms: with 8192 scalars per
# block two blocks, the last with 2085; with 2048 six blocks, the last with 37
@pytest.mark.parametrize("spt", [2, 8])
@pytest.mark.parametrize("c", range(13, 23))
def test_single_msm_two_level_sort(ctx_sort2, ol, pr, monkeypatch, c, spt):
    monkeypatch.setenv("SBN_MSM_C", str(c)); monkeypatch.setenv("SBN_SORT2_SPT", str(spt))
    n, W = 10277, wm.make_shape(c).W
    sc = mixed_scalars(wm.seam_scalars(c), n, 2000 * c + spt)
    pts, dl = tiled_bases(ol, n, 4096)
    with profiled(ctx_sort2) as ran:
        out, inf = ctx_sort2.msm(sc, pts)
        ran = ran()
    job = ctx_sort2.prof_last_job()
    assert (job["c"], job["W"], job["slots"], job["buckets"]) == (c, W, W * n, W << (c - 1))
    assert "k_s2_count" in ran and "k_s2_scatter" in ran and "k_s2_place" in ran and "k_hist_lds" not in ran, sorted(ran)
    assert out == expect_from_dlogs(ol, pr, sc, dl) and not inf
    assert out == ol.msm_pippenger(sc, pts, 8)


# ---- GLV --------------------------------------------------------------------------------------------------------------------
def glv_seam_scalars(c):
    """full scalars k = k1 + lambda k2 whose halves, split by the kernel's decomposition (the model of tests/test_glv_cpu.py), are seam
    values of the 127-bit recoding of width c -> (scalars, seam values landed on by the first halves, by the second halves)"""
    seams = wm.seam_scalars(c, 127)
    ks, got1, got2 = [], set(), set()
    for i, s in enumerate(seams):
        for t in (seams[(i + 1) % len(seams)], seams[(3 * i + 7) % len(seams)], 0, 1):
            for k1, k2 in ((s, t), (t, s)):
                k = (k1 + LAM * k2) % wm.R
                if split(k) == (k1, k2):
                    ks.append(k); got1.add(k1); got2.add(k2)
    return sorted(set(ks)), got1, got2


@pytest.mark.parametrize("n", [1024, 3001])
@pytest.mark.parametrize("c", range(13, 18))
def test_glv_single_msm(glv_pair, ol, pr, monkeypatch, c, n):
    on, off = glv_pair
    monkeypatch.setenv("SBN_MSM_C", str(c))                  # glv_shape honours it for 13 .. 17; the plain context takes it as well
    ks, got1, got2 = glv_seam_scalars(c)
    # Every seam value of the halves is landed on, by a first and by a second half, but the two largest: the model's bound 0x6f4e 2^112
    # lies above what the decomposition can give (k1 < A + 2 B, k2 < C, both 0x6f4d8248... 2^96), so bound - 1 and bound - 2 are no
    # halves of any scalar.  The largest top digit of a half comes from r - 1 and the uniform scalars instead.
    bound = wm.bound_of(127)
    want_seams = set(wm.seam_scalars(c, 127)) - {bound - 1, bound - 2}
    assert want_seams <= got1 and want_seams <= got2
    half = 1 << (c - 1); W = wm.make_shape(c, 127).W
    ind = [wm.recode_independent(h, c, W) for k in ks for h in split(k)]
    seq = [wm.recode_sequential(h, c, W)[0] for k in ks for h in split(k)]
    assert all(any(d[w] == half for d in ind) and any(d[w] == -half for d in seq) for w in range(1, W - 1))
    sc = mixed_scalars(ks + [0, 1, wm.R - 1, wm.R - 2], n, 3000 * c + n)
    pts, dl = tiled_bases(ol, n, 512)
    b = on.bases_upload(pts)
    try:
        with profiled(on) as ran:
            got = on.msm_bases(b, sc)
            ran = ran()
        job = on.prof_last_job()
        assert (job["c"], job["W"], job["slots"], job["buckets"]) == (c, W, 2 * n * W, W << (c - 1))
        assert "k_glv_split" in ran and "k_s2_count" in ran and "k_hist_lds" not in ran, sorted(ran)
        plain = off.msm_bases(b, sc)
        pj = off.prof_last_job()
        assert (pj["c"], pj["W"], pj["slots"]) == (c, wm.make_shape(c).W, n * wm.make_shape(c).W)
        assert got == plain == (expect_from_dlogs(ol, pr, sc, dl), False)
    finally:
        b.free()


# ---- row commits ------------------------------------------------------------------------------------------------------------
def generator_sets(ol, D):
    """two generator sets over the pool, each with h: D distinct points; and D distinct points followed by E columns that repeat the
    first E of them (more than 10 % repeats: the handle merges equal bases).  Columns E .. D - 1 are unique in both."""
    pts, _ = pool(ol)
    E = (D + 1) // 8 + 2
    G = pts[:64 * D]; h = pts[64 * D:64 * D + 64]
    return {"distinct": (G, h, D), "dups": (G + pts[:64 * E], h, D + E)}, E


def row_matrix(seams, R, E, seed):
    """three rows: all zero; one scalar repeated; the seam scalars in columns E .. (bases that no other column repeats, so that merging
    equal bases leaves them as they are), uniform scalars around them"""
    assert E + len(seams) <= R
    row = bytearray(rand_scalars(R, seed))
    row[32 * E:32 * (E + len(seams))] = to_bytes(seams)
    const = seams[len(seams) // 2] or 1
    return bytes(32 * R) + const.to_bytes(32, "little") * R + bytes(row), 3


FUSED_MAX_ENTRIES = 8 << 15          # k_sort_rows: estride <= 8 SORT_SL; its LDS (5/4 2^(c-1) + 34882 words) fits 160 KiB up to c = 13


def bucket_row_shapes():
    out = []
    for c in range(7, 17):
        n_seam = len(wm.seam_scalars(c))
        # the smallest row that holds the seam set beside the repeated columns
        out.append(pytest.param(c, n_seam + n_seam // 7 + 8, "k_sort_rows" if c <= 13 else "k_hist_lds", id="c%d-small" % c))
        # c <= 13: the smallest row whose W entries per column no longer fit the fused sort.  c >= 14: the fused sort's LDS alone exceeds
        # 160 KiB, every shape takes the generic sort: the small shape is the only side of the rule there.
        if c <= 13:
            out.append(pytest.param(c, FUSED_MAX_ENTRIES // wm.make_shape(c).W + 1, "k_hist_lds", id="c%d-past-fused" % c))
    return out


@pytest.mark.parametrize("c,D,sort_kernel", bucket_row_shapes())
def test_commit_rows_bucket_method(ctx, ol, monkeypatch, c, D, sort_kernel):
    """rows over ONE shared bucket set (entry = w * npts + column), D columns of distinct points (+ repeated ones, + h)"""
    monkeypatch.setenv("SBN_MSM_C", str(c))                  # choose_shape reads it for row commits too
    W, seams = wm.make_shape(c).W, wm.seam_scalars(c)
    sets, E = generator_sets(ol, D)
    for name, (G, h, R) in sets.items():
        Z, L = row_matrix(seams, R, E, 4000 * c + R)
        merged = wm.lookup_points(G, h) != R + 1
        assert merged == (name == "dups")
        b = ctx.bases_upload(G, h)
        try:
            for bl in (to_bytes([seams[-1], seams[len(seams) // 3], 0]), None):
                with profiled(ctx) as ran:
                    out, infs = ctx.commit_rows(b, Z, bl, L, R)
                    ran = ran()
                job = ctx.prof_last_job()
                cols = D + 2 if merged else R + (1 if bl else 0)          # merged: the unique points, h among them, and their sum
                assert (job["c"], job["W"], job["slots"], job["buckets"]) == (c, W, L * cols * W, L << (c - 1)), (name, bl is not None)
                assert (cols * W <= FUSED_MAX_ENTRIES) == (sort_kernel == "k_sort_rows") or c > 13
                assert sort_kernel in ran and ("k_sort_rows" in ran) != ("k_hist_lds" in ran) and "k_comb_rows" not in ran, sorted(ran)
                assert ("k_merge_scalars" in ran) == merged
                assert out == ol.commit_rows(Z, bl, L, R, G, h, 16), (name, bl is not None)
                assert infs[0] == (0 if bl else 1)
        finally:
            b.free()


def lookup_sets(ol):
    """3 to 6 tabulated points.  distinct: three points and h.  dups: eight columns over three points and one at infinity, and h; the
    handle merges them and tabulates the 5 unique points and the sum of the columns (6 points: 377 MB at c = 17)."""
    pts, _ = pool(ol)
    P = [pts[64 * i:64 * i + 64] for i in range(5)]
    inf = bytes(64)
    return {"distinct": (P[0] + P[1] + P[2], P[3], 3, 4, [0, 1, 2]),
            "dups": (P[0] + P[1] + P[0] + P[2] + P[1] + P[0] + inf + P[2], P[4], 8, 6, [0, 1, 3, 6])}      # first column of every group


@pytest.mark.parametrize("name", ["distinct", "dups"])
@pytest.mark.parametrize("c", range(wm.COMB_C_MIN, wm.COMB_C_MAX + 1))
def test_commit_rows_lookup_table(ctx, ol, sbn, monkeypatch, c, name):
    """T[w][j][d - 1] = d 2^(c w) G_j, d = 1 .. 2^(c-1), index ((w npts + j) << (c-1)) + d - 1: the width is what the budget buys.
    k_comb_rows (one block per row, sequential recoding), k_comb_rows_flat (SBN_COMB_S blocks per row, independent recoding: the corner
    digit +2^(c-1) reads the LAST entry of a column) and k_comb_rows_const (constant and zero rows of a merged set, independent recoding).
    k_comb_rows and k_comb_rows_flat share the profile label k_comb_rows; which of them ran follows from S: flat iff S > 1.
    With at most 6 columns only the first of the S blocks of a row has entries at the wide widths (ncol W <= 256); rows wide enough
    to spread over the blocks are in test_gpu_msm.py's lookup tests, at whatever width their budget gives."""
    monkeypatch.delenv("SBN_MSM_C", raising=False); monkeypatch.delenv("SBN_COMB_S", raising=False)
    G, h, R, npts, own = lookup_sets(ol)[name]
    assert wm.lookup_points(G, h) == npts
    W, seams = wm.make_shape(c).W, wm.seam_scalars(c)
    # seam rows: the seam scalars in the columns `own` (one column per distinct base: merging leaves them alone), zero elsewhere
    rows = []
    for i in range(0, len(seams), len(own)):
        r = [0] * R
        for col, v in zip(own, seams[i:i + len(own)]):
            r[col] = v
        rows.append(to_bytes(r))
    n_seam_rows = len(rows)
    rows.append(bytes(32 * R))                                                               # zero row
    const0 = len(rows)
    rows += [v.to_bytes(32, "little") * R for v in seams if v]                               # every seam scalar as a constant row
    uni = rand_scalars(32 * R, 5000 + c)
    rows += [uni[32 * R * i:32 * R * (i + 1)] for i in range(32)]                            # ordinary rows (merging sums their columns)
    L = len(rows); Z = b"".join(rows)
    assert L >= 32                                                                           # many rows: S = 1 by the host's own rule
    blinds = to_bytes([seams[(5 * i + 3) % len(seams)] for i in range(L)])
    b = ctx.bases_upload(G, h)
    try:
        need = wm.lookup_need(npts, c)
        if c > wm.COMB_C_MIN:
            assert ctx.bases_precompute(b, need - 1) == c - 1                                # one byte short buys the next narrower table
        else:
            with pytest.raises(sbn.SbnError):
                ctx.bases_precompute(b, need - 1)                                            # ... and below c = 7 there is none
        assert ctx.bases_precompute(b, need) == c
        cols = npts if name == "dups" else R
        for bl in (blinds, None):
            want = ol.commit_rows(Z, bl, L, R, G, h, 16)
            ncol = cols if name == "dups" else cols + (1 if bl else 0)
            with profiled(ctx) as ran:
                out, infs = ctx.commit_rows(b, Z, bl, L, R)                                  # S = 1: k_comb_rows (+ k_comb_rows_const)
                ran = ran()
            job = ctx.prof_last_job()
            assert (job["c"], job["W"], job["slots"], job["buckets"]) == (c, W, L * ncol * W, 0), (bl is not None)
            assert "k_comb_rows" in ran and ("k_comb_rows_const" in ran) == (name == "dups") and "k_acc_first" not in ran, sorted(ran)
            assert out == want, (bl is not None)
            assert infs[n_seam_rows] == (0 if bl else 1)
            for S in (2, 3):
                monkeypatch.setenv("SBN_COMB_S", str(S))
                with profiled(ctx) as ran:
                    out, _ = ctx.commit_rows(b, Z, bl, L, R)                                 # every row through k_comb_rows_flat
                    ran = ran()
                job = ctx.prof_last_job()
                assert (job["c"], job["W"], job["buckets"]) == (c, W, 0)
                assert "k_comb_rows" in ran and "k_comb_rows_const" not in ran, sorted(ran)
                assert out == want, (S, bl is not None)
                for pick in ([0], [n_seam_rows - 1], [1, const0 + c], [n_seam_rows, const0 + 1]):      # 1 and 2 rows: seam, zero, constant
                    Zs = b"".join(rows[i] for i in pick)
                    bs = b"".join(bl[32 * i:32 * i + 32] for i in pick) if bl else None
                    got, _ = ctx.commit_rows(b, Zs, bs, len(pick), R)
                    assert got == b"".join(want[64 * i:64 * i + 64] for i in pick), (S, pick, bl is not None)
                    assert ctx.prof_last_job()["c"] == c
                monkeypatch.delenv("SBN_COMB_S")
    finally:
        b.free()
