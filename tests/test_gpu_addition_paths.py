"""GPU: every branch of the point additions (g1.cuh: xyzz_madd, xyzz_add_inl, xyzz_add_quad, xyzz_dbl) inside the kernels that inline
them, at the smallest sizes that reach them, bit for bit against the oracle.

The common path of an addition is one straight block of products; the rare paths — the accumulator or the incoming point at
infinity, equal points (doubling), opposite points (cancellation back to infinity) — sit behind branches around it, and the
products behind the same-x test are the ones fp.cuh's fe_pin32 re-widens.  Each case builds its buckets entry by entry:

  * a CHAIN is the list of entries of one bucket: bases d * G with d known (0 = the point at infinity, r - d = the opposite point),
    all given the same digit in window 0 of a c = 7 MSM; an entry with sign -1 takes the digit's negative instead (scalar 128 - b:
    the kernel's sign bit, xyzz_madd's `neg`), which leaves a +1 in window 1;
  * the uniform scalars around them are kept out of the chains' buckets (their window-0 digit is 41 .. 63, the chains use 1 .. 36).

The order inside a bucket is decided by the sort's LDS atomics (msm_kernels.cuh); the entries of a chain are laid out in a row inside
one 64-aligned group of scalar indices, which one wave scatters with one instruction, and come out in that order in practice.  The
assertions do not depend on it: every result is compared with the discrete-log identity and with the oracle's Pippenger.
"""
import random

import pytest

import window_model as wm
from conftest import rand_scalars
from test_gpu_window_widths import _context_with, profiled, to_bytes

pytestmark = pytest.mark.gpu

R = wm.R
C7 = 7
FILL_LO, FILL_HI = 41, 63          # window-0 digits of the uniform scalars (c = 7): buckets the chains never use


def dlogs(seed, k):
    raw = rand_scalars(k, seed)
    return [int.from_bytes(raw[32 * i:32 * i + 32], "little") or 1 for i in range(k)]


def chains(seed):
    """the bucket contents, each a list of (d, sign); lengths 1 .. 8.  Names say what the accumulator meets, in laid-out order."""
    p, q, s, t, u, v, w, x = dlogs(seed, 8)
    n = lambda d: (R - d) % R
    E = lambda *ds: [(d % R, 1) for d in ds]
    out = {
        "dbl_second_and_last": E(p, p),
        "dbl_second_of_three": E(p, p, q),
        "dbl_last_of_three": E(p, q, p + q),
        "dbl_middle_of_five": E(p, q, p + q, s, t),
        "cancel_base_last": E(p, n(p)),
        "cancel_sign_last": [(p, 1), (p, -1)],
        "cancel_then_point": E(p, n(p), q),
        "cancel_then_dbl": E(p, n(p), q, q, s),
        "cancel_a_sum_then_point": E(p, q, n(p + q), s),
        "cancel_a_sum_by_sign": [(p, 1), (q, 1), ((p + q) % R, -1)],
        "inf_first": E(0, p, q),
        "inf_middle": E(p, 0, q),
        "inf_last": E(p, q, 0),
        "inf_only": E(0),
        "inf_twice_then_point": E(0, 0, p),
        "inf_negated_first": [(0, -1), (p, 1)],
        # two lanes per bucket split a bucket of up to SEG = 8 entries in halves: these put an event in each half, and as one lane's
        # chain they put doubling and cancellation at entries 6 .. 8
        "halves_dbl_dbl": E(p, p, q, s) + E(t, u, t + u, v),
        "halves_cancel_inf": E(p, n(p), q, q) + E(0, s, s, 0),
        "halves_equal_sums": E(p, q, s) + E(s, p, q),                 # the two lanes' partial sums are equal: k_reduce_l1's bucket_load doubles
        "halves_opposite_sums": E(p, q, s) + E(n(s), n(p), n(q)),     # ... and here they cancel
        "halves_inf_and_sum": E(0, 0) + E(w, x),
    }
    assert all(1 <= len(c) <= 8 for c in out.values()) and len(out) <= 36
    return out


def fill_scalars(k, seed, c=C7, lo=FILL_LO, hi=FILL_HI):
    rnd = random.Random(seed)
    return [((rnd.randrange(R) >> c) << c | rnd.randrange(lo, hi + 1)) % R for _ in range(k)]


def lay_out(groups, n, seed):
    """groups: [(digit b, [(d, sign)])] -> n scalars and base dlogs: every group in a row inside one 64-aligned index group, uniform
    scalars over random bases everywhere else"""
    fill = iter(fill_scalars(n, seed))
    fd = dlogs(seed + 1, 64)
    sc, dl = [], []
    for b, chain in groups:
        for lo in range(0, len(chain), 64):
            part = chain[lo:lo + 64]
            while len(sc) % 64 + len(part) > 64:
                sc.append(next(fill)); dl.append(fd[len(sc) % 64])
            for d, sign in part:
                sc.append(b if sign > 0 else (1 << C7) - b); dl.append(d)
    assert len(sc) <= n, (len(sc), n)
    while len(sc) < n:
        sc.append(next(fill)); dl.append(fd[len(sc) % 64])
    return sc, dl


_pts = {}


def points_of(ol, dl):
    """d * G for every d (computed once per distinct d), the point at infinity for d = 0"""
    need = sorted({d for d in dl if d and d not in _pts})
    if need:
        got = ol.g1_mul_gen_batch(to_bytes(need), 16)
        _pts.update({d: got[64 * i:64 * i + 64] for i, d in enumerate(need)})
    return b"".join(_pts[d] if d else bytes(64) for d in dl)


def expect(ol, pr, sc, dl):
    return ol.g1_mul(pr.point_to_xy(pr.G), (sum(k * d for k, d in zip(sc, dl)) % R).to_bytes(32, "little"))


def run_msm(cx, ol, pr, sc, dl, c):
    blob, pts = to_bytes(sc), points_of(ol, dl)
    with profiled(cx) as ran:
        out, inf = cx.msm(blob, pts)
        ran = ran()
    assert cx.prof_last_job()["c"] == c
    want = expect(ol, pr, sc, dl)
    assert out == want and inf == (want == bytes(64))
    if len(sc) <= 10000:
        assert out == ol.msm_pippenger(blob, pts, 8)
    return cx.prof_last_acc(), ran


def set_env(monkeypatch, **env):
    for k in ("SBN_MSM_C", "SBN_MSM_SEG", "SBN_RED_L"):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, str(v))


# ---- the mixed addition in k_acc_first<1> and <2> ------------------------------------------------------------------------------
@pytest.mark.parametrize("n,LPB", [(3007, 1), (3008, 2)])
def test_chains_in_acc_first(ctx, ol, pr, monkeypatch, n, LPB):
    """no override: c = 7, segments of 8; 3008 terms is the first size that splits a bucket over two lanes.  One bucket per chain
    (digits 1 .. 21 of window 0); neighbouring buckets hold sums of the same few points, so the reduction's full additions meet
    equal and opposite operands as well."""
    set_env(monkeypatch)
    groups = [(b + 1, ch) for b, ch in enumerate(chains(7 + LPB).values())]
    sc, dl = lay_out(groups, n, 100 + LPB)
    acc, ran = run_msm(ctx, ol, pr, sc, dl, C7)
    assert (acc["SEG"], acc["LPB"]) == (8, LPB) and "k_acc_first" in ran and "k_reduce_l1" in ran, (acc, sorted(ran))


# ---- k_acc_extra and both branches of k_acc_merge ------------------------------------------------------------------------------
def test_chains_in_acc_extra_and_merge(ctx, ol, pr, monkeypatch):
    """2100 terms, c = 7, SBN_MSM_SEG = 8: every bucket the uniform scalars fill is cut into segments (k_acc_extra) and merged by one
    lane (up to 12 extra segments).  Built on top: bucket 30 with 5 segments — two with the same entries (the lane merge doubles),
    the chains, a segment that cancels everything so far, one more; bucket 32 with 14 segments, merged by a wave: lane 0 adds two
    segments of equal sum (xyzz_add_inl doubles), lane 1 holds a segment of that same sum (the quad addition doubles), lanes 2 and 3
    hold opposite segments (the quad addition cancels), the other lanes the chains."""
    set_env(monkeypatch, SBN_MSM_SEG=8)
    ch = chains(21)
    d = dlogs(22, 64)
    neg = lambda seg: [((R - x) % R, s) for x, s in seg]
    total = lambda seg: sum(x * s for x, s in seg) % R
    plain = lambda xs: [(x, 1) for x in xs]

    def with_sum(want, xs):                     # 8 entries: seven given points and the one that brings the sum to `want`
        return plain(xs[:7]) + [((want - sum(xs[:7])) % R, 1)]
    S = plain(d[:8])
    eight = [ch["halves_dbl_dbl"], ch["halves_cancel_inf"], ch["dbl_middle_of_five"] + ch["inf_last"], ch["cancel_then_dbl"] + ch["inf_first"],
             ch["cancel_a_sum_then_point"] + ch["cancel_a_sum_then_point"], ch["dbl_last_of_three"] + ch["cancel_then_dbl"]]
    assert all(len(e) == 8 for e in eight)
    lane_bucket = S + list(reversed(S)) + eight[0]
    lane_bucket += with_sum((R - total(lane_bucket)) % R, d[8:16]) + eight[1]
    T = plain(d[16:24])
    wave_bucket = S + list(reversed(S)) + with_sum(2 * total(S) % R, d[24:32]) + T + neg(T)
    wave_bucket += eight[2] + eight[3] + eight[4] + eight[5] + plain(d[32:40]) + plain(d[40:48]) + with_sum(0, d[48:56]) + plain(d[56:64]) + S
    assert len(lane_bucket) == 5 * 8 and len(wave_bucket) == 14 * 8
    sc, dl = lay_out([(30, lane_bucket), (32, wave_bucket)], 2100, 23)
    acc, ran = run_msm(ctx, ol, pr, sc, dl, C7)
    assert (acc["SEG"], acc["LPB"]) == (8, 1), acc
    assert acc["extra_count"] > 4 + 13 and acc["big_count"] > 2 and "k_acc_extra" in ran and "k_acc_merge" in ran, (acc, sorted(ran))


# ---- the full addition through the reduction -------------------------------------------------------------------------------------
@pytest.fixture(scope="module", params=[1, 64], ids=["L1-three-levels", "L64-quad"])
def red_ctx(request, sbn):
    """a fresh context per shape, two-level sort from 1024 terms on (what c = 20 needs)"""
    c = _context_with(sbn, SBN_SORT2_MIN=1024, SBN_RED_L=request.param)
    yield c, request.param
    c.close()


def test_equal_and_opposite_bucket_sums_in_the_reduction(red_ctx, ol, pr, monkeypatch):
    """c = 20 (13 windows of 2^19 buckets), 3000 terms.  SBN_RED_L = 1: one bucket per lane, 8192 chunks per window, three launches of
    k_reduce_combine; 64: one lane walks 64 buckets, 128 chunks, two launches of k_reduce_combine_quad.  Window 0 holds single-entry
    buckets in pairs — neighbours with the same point and with opposite points (the lane loop of k_reduce_l1 at L = 64, its suffix scan
    at L = 1), and the same one chunk apart at either chunk size (64 and 4096 buckets: the suffix scans of the combine kernels) —
    below bucket 2^18; the uniform scalars' window-0 digits start at 2^18."""
    cx, L = red_ctx
    c = 20
    set_env(monkeypatch, SBN_MSM_C=c, SBN_RED_L=L)
    d = dlogs(31, 12)
    n_ = lambda x: (R - x) % R
    singles = []
    for i, (gap, base) in enumerate([(1, 10), (64, 64 * 5 + 3), (4096, 4096 * 3 + 7)]):
        a, b2, e, f = d[4 * i:4 * i + 4]
        singles += [(base, a), (base + gap, a), (base + 10 * gap, b2), (base + 11 * gap, n_(b2)),                     # equal, opposite
                    (base + 20 * gap, e), (base + 21 * gap, e), (base + 22 * gap, e), (base + 30 * gap, f), (base + 31 * gap, n_(f)), (base + 32 * gap, f)]
    assert len({b for b, _ in singles}) == len(singles) and max(b for b, _ in singles) < 1 << 18
    n = 3000
    fill = fill_scalars(n - len(singles), 32, c, 1 << 18, (1 << 19) - 1)
    fd = dlogs(33, 64)
    sc = [b for b, _ in singles] + fill
    dl = [x for _, x in singles] + [fd[i % 64] for i in range(len(fill))]
    acc, ran = run_msm(cx, ol, pr, sc, dl, c)
    assert (acc["L"], acc["chunks"], acc["levels"], acc["quad"]) == ((1, 8192, 3, 0) if L == 1 else (64, 128, 2, 1)), acc
    assert ran["k_reduce_l1"][1] == 1 and ran["k_reduce_combine"][1] == acc["levels"], ran


# ---- row commits over duplicated generators: bucket path and lookup table ---------------------------------------------------------
def test_row_commit_over_duplicated_generators(ctx, ol, monkeypatch):
    """8 rows of 300 columns over gens_new(300, "gens_r1cs_eval") — two thirds of these generators are the same point — with a zero row
    and a constant row, first through the buckets, then through the lookup table (k_comb_build, k_comb_rows*, k_comb_fold).  The
    table's budget is 32 MiB: the smallest table of this set (c = 7: 148 KiB per distinct point, over a hundred of them) is over 15 MB,
    so a budget of 1 MiB is refused."""
    set_env(monkeypatch)
    L, Rr = 8, 300
    bases, gxy = ctx.gens_new(Rr, b"gens_r1cs_eval")
    try:
        assert gxy == ol.gens_new(Rr, b"gens_r1cs_eval")[0]
        G = [gxy[64 * i:64 * i + 64] for i in range(Rr)]
        assert len(set(G)) < Rr // 2
        const = (0x1d3 | (0x7f << 72) | (1 << 250)).to_bytes(32, "little")
        Z = bytes(32 * Rr) + const * Rr + rand_scalars((L - 2) * Rr, 41)
        want = ol.commit_rows(Z, None, L, Rr, gxy[:64 * Rr], gxy[64 * Rr:], 8)
        with profiled(ctx) as ran:
            out, infs = ctx.commit_rows(bases, Z, None, L, Rr)
            ran = ran()
        assert "k_acc_first" in ran and "k_comb_rows" not in ran, sorted(ran)
        assert out == want and infs[0] == 1 and not any(infs[1:])
        assert 7 <= ctx.bases_precompute(bases, 32 << 20) <= 17
        with profiled(ctx) as ran:
            out, infs = ctx.commit_rows(bases, Z, None, L, Rr)
            ran = ran()
        assert "k_comb_rows" in ran and "k_comb_fold" in ran and "k_acc_first" not in ran, sorted(ran)
        assert out == want and infs[0] == 1 and not any(infs[1:])
    finally:
        bases.free()
