"""GPU: KZG commitments and openings over a resident SRS (sbn_kzg_*, sbn_poly_div_linear) against the pure-int model of kzg.rs
(kzg_model.py) and the C oracle's MSM; at full size the verifier's relation (tau - z) pi + y G == C is checked without a pairing."""
import random

import numpy as np
import pytest

from conftest import rand_scalars
import kzg_model as km

pytestmark = pytest.mark.gpu
R = km.R
G = (1).to_bytes(32, "little") + (2).to_bytes(32, "little")
ZERO_PT = bytes(64)
EINVAL = "rc=-1"


def _pow2(n):
    return 1 << max(0, (n - 1).bit_length())


def _upload_poly(ctx, vals, junk_seed=1):
    """vals in a table of the next power of two, the entries past len(vals) filled with non-zero junk"""
    n = len(vals); L = _pow2(max(n, 1))
    junk = km.from_bytes(rand_scalars(L - n, junk_seed)) if L > n else []
    return ctx.table_upload(km.to_bytes(list(vals) + [j or 1 for j in junk]))


def _rand(n, seed):
    return km.from_bytes(rand_scalars(n, seed)) if n else []


def _check_div(ctx, t, vals, z):
    n = len(vals)
    ev, q = ctx.poly_div_linear(t, n, km.to_bytes([z]))
    y = km.evaluate_poly(vals, z)
    assert km.from_bytes(ev) == [y], f"eval n={n} z={z}"
    want = km.compute_quotient(vals, z, y)
    if n <= 1:
        assert q is None
        return
    try:
        assert len(q) == _pow2(n - 1)
        assert ctx.table_download(q) == km.to_bytes(want + [0] * (len(q) - len(want))), f"quotient n={n} z={z}"
    finally:
        q.free()


def _points(seed):
    return [0, 1, R - 1, random.Random(seed).randrange(R)]


# lengths on both sides of the tile (1024) and carry-level (2^20) boundaries
DIV_LENS = [0, 1, 2, 3, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2047, 2049, 1 << 16, (1 << 16) + 3]


@pytest.mark.parametrize("n", DIV_LENS)
def test_poly_div_linear_vs_model(ctx, n):
    vals = _rand(n, 100 + n)
    t = _upload_poly(ctx, vals, 7 + n)
    try:
        for z in _points(n):
            _check_div(ctx, t, vals, z)
    finally:
        t.free()


@pytest.mark.parametrize("n", [(1 << 20) - 1, 1 << 20, (1 << 20) + 1025])
def test_poly_div_linear_level_edges(ctx, n):
    vals = _rand(n, 3)
    t = _upload_poly(ctx, vals, 4)
    try:
        _check_div(ctx, t, vals, random.Random(n).randrange(R))
    finally:
        t.free()


@pytest.mark.parametrize("n", [1, 2, 257, 1025, 5000])
def test_poly_div_linear_all_r_minus_1(ctx, n):
    vals = [R - 1] * n
    t = _upload_poly(ctx, vals)
    try:
        for z in _points(n):
            _check_div(ctx, t, vals, z)
    finally:
        t.free()


def test_poly_div_linear_lazy_tables(ctx, sbn):
    """tables straight from sbn_gather_merge and sbn_table_bound (values in the lazy ranges those kernels leave)"""
    mem = [ctx.table_upload(rand_scalars(256, s)) for s in (11, 12)]
    n = 3000
    rng = np.random.default_rng(5)
    addrs = [rng.integers(0, 256, size=n, dtype=np.uint32) for _ in range(2)]
    ptrs = []
    try:
        for a in addrs:
            p = ctx.dev_alloc(a.nbytes); ctx.dev_upload(p, a); ptrs.append(p)
        gm = ctx.gather_merge(mem, ptrs, n)
        Z = ctx.table_upload(rand_scalars(64 * 512, 13)); Lv = ctx.table_upload(rand_scalars(64, 14))
        bd = ctx.table_bound(Z, Lv)
        for t, m in ((gm, 2 * n), (gm, 2 * n - 5), (bd, 512), (bd, 300)):
            vals = km.from_bytes(ctx.table_download(t))[:m]
            for z in _points(m):
                _check_div(ctx, t, vals, z)
        for t in (gm, Z, Lv, bd):
            t.free()
    finally:
        for p in ptrs:
            ctx.dev_free(p)
        for t in mem:
            t.free()


def test_poly_div_linear_rejects(ctx, sbn):
    t = ctx.table_upload(rand_scalars(8, 1))
    try:
        with pytest.raises(sbn.SbnError, match=EINVAL):
            ctx.poly_div_linear(t, 9, km.to_bytes([3]))
        with pytest.raises(sbn.SbnError, match=EINVAL):
            ctx.poly_div_linear(t, 4, km.to_bytes([R]))
    finally:
        t.free()


def _powers(tau, n):
    out, x = [], 1
    for _ in range(n):
        out.append(x); x = x * tau % R
    return out


@pytest.mark.parametrize("n", [1, 2, 1000, 4097])
def test_srs_from_tau_vs_oracle(ctx, ol, n):
    tau = random.Random(n).randrange(1, R)
    srs = ctx.kzg_srs_from_tau(km.to_bytes([tau]), n)
    try:
        assert len(srs) == n
        assert ctx.bases_download(srs, 0, n) == ol.g1_mul_gen_batch(km.to_bytes(_powers(tau, n)), 8)
    finally:
        srs.free()


def test_srs_from_tau_rejects(ctx, sbn):
    for tau in (0, R, R + 5):
        with pytest.raises(sbn.SbnError, match=EINVAL):
            ctx.kzg_srs_from_tau(km.to_bytes([tau]) if tau < 2**256 else None, 4)


def test_srs_upload_matches_from_tau(ctx):
    tau = 123456789
    srs = ctx.kzg_srs_from_tau(km.to_bytes([tau]), 300)
    pts = ctx.bases_download(srs, 0, 300)
    up = ctx.kzg_srs_upload(pts)
    try:
        assert ctx.bases_download(up, 0, 300) == pts
        t = ctx.table_upload(rand_scalars(512, 3))
        assert ctx.kzg_commit(up, t, 300) == ctx.kzg_commit(srs, t, 300)
        t.free()
    finally:
        srs.free(); up.free()


@pytest.fixture(scope="module")
def srs8k(ctx):
    tau = 0x1234567890abcdef1234567890abcdef
    s = ctx.kzg_srs_from_tau(km.to_bytes([tau]), 8200)
    yield s, ctx.bases_download(s, 0, 8200)
    s.free()


@pytest.mark.parametrize("n", [1, 2, 3, 1000, 8193])
def test_commit_open_vs_oracle(ctx, ol, srs8k, n):
    srs, pts = srs8k
    vals = _rand(n, 50 + n)
    t = _upload_poly(ctx, vals, 9)
    try:
        C, inf = ctx.kzg_commit(srs, t, n)
        assert C == ol.msm_pippenger(km.to_bytes(vals), pts[:64 * n], 8) and not inf
        z = random.Random(n).randrange(R)
        ev, pi, pinf = ctx.kzg_open(srs, t, n, km.to_bytes([z]))
        y = km.evaluate_poly(vals, z)
        assert km.from_bytes(ev) == [y]
        q = km.compute_quotient(vals, z, y)
        if n <= 1:
            assert pi == ZERO_PT and pinf
        else:
            assert pi == ol.msm_pippenger(km.to_bytes(q), pts[:64 * (n - 1)], 8)
    finally:
        t.free()


def test_commit_truncates_and_open_rejects(ctx, ol, sbn):
    tau = 77
    srs = ctx.kzg_srs_from_tau(km.to_bytes([tau]), 100)
    pts = ctx.bases_download(srs, 0, 100)
    vals = _rand(200, 8)
    t = _upload_poly(ctx, vals)
    try:
        assert ctx.kzg_commit(srs, t, 200)[0] == ol.msm_pippenger(km.to_bytes(vals[:100]), pts, 8)
        assert ctx.kzg_commit(srs, t, 0) == (ZERO_PT, True)
        ev, pi, pinf = ctx.kzg_open(srs, t, 101, km.to_bytes([5]))          # 100 quotient coefficients: fits exactly
        assert km.from_bytes(ev) == [km.evaluate_poly(vals[:101], 5)] and not pinf
        with pytest.raises(sbn.SbnError, match=EINVAL):
            ctx.kzg_open(srs, t, 102, km.to_bytes([5]))
        with pytest.raises(sbn.SbnError, match=EINVAL):
            ctx.kzg_open(srs, t, 10, km.to_bytes([R]))
        with pytest.raises(sbn.SbnError, match=EINVAL):
            ctx.kzg_commit(srs, t, 257)
        for n in (0, 1):
            ev, pi, pinf = ctx.kzg_open(srs, t, n, km.to_bytes([9]))
            assert km.from_bytes(ev) == [vals[0] if n else 0] and pi == ZERO_PT and pinf
    finally:
        t.free(); srs.free()


@pytest.mark.parametrize("lens", [[700], [5, 1000, 64], [1, 0, 2, 3000, 257, 1025, 40]])
def test_open_batched_vs_model(ctx, ol, srs8k, lens):
    srs, pts = srs8k
    rng = random.Random(len(lens) * 31 + lens[0])
    polys = [_rand(n, 200 + i) for i, n in enumerate(lens)]
    tabs = [_upload_poly(ctx, p, 300 + i) for i, p in enumerate(polys)]
    try:
        for gamma in (rng.randrange(R), 0):
            z = rng.randrange(R)
            evals, pi, pinf = ctx.kzg_open_batched(srs, tabs, lens, km.to_bytes([z]), km.to_bytes([gamma]))
            want_evals, _, q = km.batch_prove(polys, z, gamma)
            assert [km.from_bytes(e)[0] for e in evals] == want_evals
            if q:
                assert pi == ol.msm_pippenger(km.to_bytes(q), pts[:64 * len(q)], 8)
                assert pinf == (pi == ZERO_PT)                                  # gamma = 0 with p_0 shorter than max(ns): an all-zero quotient
            else:
                assert pi == ZERO_PT and pinf
    finally:
        for t in tabs:
            t.free()


def test_open_batched_edges(ctx, sbn, srs8k):
    srs, _ = srs8k
    evals, pi, pinf = ctx.kzg_open_batched(srs, [], [], km.to_bytes([3]), km.to_bytes([4]))
    assert evals == [] and pi == ZERO_PT and pinf
    t = ctx.table_upload(rand_scalars(16, 2))
    try:
        with pytest.raises(sbn.SbnError, match=EINVAL):
            ctx.kzg_open_batched(srs, [t], [17], km.to_bytes([3]), km.to_bytes([4]))
        with pytest.raises(sbn.SbnError, match=EINVAL):
            ctx.kzg_open_batched(srs, [t], [16], km.to_bytes([3]), km.to_bytes([R]))
    finally:
        t.free()


def test_gather_merge_commit_open_matches_upload(ctx, srs8k):
    """the derefs shape: sbn_gather_merge output committed and opened gives the bytes of its host-uploaded copy"""
    srs, _ = srs8k
    mem = [ctx.table_upload(rand_scalars(128, s)) for s in (21, 22, 23)]
    n = 1500
    rng = np.random.default_rng(9)
    ptrs = []
    try:
        for _ in range(3):
            a = rng.integers(0, 128, size=n, dtype=np.uint32); p = ctx.dev_alloc(a.nbytes); ctx.dev_upload(p, a); ptrs.append(p)
        gm = ctx.gather_merge(mem, ptrs, n)
        up = ctx.table_upload(ctx.table_download(gm))
        z = km.to_bytes([987654321])
        for m in (3 * n, len(gm)):
            assert ctx.kzg_commit(srs, gm, m) == ctx.kzg_commit(srs, up, m)
            assert ctx.kzg_open(srs, gm, m, z) == ctx.kzg_open(srs, up, m, z)
        gm.free(); up.free()
    finally:
        for p in ptrs:
            ctx.dev_free(p)
        for t in mem:
            t.free()


def test_commit_equals_p_tau_times_g_2_20(ctx, ol):
    n = 1 << 20
    tau = random.Random(20).randrange(1, R)
    srs = ctx.kzg_srs_from_tau(km.to_bytes([tau]), n)
    raw = rand_scalars(n, 2020)
    t = ctx.table_upload(raw)
    try:
        C, _ = ctx.kzg_commit(srs, t, n)
        assert C == ol.g1_mul(G, km.to_bytes([km.evaluate_poly(km.from_bytes(raw), tau)]))
    finally:
        t.free(); srs.free()


def _verifier_relation(ol, tau, z, y, pi, C):
    lhs = ol.g1_add(ol.g1_mul(pi, km.to_bytes([(tau - z) % R])), ol.g1_mul(G, km.to_bytes([y])))
    return lhs == C


def _synthetic_table(ctx, n, first, keep):
    p = ctx.dev_alloc(32 * n); keep.append(p)
    ctx.scalars_synthetic(0x5BA27A2B4E254, first, n, p)
    return ctx.table_from_dev(p, n)


def test_full_size_open_identity(ctx, ol):
    """an SRS of 2^25 + 1 from tau; a 2^25 table: (tau - z) pi + y G == C, and the same for a batched open of 4 x 2^22"""
    n = 1 << 25
    rng = random.Random(25)
    tau, z = rng.randrange(1, R), rng.randrange(R)
    srs = ctx.kzg_srs_from_tau(km.to_bytes([tau]), n + 1)
    keep, tabs = [], []
    try:
        t = _synthetic_table(ctx, n, 0, keep); tabs.append(t)
        C, _ = ctx.kzg_commit(srs, t, n)
        ev, pi, _ = ctx.kzg_open(srs, t, n, km.to_bytes([z]))
        assert _verifier_relation(ol, tau, z, km.from_bytes(ev)[0], pi, C)
        t.free(); tabs.clear()
        for p in keep:
            ctx.dev_free(p)
        keep.clear()
        m, K = 1 << 22, 4
        gamma = rng.randrange(R)
        tabs = [_synthetic_table(ctx, m, k * m, keep) for k in range(K)]
        ns = [m, m - 1, m - 1000, 5]
        evals, pi, _ = ctx.kzg_open_batched(srs, tabs, ns, km.to_bytes([z]), km.to_bytes([gamma]))
        Cs = [ctx.kzg_commit(srs, tk, nk)[0] for tk, nk in zip(tabs, ns)]
        Ccomb, y, gp = None, 0, 1
        for Ck, e in zip(Cs, evals):
            term = ol.g1_mul(Ck, km.to_bytes([gp]))
            Ccomb = term if Ccomb is None else ol.g1_add(Ccomb, term)
            y = (y + km.from_bytes(e)[0] * gp) % R
            gp = gp * gamma % R
        assert _verifier_relation(ol, tau, z, y, pi, Ccomb)
    finally:
        for t in tabs:
            t.free()
        for p in keep:
            ctx.dev_free(p)
        srs.free()
