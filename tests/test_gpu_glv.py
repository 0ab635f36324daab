"""GPU: single MSMs over the GLV endomorphism (glv_kernels.cuh) against the plain path and the discrete-log identity, with the path
switched on and off per context (SBN_MSM_GLV is read when a context is created)."""
import numpy as np
import pytest

from conftest import rand_scalars

pytestmark = pytest.mark.gpu
S0 = 0x1234567890abcdef1234567890abcdef
DSTEP = 0x0fedcba987654321
LAM = 0x30644e72e131a029048b6e193fd84104cc37a73fec2bc5e9b8ca0b2d36636f23


def _ctx(sbn, monkeypatch, glv, sort2_min=None):
    monkeypatch.setenv("SBN_MSM_GLV", str(glv))
    monkeypatch.delenv("SBN_MSM_C", raising=False)
    if sort2_min is not None:
        monkeypatch.setenv("SBN_SORT2_MIN", str(sort2_min))
    c = sbn.Context(0)
    monkeypatch.delenv("SBN_MSM_GLV"); monkeypatch.delenv("SBN_SORT2_MIN", raising=False)
    return c


@pytest.fixture()
def glv_pair(sbn, monkeypatch):
    """(GLV forced, GLV off), both taking the two-level sort from 1024 terms on, so that small MSMs can go through the GLV path"""
    on, off = _ctx(sbn, monkeypatch, 1, 1024), _ctx(sbn, monkeypatch, 0, 1024)
    yield on, off
    on.close(); off.close()


def wide_scalars(n, seed):
    """n canonical scalars of 253 bits (numpy, fast at millions)"""
    rng = np.random.default_rng(seed)
    k = rng.integers(0, 2**64, size=(n, 4), dtype=np.uint64)
    k[:, 3] &= np.uint64((1 << 61) - 1)
    return k.tobytes()


def dlog_sum(scal, first, n, R):
    """sum_i k_i (S0 + (first + i) DSTEP) mod r over 16-bit digits of the scalars (every partial sum exact in int64 / Python ints)"""
    k16 = np.frombuffer(scal, dtype="<u2").reshape(n, 16).astype(np.int64)
    idx = np.arange(first, first + n, dtype=np.int64)
    sk, sik = 0, 0
    for j in range(16):
        col = k16[:, j]
        sk += int(col.sum()) << (16 * j)
        sik += (int((col * (idx & 0xFFFF)).sum()) + (int((col * (idx >> 16)).sum()) << 16)) << (16 * j)
    return (S0 * sk + DSTEP * sik) % R


def expect(ol, pr, scal, first, n, mult=1):
    return ol.g1_mul(pr.point_to_xy(pr.G), (mult * dlog_sum(scal, first, n, pr.R) % pr.R).to_bytes(32, "little"))


def synth(ctx, n, first=0):
    return ctx.bases_synthetic(n, first, S0.to_bytes(32, "little"), DSTEP.to_bytes(32, "little"))


@pytest.mark.parametrize("n", [512, 1024, 3001, (1 << 16) + 1])
def test_glv_small_vs_plain_and_dlog(glv_pair, ol, pr, n):
    on, off = glv_pair
    b = synth(on, n, 3)
    try:
        sc = wide_scalars(n, 100 + n)
        want = expect(ol, pr, sc, 3, n)
        got_on = on.msm_bases(b, sc)
        job = on.prof_last_job()
        assert 13 <= job["c"] <= 17 and job["slots"] == 2 * n * job["W"] and job["W"] * job["c"] < 127 + job["c"]    # 2n entries per window of 127 bits
        assert got_on == off.msm_bases(b, sc) == (want, 0)
    finally:
        b.free()


def test_glv_edge_scalars_repeated_bases_and_infinity(glv_pair, ol, pr):
    """edge scalars (0, 1, r - 1, lambda, r - lambda, 2^127 +- 1, rounding boundaries of the split), all-equal scalars (one bucket per
    window holds every base), bases repeated (P + P in a bucket), a base with k and r - k (its terms cancel), an all-zero MSM"""
    on, off = glv_pair
    n, distinct = 8192, 512
    dl = rand_scalars(distinct, 55)
    pts = ol.g1_mul_gen_batch(dl, 8) * (n // distinct)
    dls = dl * (n // distinct)
    b = on.bases_upload(pts)
    G = pr.point_to_xy(pr.G)
    A, B, C = 0x6f4d8248eeb859fc8211bbeb7d4f1128, 0x89d3256894d213e3, 0x6f4d8248eeb859fd0be4e1541221250b
    try:
        edges = [0, 1, pr.R - 1, LAM, pr.R - LAM, (1 << 127) - 1, 1 << 127, (1 << 127) + 1, 1 << 253]
        edges += [(j * pr.R) // x + d for j in range(1, 40) for x in (B, C) for d in (0, 1)]
        vals = (edges * (n // len(edges) + 1))[:n]
        cases = {
            "edges": b"".join((v % pr.R).to_bytes(32, "little") for v in vals),
            "all equal": rand_scalars(1, 8) * n,
            "two values": rand_scalars(1, 9) * (n // 2) + rand_scalars(1, 10) * (n // 2),
            "zero": bytes(32 * n),
        }
        k = int.from_bytes(rand_scalars(1, 11), "little")
        canc = bytearray(32 * n)                                  # base 0 == base 512 == ...: k P_0 + (r - k) P_512 = 0
        canc[0:32] = k.to_bytes(32, "little"); canc[32 * distinct:32 * distinct + 32] = (pr.R - k).to_bytes(32, "little")
        cases["cancelling"] = bytes(canc)
        for name, sc in cases.items():
            out_on, inf_on = on.msm_bases(b, sc)
            assert (out_on, inf_on) == off.msm_bases(b, sc), name
            assert out_on == ol.g1_mul(G, ol.fr_dot(sc, dls)), name
            assert bool(inf_on) == (name in ("zero", "cancelling")), name
    finally:
        b.free()


def test_glv_rejects_non_canonical(glv_pair, ol, pr, sbn):
    on, _ = glv_pair
    n = 4096
    b = synth(on, n)
    try:
        sc = wide_scalars(n, 3)
        good = on.msm_bases(b, sc)
        bad = bytearray(sc); bad[32 * 77:32 * 78] = pr.R.to_bytes(32, "little")
        with pytest.raises(sbn.SbnError):
            on.msm_bases(b, bytes(bad))
        assert on.msm_bases(b, sc) == good == (expect(ol, pr, sc, 0, n), 0)
    finally:
        b.free()


def test_glv_fewer_scalars_than_bases_and_blind_base(glv_pair, ol, pr):
    """n < the handle's points (the images start at the table's half, not at n) and a handle with h (n + 1 points)"""
    on, off = glv_pair
    gx, _ = ol.gens_new(5000, b"gens_glv_test", 8)
    b = on.bases_upload(gx[:64 * 5000], gx[64 * 5000:])
    try:
        for m in (1024, 4999, 5000, 5001):
            sc = rand_scalars(m, 70 + m)
            want = ol.msm_pippenger(sc, gx[:64 * m], 8)
            assert on.msm_bases(b, sc)[0] == off.msm_bases(b, sc)[0] == want, m
    finally:
        b.free()


def test_glv_handle_recreated_and_derived(glv_pair, ol, pr):
    """a freed handle and a new one (often at the same address) never share a GLV table; split_at / scale handles build their own"""
    on, off = glv_pair
    n = 6000
    sc = wide_scalars(n, 21)
    for first in (0, 1000, 0):
        b = synth(on, n, first)
        try:
            assert on.msm_bases(b, sc)[0] == expect(ol, pr, sc, first, n), first
        finally:
            b.free()
    b = synth(on, n, 0)
    try:
        assert on.msm_bases(b, sc)[0] == expect(ol, pr, sc, 0, n)          # parent's table built first
        left, right = on.bases_split_at(b, 2500)
        try:
            assert on.msm_bases(left, sc[:32 * 2500])[0] == expect(ol, pr, sc[:32 * 2500], 0, 2500)
            assert on.msm_bases(right, sc[32 * 2500:])[0] == expect(ol, pr, sc[32 * 2500:], 2500, n - 2500)
        finally:
            left.free(); right.free()
        s = 0x5eed1234567
        sb = on.bases_scale(b, s.to_bytes(32, "little"))
        try:
            assert on.msm_bases(sb, sc)[0] == off.msm_bases(sb, sc)[0] == expect(ol, pr, sc, 0, n, s)
        finally:
            sb.free()
    finally:
        b.free()


@pytest.mark.parametrize("log_n", [19, 20, 22])
def test_glv_dlog_identity_large(sbn, monkeypatch, ol, pr, log_n):
    """the default sort threshold: GLV forced vs off vs the discrete-log identity at 2^19, 2^20 (the automatic rule takes GLV there) and 2^22
    (the automatic rule keeps the plain windows; forced it runs 8 x 2^23 additions)"""
    import torch
    n = 1 << log_n
    on, off, auto = _ctx(sbn, monkeypatch, 1), _ctx(sbn, monkeypatch, 0), _ctx(sbn, monkeypatch, -1)
    b = synth(on, n, 11)
    try:
        sc = wide_scalars(n, log_n)
        want = expect(ol, pr, sc, 11, n)
        d = torch.frombuffer(bytearray(sc), dtype=torch.uint8).cuda()
        torch.cuda.synchronize()
        assert on.msm_bases_dev(b, d.data_ptr(), n) == (want, 0)
        assert (on.prof_last_job()["c"], on.prof_last_job()["W"]) == (16, 8)
        assert off.msm_bases_dev(b, d.data_ptr(), n) == (want, 0)
        assert off.prof_last_job()["W"] > 8
        assert auto.msm_bases_dev(b, d.data_ptr(), n) == (want, 0)
        assert (auto.prof_last_job()["W"] == 8) == (log_n <= 20)
    finally:
        b.free(); on.close(); off.close(); auto.close()
