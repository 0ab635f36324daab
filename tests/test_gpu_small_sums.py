"""GPU: sbn_g1_small_sums (k_window_sums: one block per (sum, 4-bit window), no table, the 64 window sums folded on the host) against the
oracle's MSM, bit for bit: every count at which a block is empty, partly filled or full, every number of sums from one to the cap, the scalars
at the edges of a window and of the top window, the inputs that take the degenerate branches of the addition, the refusals, and the launches."""
import ctypes as C

import pytest

import oracle_lib as ol
import polyeval_model as pm
from polyeval_model import INF, R_MOD, sb

pytestmark = pytest.mark.gpu
Q_MOD = 0x30644e72e131a029b85045b68181585d97816a916871ca8d3c208c16d87cfd47
COUNTS = [0, 1, 2, 3, 63, 64]
EDGE_SCALARS = [0, 1, 15, 16, R_MOD - 1] + [1 << b for b in (0, 3, 4, 251, 252, 253)] + [(1 << 253) - 1]

_POOL = []


def pool():
    """133 distinct points, computed once"""
    if not _POOL:
        raw = ol.g1_mul_gen_batch(b"".join(sb(7 * i + 3) for i in range(133)), 1)
        _POOL.extend(raw[64 * i:64 * i + 64] for i in range(133))
    return _POOL


def want_sum(scalars, points):
    return pm.msm(scalars, points) if scalars else INF


def run(ctx, sums):
    """sums: [(scalars, points)] -> the call's (points, flags), checked for shape"""
    pts = b"".join(b"".join(p) for _, p in sums)
    sc = b"".join(b"".join(sb(s) for s in ss) for ss, _ in sums)
    xy, inf = ctx.g1_small_sums(pts, sc, [len(ss) for ss, _ in sums])
    assert len(xy) == 64 * len(sums) and len(inf) == len(sums)
    return [xy[64 * i:64 * i + 64] for i in range(len(sums))], list(inf)


def check(ctx, sums):
    got, inf = run(ctx, sums)
    for i, (ss, pp) in enumerate(sums):
        w = want_sum(ss, pp)
        assert got[i] == w, (i, len(ss))
        assert inf[i] == (1 if w == INF else 0), i


def _mixed(nsums, seed):
    """nsums sums whose counts run through COUNTS, scalars of full width, points from the pool at a moving offset"""
    P = pool()
    sums = []
    for i in range(nsums):
        n = COUNTS[(i + seed) % len(COUNTS)]
        ss = [pow(5, 1 + 97 * i + j + seed, R_MOD) for j in range(n)]
        sums.append((ss, [P[(3 * i + j) % len(P)] for j in range(n)]))
    return sums


@pytest.mark.parametrize("nsums", [1, 3, 70, 256])
def test_sums_equal_the_oracles_msm_at_every_count(ctx, nsums):
    sums = _mixed(nsums, 0)
    assert nsums < len(COUNTS) or {len(s) for s, _ in sums} == set(COUNTS)
    check(ctx, sums)


@pytest.mark.parametrize("count", COUNTS)
def test_one_sum_of_each_count(ctx, count):
    P = pool()
    check(ctx, [([pow(3, 11 + j, R_MOD) for j in range(count)], P[:count])])


def test_scalars_at_the_edges_of_a_window_and_of_the_top_window(ctx):
    P = pool()
    alone = [([s], [P[i]]) for i, s in enumerate(EDGE_SCALARS)]
    together = (EDGE_SCALARS, P[20:20 + len(EDGE_SCALARS)])
    top_only = ([1 << 252, 1 << 253, 3 << 252], P[40:43])                 # every non-zero digit lies in window 63
    assert 3 << 252 < R_MOD
    check(ctx, alone + [together, top_only])


def test_inputs_that_take_the_degenerate_branches(ctx):
    P = pool()
    s = pow(7, 77, R_MOD)
    cases = [
        ([1] * 64, [P[0]] * 64),                                         # every level of the tree doubles: 64 P
        ([s, s], [P[1], ol.g1_neg(P[1])]),                               # P and -P: the identity
        ([s, R_MOD - s], [P[2], P[2]]),                                  # s P - s P: the identity
        ([s, s, 5], [P[3], P[3], P[4]]),                                 # a repeated point beside another
        ([s, 9, 11, s], [INF, P[5], INF, INF]),                          # identity points among the inputs
        ([s, 3], [INF, INF]),                                            # nothing but identities
        ([0, 0, 0], P[6:9]),                                             # nothing but zero scalars
    ]
    got, inf = run(ctx, cases)
    for i, (ss, pp) in enumerate(cases):
        assert got[i] == want_sum(ss, pp), i
    assert got[0] == ol.g1_mul(P[0], sb(64))
    assert [got[i] for i in (1, 2, 5, 6)] == [INF] * 4
    assert inf == [0, 1, 1, 0, 0, 1, 1]


def test_no_sums_is_no_work(ctx):
    ctx.prof_enable(True)
    try:
        ctx.prof_reset()
        assert ctx.g1_small_sums(b"", b"", []) == (b"", b"")
        assert ctx.prof_get() == {}
    finally:
        ctx.prof_enable(False)


def test_refusals_come_before_any_launch(ctx, sbn):
    P = pool()
    off_curve = P[0][:32] + P[1][32:]
    assert not ol.g1_on_curve(off_curve)
    x_plus_p = (pm.ib(P[0][:32]) + Q_MOD).to_bytes(32, "little") + P[0][32:]      # the same point, x not canonical
    bad = [
        (b"".join(P[:65]), b"".join(sb(1) for _ in range(65)), [65]),
        (b"", b"", [0] * 257),
        (P[0] + P[1], sb(1) + R_MOD.to_bytes(32, "little"), [1, 1]),
        (P[0] + P[1], sb(1) + b"\xff" * 32, [2]),
        (P[0] + off_curve, sb(1) + sb(2), [2]),
        (x_plus_p, sb(1), [1]),
    ]
    ctx.prof_enable(True)
    try:
        ctx.prof_reset()
        for pts, sc, counts in bad:
            with pytest.raises(sbn.SbnError):
                ctx.g1_small_sums(pts, sc, counts)
        L = sbn.lib()
        buf = lambda k: (C.c_uint8 * k)()                                # noqa: E731
        one = (C.c_uint32 * 1)(1)
        for args in ((None, buf(32), one, buf(64)), (buf(64), None, one, buf(64)), (buf(64), buf(32), None, buf(64)), (buf(64), buf(32), one, None)):
            assert L.sbn_g1_small_sums(ctx.h, args[0], args[1], args[2], C.c_size_t(1), args[3], None) == -1
        assert ctx.prof_get() == {}, "a refused call launched something"
    finally:
        ctx.prof_enable(False)
    check(ctx, _mixed(3, 1))                                             # and the context serves the next call


@pytest.mark.parametrize("nsums", [1, 70, 256])
def test_one_launch_whatever_the_number_of_sums(ctx, nsums):
    sums = _mixed(nsums, 2)
    ctx.prof_enable(True)
    try:
        ctx.prof_reset()
        check(ctx, sums)
        prof = {k: v[1] for k, v in ctx.prof_get().items()}
    finally:
        ctx.prof_enable(False)
    assert prof == {"k_window_sums": 1, "k_sums_to_host": 1}


def test_a_call_between_two_msms_leaves_them_as_a_fresh_context_computes_them(ctx, sbn):
    P = pool()
    n = 100
    sc = b"".join(sb(pow(11, i + 1, R_MOD)) for i in range(n))
    pts = b"".join(P[i] for i in range(n))
    sums = _mixed(5, 3)
    first = ctx.msm(sc, pts)
    mid = run(ctx, sums)
    second = ctx.msm(sc[:32 * 40], pts[:64 * 40])
    fresh = sbn.Context(0)
    try:
        assert run(fresh, sums) == mid
        assert fresh.msm(sc, pts) == first and fresh.msm(sc[:32 * 40], pts[:64 * 40]) == second
    finally:
        fresh.close()
    assert first[0] == ol.msm_pippenger(sc, pts, 4)
