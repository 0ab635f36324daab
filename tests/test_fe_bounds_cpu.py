"""CPU: the constant tables and the value-range contracts of the lazy field / G1 layer (csrc/fp.cuh, csrc/g1.cuh), checked with
exact integers on the limb-exact model in tests/fe_model.py (which tests/test_gpu_fe_bounds.py pins to the device bit for bit).

Every case is first shown to be a legal input of its primitive (the model's pre_* checks restate fp.cuh's comments); then the
output range the comments state, the normal form and the value modulo p are asserted.  The biases of the unsigned fast path are
re-derived for every (K, J) the kernels instantiate, parsed from the sources, so a new instantiation is covered automatically."""
import os
import random
import re
from fractions import Fraction

import pytest

import fe_model as fm
import pyref

CS = os.path.join(fm.ROOT, "spartan-bn254_amd", "csrc")
FIELDS = {"FqP": fm.FQ, "FrP": fm.FR}


def inside(v, lo, hi, p):
    """lo p <= value < hi p, exactly (lo, hi given as decimals)"""
    x = fm.to_int(v) if isinstance(v, list) else v
    return Fraction(str(lo)) * p <= x < Fraction(str(hi)) * p


@pytest.mark.parametrize("F", [fm.FQ, fm.FR], ids=["Fq", "Fr"])
def test_constant_tables(F):
    p = F.p
    assert F.words() == [(p >> (32 * i)) & fm.U32 for i in range(8)]
    for name, want in (("P29", p), ("ONE29", pow(2, 261, p)), ("R2_29", pow(2, 522, p)), ("C256_29", pow(2, 256, p)),
                       ("CIN_29", pow(2, 266, p))):
        t = F.table(name)
        assert len(t) == 9 and all(0 <= x <= fm.MASK for x in t), name
        assert sum(x << (29 * i) for i, x in enumerate(t)) == want, f"{F.name}::{name}"
    assert (F.NINV29 * p) % (1 << 29) == (1 << 29) - 1, "NINV29 is not -p^-1 mod 2^29"
    assert re.search(r"PINV29 = \(0u - NINV29\) & LMASK;", F.body)
    assert (F.PINV29 * p) % (1 << 29) == 1
    one = F.table("ONE")
    assert len(one) == 8 and sum(x << (32 * i) for i, x in enumerate(one)) == pow(2, 261, p), f"{F.name}::ONE"
    # the top limb the fix-ups read: p = (P8 + f) 2^232 with 0 < f < 1
    assert F.P8 << 232 < p < (F.P8 + 1) << 232


def test_host_field_constants():
    src = open(os.path.join(CS, "host_field.hpp")).read()

    def arr(name, scope=src):
        m = re.search(r"static const uint64_t %s\[4\] = \{([^}]*)\}" % name, scope)
        return sum(int(x, 16) << (64 * i) for i, x in enumerate(re.findall(r"0x([0-9a-f]+)ull", m.group(1))))

    def word(name, scope=src):
        return int(re.search(r"static const uint64_t %s = 0x([0-9a-f]+)ull;" % name, scope).group(1), 16)

    P, R = pyref.P, pyref.R
    assert arr("QP") == P and arr("QONE") == pow(2, 256, P) and arr("QR2") == pow(2, 512, P)
    assert (word("QNINV") * P) % (1 << 64) == (1 << 64) - 1
    fr = src[src.index("namespace fr {"):]
    assert arr("P", fr) == R and arr("R2", fr) == pow(2, 512, R)
    assert (word("NINV", fr) * R) % (1 << 64) == (1 << 64) - 1


def bias_pairs():
    """every fe_subb<M, K, J> / fe_negb<M, K> (J = 1) instantiated in the kernels"""
    subb, negb = set(), set()
    for f in os.listdir(CS):
        if f.endswith((".cuh", ".hip", ".inc", ".hpp")):
            s = open(os.path.join(CS, f)).read()
            subb |= {(m, int(k), int(j)) for m, k, j in re.findall(r"fe_subb<(\w+), (\d+), (\d+)>", s)}
            negb |= {(m, int(k), 1) for m, k in re.findall(r"fe_negb<(\w+), (\d+)>", s)}
    return subb, negb


def test_bias_instantiations_found():
    subb, negb = bias_pairs()
    want = {("FrP", 3, 1), ("FrP", 4, 2), ("FrP", 9, 1), ("FrP", 14, 1), ("FqP", 2, 1), ("FqP", 4, 1), ("FqP", 4, 3), ("FqP", 6, 1)}
    assert want <= subb, "the parser lost an instantiation"
    assert {("FqP", 2, 1), ("FqP", 4, 1), ("FrP", 2, 1)} <= negb


@pytest.mark.parametrize("pair", sorted(bias_pairs()[0] | bias_pairs()[1]), ids=lambda t: "%s_%d_%d" % t)
def test_bias(pair):
    """bias29<M, K, J>: value K p; limbs 0..7 >= J 2^29 - J; a - b + bias has no negative limb for every legal a, b"""
    name, K, J = pair
    F = FIELDS[name]
    b = fm.bias(F, K, J)
    assert fm.to_int(b) == K * F.p
    assert all(x >= J * (1 << 29) - J for x in b[:8]), "limbs 0..7 below J 2^29 - J"
    # the worst legal subtrahend: J normalised values (limbs 0..7 at J (2^29 - 1)) and the largest top limb below (K - 0.001) p
    top_max = int(Fraction(K * 1000 - 1, 1000) * F.p / (1 << 232))
    worst = [J * fm.MASK] * 8 + [top_max]
    assert all(b[k] - worst[k] >= 0 for k in range(9)), "a - b + bias can go negative"
    # and the result's uint32 limbs: no wrap (fe_normu reads them unsigned), below 2^30.6 for J = 1 (fe_mulu / cols_mac_lazy)
    hi = [fm.MASK + b[k] for k in range(8)] + [int(4.5 * F.p) // (1 << 232) + b[8]]
    assert max(hi) < 1 << 32
    if J == 1:
        assert max(hi[:8]) < 2 ** 30.6
    rng = random.Random(K * 100 + J)
    for _ in range(200):
        a = fm.from_int(rng.randrange(0, 2 * F.p))
        parts = [fm.from_int(rng.randrange(0, int(min(F.p, (K - 0.001) * F.p / J)))) for _ in range(J)]
        bb = parts[0]
        for q in parts[1:]:
            bb = fm.fe_add_lazy(bb, q)
        if rng.random() < 0.3:
            bb = worst[:8] + [top_max - J]         # limbs 0..7 at their maximum, the value still legal
        assert fm.pre_subb(F, K, J, a, bb)
        exact = [a[k] - bb[k] + b[k] for k in range(9)]
        assert all(0 <= x < 1 << 32 for x in exact), "a limb of a - b + bias is negative or wraps"
        assert [fm.u32(x) for x in fm.fe_subb(F, K, J, a, bb)] == exact and sum(x << (29 * k) for k, x in enumerate(exact)) == fm.to_int(a) - fm.to_int(bb) + K * F.p
        if J == 1:
            r = fm.fe_negb(F, K, bb)
            assert all(x >= 0 for x in r) and fm.to_int(r) == K * F.p - fm.to_int(bb)


# ---------------------------------------------------------------- the model at the edges
@pytest.mark.parametrize("F", [fm.FQ, fm.FR], ids=["Fq", "Fr"])
def test_fix_tab_thresholds(F):
    """(-2p, 4.5p) -> [0, 2.5p), deciding on the top limb only: every threshold neighbourhood, low limbs all 0 / all 2^29 - 1"""
    P8, n = F.P8, 0
    tops = set()
    for t in (-2 * P8, -P8, 0, 2 * P8 + 2, int(4.5 * P8)):
        tops |= set(range(t - 3, t + 4))
    rng = random.Random(5)
    for top in sorted(tops):
        for low in (0, fm.MASK, rng.randrange(fm.MASK + 1)):
            x = fm.top_at(F, top, low)
            if not fm.pre_fix_tab(F, x):
                continue
            r = fm.fe_fix_tab(F, x)
            assert fm.is_normalised(r) and inside(r, 0, 2.5, F.p), (top, low)
            assert (fm.to_int(r) - fm.to_int(x)) % F.p == 0
            n += 1
    # the open ends themselves, exactly
    for x in (-2 * F.p + 1, -F.p - 1, -F.p, -F.p + 1, -1, 0, 2 * F.p - 1, 2 * F.p, 2 * F.p + 1, (9 * F.p) // 2 - 1):
        r = fm.fe_fix_tab(F, fm.from_int(x))
        assert inside(r, 0, 2.5, F.p) and (fm.to_int(r) - x) % F.p == 0, x
    assert n > 60


@pytest.mark.parametrize("F", [fm.FQ, fm.FR], ids=["Fq", "Fr"])
def test_maybe_zero_never_misses(F):
    """every k p with |k| <= 8 passes the filter, normalised or not, and as the biased differences of the hot formulas"""
    rng = random.Random(11)
    for k in range(-8, 9):
        x = k * F.p
        reps = [fm.from_int(x)] + [fm.unnormalised(x, rng) for _ in range(8)]
        if k > 0:
            for K in (2, 4, 6):                # fe_subb<K, 1>(a, b) with a - b = (k - K) p, before fe_normu
                if 0 < K - k + 1 <= K and k - K <= 1:
                    b = rng.randrange(0, F.p)
                    a = b + (k - K) * F.p
                    if a >= 0 and fm.pre_subb(F, K, 1, fm.from_int(a), fm.from_int(b)):
                        reps.append(fm.fe_subb(F, K, 1, fm.from_int(a), fm.from_int(b)))
        for v in reps:
            assert fm.to_int(v) == x and fm.fe_maybe_zero(F, v), (k, v)
    # and it is a filter: random non-zero values almost never pass
    hits = sum(fm.fe_maybe_zero(F, fm.from_int(rng.randrange(1, 8 * F.p))) for _ in range(2000))
    assert hits <= 2


@pytest.mark.parametrize("F", [fm.FQ, fm.FR], ids=["Fq", "Fr"])
def test_canon_small_edges(F):
    p = F.p
    rng = random.Random(3)
    xs = [-p + 1, -1, 0, 1, p - 1, p, p + 1, 2 * p - 1] + [rng.randrange(-p + 1, 2 * p) for _ in range(200)]
    for x in xs:
        v = fm.from_int(x)
        assert fm.pre_canon_small(F, v)
        r = fm.fe_canon_small(F, v)
        assert r == fm.from_int(x % p), x


@pytest.mark.parametrize("F", [fm.FQ, fm.FR], ids=["Fq", "Fr"])
def test_reduce_and_mul_ranges(F):
    """fe_reduce: |a| < 13p -> (-0.1p, 1.1p); fe_mul: |ab| < 169 p^2 -> (-p, 2p), |a|, |b| < 2p -> (-0.1p, 1.1p); fe_mulu: [0, ab/2^261 + p)"""
    p, rinv = F.p, pow(fm.RMONT, -1, F.p)
    rng = random.Random(7)
    near = [13 * p - 1, 13 * p - (1 << 200), 13 * p - p // 3] + [rng.randrange(12 * p, 13 * p) for _ in range(40)]
    for x in near + [-v for v in near]:
        for v in (fm.from_int(x), fm.unnormalised(x, rng)):
            assert fm.pre_reduce(F, v)
            r = fm.fe_reduce(F, v)
            assert fm.is_normalised(r) and inside(r, -0.1, 1.1, p) and (fm.to_int(r) - x) % p == 0
    for a in (13 * p - 1, -(13 * p - 1), 2 * p - 1, -(2 * p - 1), p, 0):
        for b in (13 * p - 1, -(13 * p - 1), 2 * p - 1, -(2 * p - 1), 1, -1):
            if abs(a * b) >= 169 * p * p:
                continue
            va, vb = fm.from_int(a), fm.from_int(b)
            assert fm.pre_mul(va, vb)
            r = fm.to_int(fm.fe_mul(F, va, vb))
            assert -p < r < 2 * p and (r - a * b * rinv) % p == 0
            if abs(a) < 2 * p and abs(b) < 2 * p:
                assert -0.1 * p < r < 1.1 * p
            r = fm.to_int(fm.fe_sqr(F, va))
            assert -p < r < 2 * p and (r - a * a * rinv) % p == 0
    # unsigned: operands at the fe_mulu limits (a biased difference times a normalised value; two 2-term sums)
    for _ in range(100):
        a = fm.fe_subb(F, 6, 1, fm.from_int(rng.randrange(2 * p)), fm.from_int(rng.randrange(5 * p)))
        b = fm.from_int(rng.randrange(1 << 256))
        for x, y in ((a, b), ([fm.MASK * 2] * 8 + [2 * F.P8], [fm.MASK * 2] * 8 + [2 * F.P8])):
            assert fm.pre_mulu(x, y)
            r = fm.fe_mulu(F, x, y)
            vx, vy = fm.to_int(x), fm.to_int(y)
            assert fm.is_normalised(r) and 0 <= fm.to_int(r) < Fraction(vx * vy, fm.RMONT) + p and (fm.to_int(r) - vx * vy * rinv) % p == 0
        sq = [fm.MASK * 2] * 8 + [2 * F.P8 + 1]
        assert fm.pre_squ(sq)
        r = fm.fe_squ(F, sq)
        assert 0 <= fm.to_int(r) < Fraction(fm.to_int(sq) ** 2, fm.RMONT) + p


def wide_edges(F, rng):
    """values at the top of fe_reduce's wide domain (|a| < 448 p) and at the sums the equal-base merge feeds it (160, 320 r)"""
    p, K = F.p, fm.REDUCE_WIDE
    xs = [K * p - 1, K * p - (1 << 200), K * p - p // 3, (K - 1) * p, (K - 1) * p + 1, 320 * p - 1, 320 * p, 160 * p + 1, 13 * p, 13 * p + 1]
    xs += [rng.randrange(13 * p, K * p) for _ in range(40)]
    return xs + [-x for x in xs]


@pytest.mark.parametrize("F", [fm.FQ, fm.FR], ids=["Fq", "Fr"])
def test_reduce_wide_contract_derivation(F):
    """the second line of fe_reduce's contract, from the arithmetic: e = ONE29 / 2^261 < 1 / 594 bounds the output, the signed
    column bound of fe_mul against ONE29 bounds the top limb; 448 p satisfies both with room, and covers the merge's 320 r"""
    p, K = F.p, fm.REDUCE_WIDE
    e = Fraction(fm.to_int(F.ONE29), fm.RMONT)
    assert Fraction(1, 595) < e < Fraction(1, 594)
    assert K * p * e < Fraction(76, 100) * p and fm.REDUCE_TIGHT * p * e < Fraction(1, 10) * p      # (-0.76p, 1.76p) and (-0.1p, 1.1p)
    assert 594 * p * e < p < 595 * p * e                                                             # (-p, 2p) itself would hold up to 594 p
    amax = ((1 << 63) - 9 * (1 << 58) - 1) // (9 * max(F.ONE29))                                     # 9 |a_k| max ONE29 + 9 2^58 < 2^63
    assert amax >= 1 << 30                                                                          # limbs 0..7 of any fe_add_lazy of two normalised values
    kmax = (amax - 1) // (F.P8 + 1)                                                                 # |top limb| <= K (P8 + 1) + 1
    assert K <= kmax and kmax == {"FqP": 473, "FrP": 451}[F.name]
    assert fm.pre_mul([fm.MASK] * 8 + [K * (F.P8 + 1) + 1], F.ONE29) and not fm.pre_mul([fm.MASK] * 8 + [amax + 1], F.ONE29)
    assert K * 10 >= 320 * 14                                                                       # 40 % above the largest sum of the merge


@pytest.mark.parametrize("F", [fm.FQ, fm.FR], ids=["Fq", "Fr"])
def test_reduce_canon_is_zero_wide_domain(F):
    """|a| < 448 p, normalised or not, both signs: fe_reduce lands in [a e, a e + p), inside (-0.76p, 1.76p); fe_canon and
    fe_is_zero are exact"""
    p = F.p
    rng = random.Random(29)
    n = 0
    for x in wide_edges(F, rng):
        for v in (fm.from_int(x), fm.unnormalised(x, rng)):
            assert fm.pre_reduce(F, v, wide=True) and not fm.pre_reduce(F, v)
            r = fm.fe_reduce(F, v)
            lo, hi = fm.reduce_interval(F, v)
            assert fm.is_normalised(r) and lo <= fm.to_int(r) < hi and inside(r, -0.76, 1.76, p) and (fm.to_int(r) - x) % p == 0
            assert fm.pre_canon_small(F, r)
            assert fm.fe_canon(F, v) == fm.from_int(x % p), x
            assert fm.fe_is_zero(F, v) == (x % p == 0)
            n += 1
    for k in (14, 160, 320, 400, fm.REDUCE_WIDE - 1):                  # every k p is zero, its neighbours are not
        for s in (1, -1):
            for v in (fm.from_int(s * k * p), fm.unnormalised(s * k * p, rng)):
                assert fm.pre_reduce(F, v, wide=True) and fm.fe_is_zero(F, v) and fm.fe_canon(F, v) == [0] * 9
            assert not fm.fe_is_zero(F, fm.from_int(s * k * p + 1)) and not fm.fe_is_zero(F, fm.unnormalised(s * k * p - 1, rng))
    assert n >= 200
    # outside the domain the model says so: the value bound first, the column bound before (-p, 2p) is lost
    assert not fm.pre_reduce(F, fm.from_int(fm.REDUCE_WIDE * p), wide=True)
    assert not fm.pre_mul(fm.from_int(512 * p), F.ONE29)


@pytest.mark.parametrize("F", [fm.FQ, fm.FR], ids=["Fq", "Fr"])
def test_cols_at_capacity(F):
    """6 products, a carry pass, 6 more, one reduction, every limb at 2^29 - 1; and the lazy two-product form at its limits"""
    p, rinv = F.p, pow(fm.RMONT, -1, F.p)
    s, total = fm.cols_zero(), 0
    full = [fm.MASK] * 8 + [3 * F.P8]                  # limbs 0..7 at their maximum, the value ~3p (a [0, 2.5p) table entry and more)
    for i in range(12):
        fm.cols_mac(s, full, full)
        total += fm.to_int(full) ** 2
        if i == 5:
            fm.cols_carry(s)
    r = fm.cols_reduce(F, s)
    assert fm.is_normalised(r) and 0 <= fm.to_int(r) < Fraction(total, fm.RMONT) + p and (fm.to_int(r) - total * rinv) % p == 0
    # g1.cuh's Y3: R (< 5.2p) times Q - X3 + 6p (fe_subb<6, 1>: limbs up to 2^29 - 1 + bias), plus PPP times 4p - Y (fe_negb<4>)
    R = [fm.MASK] * 8 + [int(5.2 * F.P8)]
    t1 = fm.fe_subb(F, 6, 1, [fm.MASK] * 8 + [F.P8 + 1], [0] * 9)
    t2 = fm.fe_negb(F, 4, [0] * 9)
    s = fm.cols_zero()
    fm.cols_mac(s, R, t1)
    fm.cols_mac(s, full, t2)
    fm.cols_reduce(F, s)


@pytest.mark.parametrize("F", [fm.FQ], ids=["Fq"])
def test_fix_nonneg_edges(F):
    for K in (1, 2, 4):
        for x in (-K * F.p + 1, -1, 0, 1, F.p, (1 << 256) - K * F.p - 1):
            v = fm.from_int(x)
            assert fm.pre_fix_nonneg(F, K, v)
            r = fm.fe_fix_nonneg(F, K, v)
            assert fm.is_normalised(r) and 0 <= fm.to_int(r) < 1 << 256 and (fm.to_int(r) - x) % F.p == 0
            if x == 0:
                assert r == [0] * 9


# ---------------------------------------------------------------- G1 formulas on the model, coordinates at the top of their ranges
def check_xyzz(F, pt, want, where):
    for name, v, lim in zip(fm.RANGES, pt, fm.RANGES.values()):
        assert fm.is_normalised(v) and 0 <= fm.to_int(v) < lim * F.p, (where, name, fm.ratio(F, v))
    assert fm.xyzz_affine(pt) == want, where


def g1_cases(seed, n):
    """(acc point, q point) pairs, plain affine ints: random, equal, opposite, infinity on either side"""
    rng = random.Random(seed)
    pts = [pyref.mul(pyref.G, rng.randrange(1, pyref.R)) for _ in range(n)]
    out = []
    for i, a in enumerate(pts):
        b = pts[(i + 1) % n]
        out += [(a, b), (a, a), (a, pyref.neg(a)), (None, a), (a, None)]
    return rng, out


def test_g1_model_at_range_tops():
    """xyzz_madd (both signs) and xyzz_add_inl: every intermediate the comments bound, and every output coordinate, on inputs at
    the top of their ranges; the affine result against pyref"""
    F = fm.FQ
    rng, cases = g1_cases(21, 12)
    for a, b in cases:
        la, lb = rng.randrange(2, F.p), rng.randrange(2, F.p)
        acc = fm.xyzz_of(a, la)
        for neg in (False, True):
            q = pyref.neg(b) if neg else b
            tr = {}
            r = fm.xyzz_madd(acc, fm.affine_of(b), neg, tr)
            check_xyzz(F, r, pyref.add(a, q), ("madd", neg))
            if "P" in tr:
                assert 0.8 * F.p < fm.to_int(tr["P"]) < 7.2 * F.p and 0.8 * F.p < fm.to_int(tr["R"]) < 5.2 * F.p
                assert fm.pre_subb(F, 6, 1, tr["U2"], acc[0]) and fm.pre_subb(F, 4, 1, tr["S2"], acc[1])
            if "X3" in tr:
                assert 0.4 * F.p < fm.to_int(tr["X3"]) < 5.2 * F.p
                assert fm.pre_subb(F, 4, 3, tr["RR"], fm.fe_add_lazy(fm.fe_add_lazy(tr["PPP"], tr["Q"]), tr["Q"]))
                assert max(tr["t1"][:8] + tr["t2"][:8]) < 2 ** 30.6
        tr = {}
        r = fm.xyzz_add_inl(acc, fm.xyzz_of(b, lb), tr)
        check_xyzz(F, r, pyref.add(a, b), "add_inl")
        if "P" in tr:
            assert 0.8 * F.p < fm.to_int(tr["P"]) < 3.2 * F.p and 0.8 * F.p < fm.to_int(tr["R"]) < 3.2 * F.p


def test_g1_model_store_and_doubling():
    """xyzz_dbl's signed X (down to -2.2p) and Y (-1.2p, 1.2p) before the fix-ups; the store -> load round trip keeps the point"""
    F = fm.FQ
    rng = random.Random(9)
    for i in range(24):
        a = pyref.mul(pyref.G, rng.randrange(1, pyref.R))
        acc = fm.xyzz_of(a, rng.randrange(2, F.p))
        r, (X, Y) = fm.xyzz_dbl(acc)
        assert -2.2 * F.p < fm.to_int(X) < 1.1 * F.p and -1.2 * F.p < fm.to_int(Y) < 1.2 * F.p
        check_xyzz(F, r, pyref.add(a, a), "dbl")
        r2, (X, Y) = fm.xyzz_dbl_affine(*fm.affine_of(a))
        assert -2.2 * F.p < fm.to_int(X) < 1.1 * F.p and -1.2 * F.p < fm.to_int(Y) < 1.2 * F.p
        check_xyzz(F, r2, pyref.add(a, a), "dbl_affine")
        for p in (acc, r):
            assert fm.xyzz_affine(fm.xyzz_store_load(p)) == fm.xyzz_affine(p)


# ---------------------------------------------------------------- the biases and fix-ups at each call site of g1.cuh
def body(src, name, end="\n}\n"):
    i = src.index(name + "(")
    return src[i:src.index(end, i)]


# (function, call pattern with the bias captured, bound of the subtrahend in units of p, number of normalised terms in it)
SITES = [
    ("xyzz_madd", r"fe_negb<FqP, (\d+)>\(q_in\.y\)", 1.0, 1),                                   # canonical table y
    ("xyzz_madd", r"fe_subb<FqP, (\d+), (\d+)>\(U2, acc\.X\)", 5.2, 1),
    ("xyzz_madd", r"fe_subb<FqP, (\d+), (\d+)>\(S2, acc\.Y\)", 3.2, 1),
    ("xyzz_madd", r"fe_subb<FqP, (\d+), (\d+)>\(fe_squ\(R\), fe_add_lazy", 3.3, 3),             # PPP + 2Q, each < 1.1p
    ("xyzz_madd", r"fe_subb<FqP, (\d+), (\d+)>\(Q, X3\)", 5.2, 1),
    ("xyzz_madd", r"fe_negb<FqP, (\d+)>\(acc\.Y\)", 3.2, 1),
    ("xyzz_add_inl", r"fe_subb<FqP, (\d+), (\d+)>\(U2, U1\)", 1.2, 1),
    ("xyzz_add_inl", r"fe_subb<FqP, (\d+), (\d+)>\(S2, S1\)", 1.2, 1),
    ("xyzz_add_inl", r"fe_subb<FqP, (\d+), (\d+)>\(fe_squ\(R\), fe_add_lazy", 3.3, 3),
    ("xyzz_add_inl", r"fe_subb<FqP, (\d+), (\d+)>\(Q, r\.X\)", 5.2, 1),
    ("xyzz_add_inl", r"fe_negb<FqP, (\d+)>\(S1\)", 1.2, 1),
    ("xyzz_add_quad", r"fe_subb<FqP, (\d+), (\d+)>\(U2, U1\)", 1.2, 1),
    ("xyzz_add_quad", r"fe_subb<FqP, (\d+), (\d+)>\(S2, S1\)", 1.2, 1),
    ("xyzz_add_quad", r"fe_subb<FqP, (\d+), (\d+)>\(RR, fe_add_lazy", 3.3, 3),
    ("xyzz_add_quad", r"fe_subb<FqP, (\d+), (\d+)>\(Q, r\.X\)", 5.2, 1),
    ("xyzz_add_quad", r"fe_subb<FqP, (\d+), (\d+)>\(fe_quad_bcast<0>\(t4\), fe_quad_bcast<1>\(t4\)\)", 1.2, 1),   # T2 = S1 PPP
]
# fe_fix_nonneg<FqP, K> before a store: K p must cover the most negative value that can reach it
FIXES = [
    ("xyzz_store", r"fe_fix_nonneg<FqP, (\d+)>\(fe_norm\(a\.X\)\)", 2.2),      # xyzz_dbl's signed X, (-2.2p, 1.1p)
    ("xyzz_store", r"fe_fix_nonneg<FqP, (\d+)>\(fe_norm\(a\.Y\)\)", 1.2),
    ("xyzz_store", r"fe_fix_nonneg<FqP, (\d+)>\(fe_norm\(a\.ZZ\)\)", 1.0),
    ("xyzz_store", r"fe_fix_nonneg<FqP, (\d+)>\(fe_norm\(a\.ZZZ\)\)", 1.0),
    ("xyzz_dbl_affine", r"r\.X = fe_fix_nonneg<FqP, (\d+)>\(X\)", 2.2),
    ("xyzz_dbl_affine", r"r\.Y = fe_fix_nonneg<FqP, (\d+)>", 1.2),
    ("xyzz_dbl(", r"r\.X = fe_fix_nonneg<FqP, (\d+)>\(X\)", 2.2),
    ("xyzz_dbl(", r"r\.Y = fe_fix_nonneg<FqP, (\d+)>", 1.2),
]


def test_g1_call_site_biases():
    """each fe_subb / fe_negb in g1.cuh has K p above its subtrahend's range (K - 0.001 > bound) and J >= its number of terms,
    and each fix-up before a store adds enough multiples of p; the model's G1 formulas use the same constants"""
    src = open(os.path.join(CS, "g1.cuh")).read()
    model = open(os.path.join(fm.ROOT, "tests", "fe_model.py")).read()
    for fn, pat, bound, terms in SITES:
        m = re.search(pat, body(src, fn))
        assert m, (fn, pat)
        K, J = int(m.group(1)), int(m.group(2)) if m.lastindex > 1 else 1
        assert K - 0.001 > bound and J >= terms, f"{fn}: {m.group(0)} cannot absorb a subtrahend below {bound}p"
    for fn, pat, low in FIXES:
        m = re.search(pat, body(src, fn.rstrip("(")) if not fn.endswith("(") else body(src, "XYZZ xyzz_dbl"))
        assert m, (fn, pat)
        assert int(m.group(1)) >= low, f"{fn}: {m.group(0)} leaves values down to -{low}p negative"
    # the limb-exact model hard-codes the same biases (tests/test_gpu_fe_bounds.py compares the device with it bit for bit)
    for fn in ("xyzz_madd", "xyzz_add_inl"):
        got = re.findall(r"fe_(subb|negb)<FqP, (\d+)(?:, (\d+))?>", body(src, fn))
        want = re.findall(r"fe_(subb|negb)\(F, (\d+)(?:, (\d+))?", body(model, "def " + fn, "\n\n\ndef "))
        assert got == want, (fn, got, want)
