"""CPU: tests/pairing_model.py anchored without any outside library — the curve constants, the twist and its order, the lines of a table, the
non-degeneracy and bilinearity of the pairing, the independence of the schedule, the kernel's final-exponentiation program and Frobenius
constants (tools/gen_pairing_consts.py) against the literal exponent, and the KZG verdict against the G1 relation a known tau allows."""
import os
import random
import sys

import pytest

import pairing_model as pm
import sparse_eval_kzg_model as skm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import gen_pairing_consts as gen  # noqa: E402

U, Q, R = pm.U, pm.Q, pm.R


@pytest.fixture(scope="module")
def e_gen():
    return pm.pairing(pm.G1, pm.G2)


def test_constants():
    assert Q == 0x30644e72e131a029b85045b68181585d97816a916871ca8d3c208c16d87cfd47
    assert R == skm.R == 0x30644e72e131a029b85045b68181585d2833e84879b9709143e1f593f0000001 and U == 4965661367192848881
    assert Q == 36 * U**4 + 36 * U**3 + 24 * U**2 + 6 * U + 1 and R == 36 * U**4 + 36 * U**3 + 18 * U**2 + 6 * U + 1
    assert pm.ATE.bit_length() == 65 and bin(pm.ATE).count("1") == 37
    assert pm.f2_mul(pm.B_TWIST, pm.XI) == (3, 0)
    assert (Q**12 - 1) % R == 0 and (Q**4 - Q**2 + 1) % R == 0


def test_generator_and_the_order_of_the_twist():
    assert pm.g2_on_curve(pm.G2) and pm.g2_mul(pm.G2, R) is None and pm.g2_in_subgroup(pm.G2)
    for s in (1, 2, 3):
        P = pm.g2_curve_point(s)
        assert pm.g2_on_curve(P) and pm.g2_mul(P, R * (2 * Q - R)) is None          # #E'(Fq2) = r (2q - r)
        assert not pm.g2_in_subgroup(P) and pm.g2_in_subgroup(pm.g2_mul(P, pm.COFACTOR))
    # Hasse over Fq2: |#E'(Fq2) - (q^2 + 1)| <= 2q, so r (2q - r) is the ONLY multiple of itself in range: the group order, not a multiple of it
    n = R * (2 * Q - R)
    assert abs(n - (Q * Q + 1)) <= 2 * Q and 2 * n > Q * Q + 1 + 2 * Q
    assert pm.f2_sqrt(pm.XI) is None                                                 # xi is no square: w^6 - xi can be irreducible


def _untwist(P):
    """(x, y) -> (x w^2, y w^3) as Fq12 values"""
    return pm.f12_from_fq2(P[0], 2), pm.f12_from_fq2(P[1], 3)


def _f12_add(a, b):
    return tuple(pm.f2_add(x, y) for x, y in zip(a, b))


def test_the_untwisted_generator_lies_on_the_curve_over_fq12():
    X, Y = _untwist(pm.G2)
    three = pm.f12_from_fq2((3, 0))
    assert pm.f12_mul(Y, Y) == _f12_add(pm.f12_mul(X, pm.f12_mul(X, X)), three)


def _line_at(line, X, Y):
    """l(X, Y) = Y - lam X w + (lam xT - yT) w^3 at a point with Fq12 coordinates"""
    _, nl, cc = line
    return _f12_add(_f12_add(Y, pm.f12_mul(pm.f12_from_fq2(nl, 1), X)), pm.f12_from_fq2(cc, 3))


@pytest.mark.parametrize("sched", ["binary", "naf"])
def test_every_line_vanishes_at_the_points_it_passes_through(sched):
    schedule = pm.schedule_binary() if sched == "binary" else pm.schedule_naf()
    assert sum(d * 2**i for i, d in enumerate(reversed(schedule))) == pm.ATE and schedule[0] == 1
    Qp = pm.g2_from_seed(4)
    table = pm.line_table(Qp, schedule)
    assert len(table) == len(schedule) - 1 + sum(1 for d in schedule[1:] if d) + 2
    zero = (pm.F2_ZERO,) * 6
    T, i = Qp, 0
    nq = pm.g2_neg(Qp)
    q1 = pm.g2_frobenius(Qp)
    q2 = pm.g2_neg(pm.g2_frobenius(q1))
    assert pm.g2_on_curve(q1) and q1 == pm.g2_mul(Qp, Q % R)                        # pi acts on G2 as multiplication by q
    steps = []
    for d in schedule[1:]:
        steps.append((None, 1))
        if d:
            steps.append((Qp if d > 0 else nq, 0))
    steps += [(q1, 0), (q2, 0)]
    for other, sq in steps:
        B = T if other is None else other
        assert table[i][0] == sq
        for pt in (T, B, pm.g2_neg(pm.g2_add(T, B))):
            assert _line_at(table[i], *_untwist(pt)) == zero
        T = pm.g2_add(T, B)
        i += 1
    assert i == len(table)


def test_non_degenerate_and_of_order_r(e_gen):
    assert e_gen != pm.F12_ONE and pm.f12_pow(e_gen, R) == pm.F12_ONE
    assert pm.pairing(None, pm.G2) == pm.F12_ONE and pm.pairing_product([]) == pm.F12_ONE


@pytest.mark.parametrize("a,b", [(1, 1), (2, 1), (1, 2), (R - 1, 1), (1, R - 1), (R - 1, R - 1), (None, None)])
def test_bilinear_in_each_argument(e_gen, a, b):
    rng = random.Random(5)
    a = rng.randrange(1, R) if a is None else a
    b = rng.randrange(1, R) if b is None else b
    assert pm.pairing(pm.g1_mul(pm.G1, a), pm.g2_mul(pm.G2, b)) == pm.f12_pow(e_gen, a * b % R)


def test_inverse_pairs_cancel_in_a_product(e_gen):
    P = pm.g1_mul(pm.G1, 991)
    Qp = pm.g2_from_seed(2)
    assert pm.f12_mul(pm.pairing(P, Qp), pm.pairing(pm.g1_neg(P), Qp)) == pm.F12_ONE
    assert pm.pairing_product([(P, Qp), (pm.g1_neg(P), Qp)]) == pm.F12_ONE
    assert pm.pairing_product([(P, Qp), (pm.G1, pm.G2)]) == pm.f12_mul(pm.pairing(P, Qp), e_gen)


def test_the_value_does_not_depend_on_the_schedule(e_gen):
    assert pm.schedule_naf() != pm.schedule_binary() and sum(1 for d in pm.schedule_naf() if d) == 22
    assert pm.pairing(pm.G1, pm.G2, pm.schedule_naf()) == e_gen
    P, Qp = pm.g1_mul(pm.G1, 77), pm.g2_from_seed(3)
    assert pm.pairing(P, Qp, pm.schedule_naf()) == pm.pairing(P, Qp)


def test_gt_bytes_order():
    f = tuple((2 * i + 1, 2 * i + 2) for i in range(6))                              # coefficient of w^i
    got = [int.from_bytes(pm.gt_bytes(f)[32 * k:32 * k + 32], "little") for k in range(12)]
    assert got == [1, 2, 5, 6, 9, 10, 3, 4, 7, 8, 11, 12]                             # c0 = (w^0, w^2, w^4), c1 = (w^1, w^3, w^5)


def test_frobenius_constants_and_the_exact_hard_part():
    f = pm.miller(pm.g1_mul(pm.G1, 31), pm.line_table(pm.g2_from_seed(6), pm.schedule_naf()))
    for k in (1, 2, 3):
        assert pm.f12_frobenius(f, k) == pm.f12_pow(f, Q**k)
    assert sum(l * Q**i for i, l in enumerate(pm.LAMBDA)) == (Q**4 - Q**2 + 1) // R


def test_the_kernels_final_exponentiation_program_is_the_literal_exponent():
    prog = gen.final_exp_program()
    assert all(0 <= s < 10 for (_, d, a, b) in prog for s in (d, a, b))
    for seed in (1, 2):
        f = pm.miller(pm.g1_mul(pm.G1, 1000 + seed), pm.line_table(pm.g2_from_seed(seed), pm.schedule_naf()))
        S = [None] * 10
        S[0] = f
        for op, d, a, b in prog:
            if op == gen.MUL:
                S[d] = pm.f12_mul(S[a], S[b])
            elif op == gen.FROB:
                S[d] = pm.f12_frobenius(S[a])
            elif op == gen.CONJ:
                S[d] = pm.f12_conj(S[a])
            else:
                assert S[a][0][1] == 0 and all(c == pm.F2_ZERO for c in S[a][1:]), "the inversion's operand lies in Fq"
                S[d] = pm.f12_from_fq2((pow(S[a][0][0], -1, Q), 0))
        assert S[0] == pm.final_exp(f)


def test_kzg_verdict_equals_the_g1_relation_of_a_known_tau():
    rng = random.Random(9)
    tau = rng.randrange(1, R)
    srs = skm.Srs(tau, 8)
    g2, tau_g2 = pm.G2, pm.g2_mul(pm.G2, tau)
    coeffs = [rng.randrange(R) for _ in range(5)]
    z = rng.randrange(R)
    pi, y = skm.kzg_prove(coeffs, z, srs)
    Cb = skm.mul_g(srs.commit_scalar(coeffs))
    pt = pm.g1_from_bytes
    two_pi = pm.g1_bytes(pm.g1_add(pt(pi), pt(pi)))
    c_plus_g = pm.g1_bytes(pm.g1_add(pt(Cb), pm.G1))
    cases = [(Cb, z, y, pi), (Cb, z, (y + 1) % R, pi), (Cb, z, y, two_pi), (c_plus_g, z, y, pi), (Cb, (z + 1) % R, y, pi), (c_plus_g, z, (y + 1) % R, pi),
             (Cb, z, y, skm.INF), (skm.mul_g(coeffs[0]), z, coeffs[0], skm.INF)]
    verdicts = []
    for (c, zz, yy, p) in cases:
        want = skm.kzg_verify(c, zz, yy, p, srs)
        assert pm.kzg_check(pt(c), zz, yy, pt(p), g2, tau_g2, pm.schedule_naf()) == want
        verdicts.append(want)
    assert verdicts == [True, False, False, False, False, True, False, True]
    tz, tzy = skm.kzg_prove(coeffs, tau, srs)                                         # z = tau
    assert skm.kzg_verify(Cb, tau, tzy, tz, srs) and pm.kzg_check(pt(Cb), tau, tzy, pt(tz), g2, tau_g2)
    assert not pm.kzg_check(pt(Cb), z, y, pt(pi), tau_g2, g2)                         # the two G2 points swapped
