"""CPU: the range argument of f12_mul (csrc/pairing_kernels.cuh) on the limb-exact model tests/f12_model.py.

The model asserts every range the header states while it runs (64-bit per-lane columns, carried columns below 2^29, 32-bit quad sums, the
table entries' ranges, fe_canon_small's (-p, 2p)); this test runs it over the operands that maximise each output coefficient's unreduced
sum, the other edge operands and a random batch, and requires of every case the big-integer product of tests/pairing_model.py, scaled by
2^-261 (the operands are Montgomery representatives), coefficient by coefficient.  It prints the largest unreduced sum in p^2 and the
largest reduced value in p: the maximisers are among the cases, so the maxima are the true ones over canonical operands."""
import random
from fractions import Fraction

import pytest

import f12_model as f12
import fe_model as fm
import pairing_model as pm

P = f12.P
N_RANDOM = 48


@pytest.fixture(scope="module")
def ranges():
    r = f12.Ranges()
    yield r
    if r.products:
        print(f"\nf12_mul over {r.products} reductions: largest unreduced sum {float(r.sum):.4f} p^2 of {f12.SUM_BOUND} p^2, "
              f"largest reduced value {float(r.reduced):.4f} p of {f12.REDUCED_BOUND} p")


def check(a, b, ranges, name):
    got = f12.f12_mul(a, b, ranges)
    assert all(f12.canonical(c) for c in got), name
    assert got == f12.exact_mul(a, b), name


def test_range_tops_edges_and_the_stated_bounds(ranges):
    cases = f12.edge_pairs()
    assert [n for n, _, _ in cases[:12]] == ["top(%d,%d)" % (k, part) for k in range(6) for part in range(2)]
    for name, a, b in cases:
        check(a, b, ranges, name)
    assert ranges.sum == Fraction((P - 1) * ((3 * P - 1) + 5 * (21 * P - 8)), P * P), "the largest sum is output (0, re) of its maximiser"
    print(f"\nrange tops: unreduced sum {float(ranges.sum):.4f} p^2 (stated: below {f12.SUM_BOUND}), reduced {float(ranges.reduced):.4f} p (stated: below {f12.REDUCED_BOUND})")
    assert ranges.sum < f12.SUM_BOUND and ranges.reduced < f12.REDUCED_BOUND


def test_the_range_tops_are_the_maxima_of_their_sums():
    """output (k, part) of the k-th maximiser is at least the same output's sum for every other corner assignment of b tried at random,
    and the closed form of the largest one: k = 0, real part: (3p - 1) + 5 (21p - 8) times p - 1"""
    rng = random.Random(12)
    pairs = f12.range_top_pairs()

    def sums(a, b):
        T = [fm.to_int(e) for e in f12.operand_table(b)]
        A = [fm.to_int(x) for x in a]
        return [sum(A[ai] * T[ti] for r in range(4) for ai, ti in f12.lane_products(q, r)) for q in range(12)]

    tops = [sums(a, b)[q] for q, (a, b) in enumerate(pairs)]
    assert max(tops) == tops[0] == (P - 1) * ((3 * P - 1) + 5 * (21 * P - 8))
    for _ in range(64):
        b = f12.fq12_of([rng.choice((0, P - 1, rng.randrange(P))) for _ in range(12)])
        a = f12.fq12_of([rng.choice((P - 1, rng.randrange(P))) for _ in range(12)])
        assert all(s <= t for s, t in zip(sums(a, b), tops))


def test_every_product_is_dealt_to_one_lane():
    """the 48 lanes' three products are the 144 terms of c_k = sum_{i <= k} a_i b_(k-i) + sum_{i > k} a_i (xi b)_(k+6-i)"""
    for q in range(12):
        k, part = q >> 1, q & 1
        got = sorted(t for r in range(4) for t in f12.lane_products(q, r))
        want = []
        for i in range(6):
            row = k - i if i <= k else 12 + k - i
            want += [(2 * i, 3 * row + (1 if part else 0)), (2 * i + 1, 3 * row + (0 if part else 2))]
        assert got == sorted(want) and len(set(got)) == 12


def test_random_batch(ranges):
    rng = random.Random(2261)
    for i in range(N_RANDOM):
        a, b = f12.random_f12(rng), f12.random_f12(rng)
        check(a, b if i % 4 else a, ranges, f"random {i}")
    assert ranges.sum < f12.SUM_BOUND and ranges.reduced < f12.REDUCED_BOUND


def test_fe_nine():
    rng = random.Random(9)
    for x in [0, 1, P - 1, (1 << 29) - 1, 1 << 252] + [rng.randrange(P) for _ in range(256)]:
        v = f12.fe_nine(fm.from_int(x))
        assert v == fm.from_int(9 * x)


def test_frobenius_and_conjugate_models():
    rng = random.Random(6)
    vals = [f12.fq12_of([c] * 12) for c in (0, 1, P - 1)] + [f12.fq12_of([rng.choice((0, 1, P - 1)) for _ in range(12)]) for _ in range(32)]
    vals += [f12.random_f12(rng) for _ in range(32)]
    for a in vals:
        assert f12.f12_frob(a) == f12.from_f12(pm.f12_frobenius(f12.to_f12(a))), "the Frobenius is Fq-linear: no Montgomery factor"
        assert f12.f12_conj(a) == f12.from_f12(pm.f12_conj(f12.to_f12(a)))
        x = a
        for _ in range(12):
            x = f12.f12_frob(x)
        assert x == a
