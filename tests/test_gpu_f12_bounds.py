"""GPU: the pairing's Fq12 layer (csrc/pairing_kernels.cuh: fe_nine, fe_negb<11>, f12_mul, f12_frob, f12_conj, f12_inv_fq, f12_final_exp) at
the edges of its value ranges, through the probe library (harness/fe_probe.hip: the shipped routines, one 64-lane block per case over an LDS
image of the kernel's size, raw 9-limb I/O).

Every output is compared limb for limb with the canonical limbs of the exact result of tests/pairing_model.py; there is no tolerance.  For
f12_mul and f12_frob the edge cases also run through the limb-exact model tests/f12_model.py, which asserts the header's ranges on the way and
which tests/test_f12_bounds_cpu.py ties to the same exact results.  f12_mul runs under every slot pattern k_pairing_products uses (all
distinct, the Miller step, the squaring, dst == b, a == b != dst) and the operands that are not the destination must come back unchanged.
The last test feeds sbn_pairing_products G1 points whose coordinates lie at the ends of [0, p)."""
import ctypes
import functools
import os
import random
import subprocess

import pytest

from conftest import golden
from test_gpu_fe_bounds import PKG_DIR, SO, Probe
import f12_model as f12
import fe_model as fm
import pairing_model as pm

pytestmark = pytest.mark.gpu
F, P = fm.FQ, fm.FQ.p
N_RANDOM = 1 << 12
KAT = golden("pairing_kat.json")
KAT_CASES = {c["name"]: c for c in KAT["cases"]}
# f12_mul's placement selectors (fe_probe.hip): name -> (selector, b is a, a comes back, b comes back)
PATTERNS = {"distinct": (0, False, True, True), "miller_step": (1, False, False, True), "squaring": (2, True, False, False),
            "dst_is_b": (3, False, True, False), "a_is_b": (4, True, True, True)}


@pytest.fixture(scope="module")
def probe():
    if not os.path.exists(SO):
        subprocess.run(["make", "-s", "-C", PKG_DIR, "libsbn_fe_probe.so"], check=True)
    return Probe(ctypes.CDLL(SO))


def sel_elem(sel):
    return [[sel] + [0] * (fm.NL - 1)]


def mont12(f):
    """six Fq2 coefficients (values) -> the 12 canonical limb vectors the kernel holds"""
    return [fm.from_int(F.mont(c)) for pair in f for c in pair]


def unmont12(v):
    return f12.scale(f12.to_f12(v), f12.RINV)


# ---------------------------------------------------------------- f12_mul
@functools.lru_cache(maxsize=None)
def mul_cases():
    """[(name, a, b, a * b, a * a)]: the edge pairs of the range argument (results from the limb model, which asserts the ranges, and equal to
    the exact ones), then the random pairs (exact results)"""
    rng = random.Random(1212)
    out, squares = [], {}
    for name, a, b in f12.edge_pairs():
        key = tuple(map(tuple, a))
        if key not in squares:
            squares[key] = f12.f12_mul(a, a)
            assert squares[key] == f12.exact_mul(a, a)
        ab = f12.f12_mul(a, b)
        assert ab == f12.exact_mul(a, b)
        out.append((name, a, b, ab, squares[key]))
    for i in range(N_RANDOM):
        a, b = f12.random_f12(rng), f12.random_f12(rng)
        out.append(("random %d" % i, a, b, f12.exact_mul(a, b), f12.exact_mul(a, a)))
    return out


@pytest.mark.parametrize("pattern", list(PATTERNS))
def test_f12_mul(probe, pattern):
    sel, square, a_back, b_back = PATTERNS[pattern]
    cases = mul_cases()
    assert len(cases) >= 12 + N_RANDOM
    got = probe.run("f12_mul", F, [a + b + sel_elem(sel) for _, a, b, _, _ in cases])
    bad = []
    for (name, a, b, ab, aa), o in zip(cases, got):
        res, ra, rb = o[0][:12], o[0][12:24], o[0][24:]
        want = aa if square else ab
        if res != want:
            bad.append((name, "result", [i for i in range(12) if res[i] != want[i]]))
        if a_back and ra != a:
            bad.append((name, "a changed"))
        if b_back and rb != (a if square else b):
            bad.append((name, "b changed"))
    assert not bad, f"f12_mul, {pattern}: {len(bad)} findings in {len(cases)} cases, first: {bad[:3]}"


# ---------------------------------------------------------------- Frobenius, conjugate, the inversion in Fq
def unary_values(rng, n_random):
    vals = [f12.fq12_of([c] * 12) for c in (0, 1, P - 1)]
    vals += [f12.fq12_of([rng.choice((0, 1, P - 1)) for _ in range(12)]) for _ in range(61)]
    return vals + [f12.random_f12(rng) for _ in range(n_random)]


def run_unary(probe, op, vals, want, modes=(0, 1)):
    for sel in modes:                                                     # 0: dst != a (a must come back unchanged), 1: dst == a
        got = probe.run(op, F, [a + sel_elem(sel) for a in vals])
        bad = [(i, "result") for i, (o, w) in enumerate(zip(got, want)) if o[0][:12] != w]
        if sel == 0:
            bad += [(i, "a changed") for i, (o, a) in enumerate(zip(got, vals)) if o[0][12:] != a]
        assert not bad, f"{op}, dst {'==' if sel else '!='} a: {len(bad)} findings in {len(vals)} cases, first: {bad[:3]} {vals[bad[0][0]]}"


def test_f12_frob(probe):
    vals = unary_values(random.Random(77), N_RANDOM)
    want = [f12.from_f12(pm.f12_frobenius(f12.to_f12(a))) for a in vals]          # Fq-linear: the representatives map like the values
    for a, w in zip(vals[:96], want):
        assert f12.f12_frob(a) == w
    run_unary(probe, "f12_frob", vals, want)
    x = vals[:128]
    for _ in range(12):
        x = [o[0][:12] for o in probe.run("f12_frob", F, [a + sel_elem(1) for a in x])]
    assert x == vals[:128], "twelve Frobenius maps are not the identity"


def test_f12_conj(probe):
    vals = unary_values(random.Random(78), 512)
    want = [f12.from_f12(pm.f12_conj(f12.to_f12(a))) for a in vals]
    assert all(f12.f12_conj(a) == w for a, w in zip(vals, want))
    zero = [0] * fm.NL
    assert all(w[i] == zero for a, w in zip(vals, want) for i in range(12) if a[i] == zero) and any(a[3] == zero for a in vals)
    run_unary(probe, "f12_conj", vals, want)


def test_f12_inv_fq(probe):
    """x as a value and as a representative at 0, 1, 2, p - 1, p - 2, then random; the other eleven coefficients of the operand are not read"""
    rng = random.Random(79)
    reps = [0, 1, 2, P - 1, P - 2] + [F.mont(x) for x in (1, 2, P - 1, P - 2)] + [rng.randrange(P) for _ in range(247)]
    vals = [f12.fq12_of([r] + [rng.randrange(P) for _ in range(11)]) for r in reps]
    want = [f12.fq12_of([F.mont(pow(F.unmont(r), P - 2, P))] + [0] * 11) for r in reps]
    assert want[0][0] == [0] * fm.NL and want[5] == f12.fq12_of([F.mont(1)] + [0] * 11)
    run_unary(probe, "f12_inv_fq", vals, want)


# ---------------------------------------------------------------- the two field helpers only the pairing uses
def test_fe_nine(probe):
    rng = random.Random(80)
    xs = [0, 1, P - 1, (1 << 29) - 1, (1 << 232) - 1] + [rng.randrange(P) for _ in range(N_RANDOM)]
    got = probe.run("nine", F, [[fm.from_int(x)] for x in xs])
    for x, o in zip(xs, got):
        assert o[0][0] == fm.from_int(9 * x) == f12.fe_nine(fm.from_int(x)), f"fe_nine({x:#x})"


def test_negb_11(probe):
    rng = random.Random(81)
    xs = [0, 1, P - 1, P, 10 * P - 1] + [rng.randrange(10 * P) for _ in range(N_RANDOM)]
    got = probe.run("negb_11", F, [[fm.from_int(x)] for x in xs])
    for x, o in zip(xs, got):
        v = o[0][0]
        assert v == fm.fe_negb(F, 11, fm.from_int(x)), f"fe_negb<11>({x:#x})"
        assert all(0 <= limb < 1 << 31 for limb in v) and fm.to_int(v) == 11 * P - x


# ---------------------------------------------------------------- the final exponentiation's program
def parse_gt(b):
    """the inverse of pairing_model.gt_bytes"""
    c = [int.from_bytes(b[32 * i:32 * i + 32], "little") for i in range(12)]
    f, k = [None] * 6, 0
    for h in (0, 1):
        for m in (0, 1, 2):
            f[2 * m + h] = (c[k], c[k + 1])
            k += 2
    return tuple(f)


def test_f12_final_exp(probe):
    """against the literal power by (q^12 - 1)/r.  Zero is left out: it is not a value a Miller product can take (every line and every square
    of a non-zero value is non-zero in the field Fq12), and the model has no answer for it (the program divides by the norm)."""
    rng = random.Random(82)
    term = KAT_CASES["pair1"]["terms"][0]
    g2 = _g2(bytes.fromhex(KAT["g2"][term[1]]))
    miller = pm.miller(pm.g1_from_bytes(bytes.fromhex(term[0])), pm.line_table(g2, pm.schedule_naf()))
    gt = parse_gt(bytes.fromhex(KAT_CASES["gen"]["gt"]))
    assert pm.gt_bytes(gt).hex() == KAT_CASES["gen"]["gt"] and gt != pm.F12_ONE
    r = lambda: rng.randrange(1, P)
    in_fq6 = tuple((r(), r()) if i % 2 == 0 else pm.F2_ZERO for i in range(6))
    ones = [pm.F12_ONE, pm.f12_from_fq2((r(), 0)), pm.f12_from_fq2((r(), r())), in_fq6, pm.f12_from_fq2((P - 1, 0))]       # a proper subfield, and -1
    vals = [mont12(f) for f in ones + [miller, gt]] + [f12.fq12_of([P - 1] * 12)] + [f12.random_f12(rng) for _ in range(3)]
    want = [mont12(pm.final_exp(unmont12(v))) for v in vals]
    assert all(w == mont12(pm.F12_ONE) for w in want[:len(ones)]) and want[5] == mont12(parse_gt(bytes.fromhex(KAT_CASES["pair1"]["gt"])))
    assert want[6] == mont12(pm.f12_pow(gt, pm.FINAL_EXPONENT)) and want[6] != mont12(pm.F12_ONE)
    got = probe.run("f12_final_exp", F, vals)
    bad = [i for i, (o, w) in enumerate(zip(got, want)) if o[0] != w]
    assert not bad, f"f12_final_exp: cases {bad} of {len(vals)} differ from the literal power"


# ---------------------------------------------------------------- through the public ABI: G1 coordinates at the ends of [0, p)
def _g2(b):
    c = [int.from_bytes(b[32 * i:32 * i + 32], "little") for i in range(4)]
    return ((c[0], c[1]), (c[2], c[3]))


def g1_with_x_from(start, step):
    """the curve point whose x is the first from `start` in direction `step` for which x^3 + 3 is a square (q = 3 mod 4: one power finds the
    root); G1 has cofactor 1, so every curve point is a legal input"""
    x = start
    while True:
        rhs = (x * x * x + 3) % P
        y = pow(rhs, (P + 1) // 4, P)
        if y * y % P == rhs:
            return (x, y)
        x += step


def test_pairing_products_with_g1_coordinates_at_the_ends_of_the_range(ctx):
    lo, hi = g1_with_x_from(0, 1), g1_with_x_from(P - 1, -1)
    assert lo[0] < 8 and P - hi[0] < 8
    pts = [lo, pm.g1_neg(lo), hi, pm.g1_neg(hi)]
    names = ["s1", "s1", "tau", "tau"]
    qs = {n: _g2(bytes.fromhex(KAT["g2"][n])) for n in set(names)}
    hs = {n: ctx.g2_prepare(bytes.fromhex(KAT["g2"][n])) for n in set(names)}
    try:
        checks = [[(p, n)] for p, n in zip(pts, names)] + [list(zip(pts, names))]
        want = [pm.pairing_product([(p, qs[n]) for p, n in terms]) for terms in checks]
        assert want[4] == pm.F12_ONE and all(w != pm.F12_ONE for w in want[:4]) and pm.f12_mul(want[0], want[1]) == pm.F12_ONE
        p_bytes = b"".join(pm.g1_bytes(p) for terms in checks for p, _ in terms)
        one, gt = ctx.pairing_products(p_bytes, [hs[n] for terms in checks for _, n in terms], [len(t) for t in checks])
        assert [g.hex() for g in gt] == [pm.gt_bytes(w).hex() for w in want]
        assert list(one) == [0, 0, 0, 0, 1]
    finally:
        for h in hs.values():
            h.free()
