"""Limb-exact model of the pairing's Fq12 layer (spartan-bn254_amd/csrc/pairing_kernels.cuh) on top of tests/fe_model.py.

Test infrastructure only.  f12_mul restates the device routine step by step — the operand table lanes 0..5 write, the three products each
of the 48 working lanes takes, cols_mac x 3 and cols_carry, the quad sum (low columns in 32-bit registers, the top column in 64 bits),
the one cols_reduce and fe_canon_small — and asserts at every step the range the header states for it (`Ranges` below).  fe_nine,
f12_frob and f12_conj are modelled the same way.  An Fq12 value is a list of 12 limb vectors: coefficient 2 i + part is part `part` of
the Fq2 coefficient of w^i, every one a canonical Montgomery representative (R = 2^261), as the kernel keeps them in LDS.

tests/test_f12_bounds_cpu.py ties this model to the big-integer product of tests/pairing_model.py; tests/test_gpu_f12_bounds.py ties the
device to both.
"""
from fractions import Fraction

import fe_model as fm
import pairing_model as pm

F = fm.FQ
P = F.p
NC = 2 * fm.NL - 1
SUM_BOUND, REDUCED_BOUND = 132, 2            # the header: a sum of 12 products is below 132 p^2, the reduction returns below 2p


class Ranges:
    """the largest unreduced sum (in p^2) and reduced value (in p) over every f12_mul the model ran"""

    def __init__(self):
        self.sum, self.reduced, self.products = Fraction(0), Fraction(0), 0

    def note(self, total, reduced):
        self.sum = max(self.sum, Fraction(total, P * P))
        self.reduced = max(self.reduced, Fraction(reduced, P))
        self.products += 1


def canonical(v):
    return fm.is_normalised(v) and 0 <= fm.to_int(v) < P


def fe_dbl_lazy(a):
    return [fm.i32(fm.u32(x) << 1) for x in a]


def fe_nine(a):
    """9 a of a normalised non-negative a, normalised: (a << 2) carried, doubled, plus a, carried"""
    t = fm.fe_normu([fm.i32(fm.u32(x) << 2) for x in a])
    return fm.fe_normu(fm.fe_add_lazy(fe_dbl_lazy(t), a))


def _entry(v, lo, hi, what):
    """a table entry: normalised, non-negative limbs, lo <= value <= hi"""
    assert fm.is_normalised(v) and fm.i32(v[fm.NL - 1]) >= 0, f"{what}: not normalised"
    assert lo <= fm.to_int(v) <= hi, f"{what}: {fm.to_int(v) / P:.4f} p outside [{lo / P:.0f} p, {hi / P:.0f} p]"
    return v


def table_rows(x, y):
    """what lane j writes for b_j = x + y u: row j = (x, y, 2p - y) and row 6 + j = (9x - y + 2p, x + 9y, 11p - (x + 9y))"""
    assert canonical(x) and canonical(y), "f12_mul: b is not canonical"
    nx, ny = fe_nine(x), fe_nine(y)
    assert fm.to_int(nx) == 9 * fm.to_int(x) and fm.to_int(ny) == 9 * fm.to_int(y) and fm.is_normalised(nx) and fm.is_normalised(ny)
    assert fm.pre_subb(F, 2, 1, nx, y)
    wx = fm.fe_normu(fm.fe_subb(F, 2, 1, nx, y))
    wy = fm.fe_normu(fm.fe_add_lazy(x, ny))
    assert fm.to_int(wy) < (11 - Fraction(1, 1000)) * P                                    # fe_negb<11>'s operand
    lo = [_entry(x, 0, P - 1, "b.c0"), _entry(y, 0, P - 1, "b.c1"), _entry(fm.fe_normu(fm.fe_negb(F, 2, y)), P + 1, 2 * P, "-b.c1")]
    hi = [_entry(wx, 0, 11 * P - 1, "(xi b).c0"), _entry(wy, 0, 10 * P - 1, "(xi b).c1"),
          _entry(fm.fe_normu(fm.fe_negb(F, 11, wy)), P + 1, 11 * P, "-(xi b).c1")]
    assert fm.to_int(lo[2]) == 2 * P - fm.to_int(y) and fm.to_int(wx) == 9 * fm.to_int(x) - fm.to_int(y) + 2 * P
    assert fm.to_int(wy) == fm.to_int(x) + 9 * fm.to_int(y) and fm.to_int(hi[2]) == 11 * P - fm.to_int(wy)
    return lo, hi


def operand_table(b):
    T = [None] * 36
    for j in range(6):
        lo, hi = table_rows(b[2 * j], b[2 * j + 1])
        T[3 * j:3 * j + 3] = lo
        T[3 * (6 + j):3 * (6 + j) + 3] = hi
    return T


def lane_products(q, r):
    """the three (coefficient of a, table index) pairs lane r of quad q = 2 k + part multiplies"""
    k, part = q >> 1, q & 1
    out = []
    for u in range(3):
        t = 3 * r + u
        i, h = t >> 1, t & 1
        j = k - i if i <= k else 12 + k - i
        sel = ((0 if h else 1) if part else (2 if h else 0))
        out.append((2 * i + h, 3 * j + sel))
    return out


def f12_mul(a, b, ranges=None):
    """S[dst] = S[a] * S[b] as the device computes it; the 12 canonical limb vectors of the result"""
    assert all(canonical(x) for x in a), "f12_mul: a is not canonical"
    T = operand_table(b)
    out = []
    for q in range(12):
        lanes = []
        for r in range(4):
            s = fm.cols_zero()
            for ai, ti in lane_products(q, r):
                fm.cols_mac(s, a[ai], T[ti])                                                # every column inside uint64 (asserted there)
            fm.cols_carry(s)
            assert all(c < 1 << 29 for c in s[:NC - 1]), "a carried column is not below 2^29"
            lanes.append(s)
        tot = []
        for c in range(NC - 1):                                                             # the 32-bit registers of the quad sum
            v = sum(s[c] for s in lanes)
            assert v < 1 << 32, f"quad sum of column {c} leaves 32 bits"
            tot.append(v & fm.U32)
        tot.append(fm._in(sum(s[NC - 1] for s in lanes), fm.U64, "quad sum of the top column"))
        total = sum(c << (fm.W * k) for k, c in enumerate(tot))
        assert total < SUM_BOUND * P * P, f"unreduced sum {total / P / P:.3f} p^2"
        red = fm.cols_reduce(F, tot)
        assert fm.pre_canon_small(F, red) and fm.to_int(red) >= 0, f"reduced value {fm.to_int(red) / P:.4f} p outside fe_canon_small's range"
        assert fm.to_int(red) * fm.RMONT < total + P * fm.RMONT and (fm.to_int(red) * fm.RMONT - total) % P == 0
        if ranges is not None:
            ranges.note(total, fm.to_int(red))
        out.append(fm.fe_canon_small(F, red))
    return out


# the rows f12_frob reads (pairing_consts.inc: SBN_PAIRING_FROB_ROWS), restated from the tower: row 2 i + part = (k0, k1) with
# output (i, part) = a_i.c0 k0 + a_i.c1 k1 for conj(a_i) g_i, g_i = xi^(i (q - 1) / 6)
def frob_rows():
    rows = []
    for i in range(6):
        g = pm.FROB_GAMMA[1][i]
        for k0, k1 in ((g[0], g[1]), (g[1], -g[0] % P)):
            rows.append((fm.from_int(F.mont(k0)), fm.from_int(F.mont(k1))))
    return rows


FROB_ROWS = frob_rows()


def f12_frob(a):
    """S[dst] = S[a]^q: two products and one reduction per output coefficient"""
    assert all(canonical(x) for x in a)
    out = []
    for lane in range(12):
        i = lane >> 1
        s = fm.cols_zero()
        fm.cols_mac(s, a[2 * i], FROB_ROWS[lane][0])
        fm.cols_mac(s, a[2 * i + 1], FROB_ROWS[lane][1])
        red = fm.cols_reduce(F, s)
        assert fm.pre_canon_small(F, red)
        out.append(fm.fe_canon_small(F, red))
    return out


def f12_conj(a):
    """S[dst] = S[a]^(q^6): the coefficients of odd powers of w negated"""
    assert all(canonical(x) for x in a)
    out = []
    for lane in range(12):
        v = list(a[lane])
        if (lane >> 1) & 1:
            v = fm.fe_norm([fm.i32(-x) for x in v])
            assert fm.pre_canon_small(F, v)
            v = fm.fe_canon_small(F, v)
        out.append(v)
    return out


# ---------------------------------------------------------------- between limb vectors and pairing_model's tuples
def to_f12(v):
    """12 limb vectors -> six Fq2 coefficients of plain integers (the representatives as they are: no Montgomery scaling)"""
    x = [fm.to_int(c) for c in v]
    return tuple((x[2 * i] % P, x[2 * i + 1] % P) for i in range(6))


def from_f12(f):
    return [fm.from_int(c) for pair in f for c in pair]


RINV = pow(fm.RMONT, -1, P)


def scale(f, k):
    return tuple((c[0] * k % P, c[1] * k % P) for c in f)


def exact_mul(a, b):
    """the canonical limbs of the Montgomery product of two Fq12 values given as Montgomery representatives: pairing_model's product by 2^-261"""
    return from_f12(scale(pm.f12_mul(to_f12(a), to_f12(b)), RINV))


# ---------------------------------------------------------------- the cases of f12_mul's range argument
TOP = P - 1


def fq12_of(coeffs):
    return [fm.from_int(c) for c in coeffs]


def range_top_pairs():
    """per output coefficient (k, part) the pair that maximises its unreduced sum: a all p - 1 (every table entry is non-negative, so the
    sum grows with every coefficient of a), and each b_j at the corner of {0, p - 1}^2 that maximises the two table entries its term
    takes (the entries are affine in b_j's parts, so a corner is the maximum; b_j enters through ONE table row, so the terms are
    independent)"""
    corners = [(x, y) for x in (0, TOP) for y in (0, TOP)]
    rows = {c: [[fm.to_int(e) for e in half] for half in table_rows(fm.from_int(c[0]), fm.from_int(c[1]))] for c in corners}
    pairs = []
    for k in range(6):
        for part in range(2):
            b = []
            for j in range(6):
                half = 0 if j <= k else 1                                                   # b_j itself, or xi b_j
                sels = (0, 2) if part == 0 else (1, 0)                                      # re: a0 B0 + a1 (-B1);  im: a0 B1 + a1 B0
                best = max(corners, key=lambda c: sum(rows[c][half][s] for s in sels))
                b += list(best)
            pairs.append((fq12_of([TOP] * 12), fq12_of(b)))
    return pairs


def edge_pairs():
    """[(name, a, b)]: the range tops, all p - 1, all zero, b = one, b a line whose coefficients are p - 1, single coefficients"""
    top, zero = fq12_of([TOP] * 12), fq12_of([0] * 12)
    one = fq12_of([F.mont(1)] + [0] * 11)
    line = fq12_of([TOP if i in (0, 2, 3, 6, 7) else 0 for i in range(12)])
    out = [("top(%d,%d)" % (i >> 1, i & 1), a, b) for i, (a, b) in enumerate(range_top_pairs())]
    out += [("all p-1", top, top), ("zero", zero, zero), ("zero a", zero, top), ("zero b", top, zero), ("b one", top, one), ("a one", one, top), ("b line", top, line)]
    for i in range(12):
        single = fq12_of([TOP if j == i else 0 for j in range(12)])
        out += [("single b %d" % i, top, single), ("single a %d" % i, single, top)]
    return out


def random_f12(rng):
    return fq12_of([rng.randrange(P) for _ in range(12)])
