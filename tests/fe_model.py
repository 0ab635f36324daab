"""Limb-exact model of the lazy field layer (spartan-bn254_amd/csrc/fp.cuh) in pure Python ints.

Test infrastructure only.  Each function mirrors one inline primitive instruction by instruction: 9 signed 29-bit limbs held as
int32 values (what the device's uint32 limbs mean as signed integers), 64-bit columns for the products.  Every column update
asserts that it stays inside int64 (fe_mul) or uint64 (fe_mulu, Cols), as the C code needs; limb-wise operations wrap at 32 bits
exactly as the C code does, so a test can see a limb that went negative or overflowed.  tests/test_gpu_fe_bounds.py pins this
model to the device bit for bit, and tests/test_fe_bounds_cpu.py uses it to check the range claims of fp.cuh and g1.cuh at the
edges of their value ranges.

Limbs are lists of 9 ints.  `Field` carries one modulus and the constant tables; FQ and FR are the two BN254 fields.
"""
import os
import re
from fractions import Fraction

import pyref

NL = 9
W = 29
MASK = (1 << W) - 1
U32 = (1 << 32) - 1
I64 = (-(1 << 63), (1 << 63) - 1)
U64 = (0, (1 << 64) - 1)
RMONT = 1 << (W * NL)                      # 2^261, the Montgomery radix of the device layer

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FP_CUH = os.path.join(ROOT, "spartan-bn254_amd", "csrc", "fp.cuh")


def i32(x):
    """x as the device reads a uint32 limb back as int32"""
    x &= U32
    return x - (1 << 32) if x >> 31 else x


def u32(x):
    return x & U32


def _in(v, rng, what):
    assert rng[0] <= v <= rng[1], f"{what}: column {v:#x} outside its 64-bit type"
    return v


# ---------------------------------------------------------------- limbs <-> integers
def to_int(v):
    """the value of a limb vector: sum (int32) v[k] 2^(29 k)"""
    return sum(i32(x) << (W * k) for k, x in enumerate(v))


def from_int(x):
    """the normalised limbs of x: limbs 0..7 in [0, 2^29), the signed rest in the top limb (x may be negative)"""
    v = []
    for _ in range(NL - 1):
        v.append(x & MASK)
        x >>= W
    assert -(1 << 31) <= x < (1 << 31), "top limb does not fit"
    v.append(x)
    return v


def is_normalised(v):
    return all(0 <= i32(x) <= MASK for x in v[:NL - 1])


def words_to_int(w):
    return sum((x & U32) << (32 * i) for i, x in enumerate(w[:8]))


def int_to_words(x):
    return [i32(x >> (32 * i)) for i in range(8)]


# ---------------------------------------------------------------- the two fields, constants parsed from fp.cuh
class Field:
    def __init__(self, name, p):
        self.name, self.p = name, p
        src = open(FP_CUH).read()
        body = re.search(r"struct %s \{(.*?)\n\};" % name, src, re.S).group(1)
        self.body = body
        self.P29 = self.table("P29")
        self.ONE29, self.R2_29 = self.table("ONE29"), self.table("R2_29")
        self.C256_29, self.CIN_29 = self.table("C256_29"), self.table("CIN_29")
        self.NINV29 = int(re.search(r"NINV29 = 0x([0-9a-fA-F]+)u", body).group(1), 16)
        self.PINV29 = (-self.NINV29) & MASK
        self.P8 = self.P29[8]

    def table(self, name):
        m = re.search(r"\b%s\[(\d+)\] = \{([^}]*)\}" % name, self.body)
        return [int(x, 16) for x in re.findall(r"0x([0-9a-fA-F]+)u", m.group(2))]

    def words(self):
        return [int(re.search(r"\bP%d = 0x([0-9a-fA-F]+)u" % i, self.body).group(1), 16) for i in range(8)]

    def mont(self, x):
        """x in the device's Montgomery domain: x 2^261 mod p"""
        return x * RMONT % self.p

    def unmont(self, x):
        return x * pow(RMONT, -1, self.p) % self.p


FQ = Field("FqP", pyref.P)
FR = Field("FrP", pyref.R)


# ---------------------------------------------------------------- limb-wise operations
def fe_norm(v):
    v = [i32(x) for x in v]
    for i in range(NL - 1):
        c = v[i] >> W
        v[i] &= MASK
        v[i + 1] = i32(v[i + 1] + c)
    return v


def fe_normu(v):
    v = [u32(x) for x in v]
    for i in range(NL - 1):
        c = v[i] >> W
        v[i] &= MASK
        v[i + 1] = u32(v[i + 1] + c)
    return [i32(x) for x in v]


def fe_add_lazy(a, b):
    return [i32(x + y) for x, y in zip(a, b)]


def fe_sub_lazy(a, b):
    return [i32(x - y) for x, y in zip(a, b)]


def fe_add(a, b):
    return fe_norm(fe_add_lazy(a, b))


def fe_sub(a, b):
    return fe_norm(fe_sub_lazy(a, b))


def fe_neg(a):
    return fe_norm([i32(-x) for x in a])


def fe_dbl(a):
    return fe_norm([i32(u32(x) << 1) for x in a])


# ---------------------------------------------------------------- the multipliers
def fe_mul_impl(F, a, b, sqr=False):
    """fe_mul_impl<M, SQR>: signed int64 columns"""
    a = [i32(x) for x in a]
    b = a if sqr else [i32(x) for x in b]
    a2 = [i32(u32(x) << 1) for x in a]
    c = [0] * NL
    for i in range(NL):
        for k in range(NL):
            has = True
            if not sqr:
                t = a[k] * b[i]
            elif k == i:
                t = a[k] * a[i]
            elif k > i:
                t = a2[k] * a[i]
            else:
                t, has = 0, False
            if i == 0 or k == NL - 1:
                c[k] = t if has else 0
            elif has:
                c[k] = _in(c[k] + t, I64, "fe_mul product")
        m = (u32(c[0]) * F.NINV29) & MASK
        for k in range(NL):
            c[k] = _in(c[k] + m * F.P29[k], I64, "fe_mul reduction")
        assert c[0] & MASK == 0
        c[1] = _in(c[1] + (c[0] >> W), I64, "fe_mul shift")
        c = c[1:] + [c[NL - 1]]
    r = [0] * NL
    for k in range(NL - 1):
        r[k] = c[k] & MASK
        carry = c[k] >> W
        if k < NL - 2:
            c[k + 1] = _in(c[k + 1] + carry, I64, "fe_mul carry")
        else:
            r[NL - 1] = i32(carry)
    return r


def fe_mulu_impl(F, a, b, sqr=False):
    """fe_mulu_impl<M, SQR>: unsigned uint64 columns (all limbs read as uint32)"""
    a = [u32(x) for x in a]
    b = a if sqr else [u32(x) for x in b]
    a2 = [u32(x << 1) for x in a]
    c = [0] * NL
    for i in range(NL):
        for k in range(NL):
            has = True
            if not sqr:
                t = a[k] * b[i]
            elif k == i:
                t = a[k] * a[i]
            elif k > i:
                t = a2[k] * a[i]
            else:
                t, has = 0, False
            if i == 0 or k == NL - 1:
                c[k] = t if has else 0
            elif has:
                c[k] = _in(c[k] + t, U64, "fe_mulu product")
        m = (u32(c[0]) * F.NINV29) & MASK
        for k in range(NL):
            c[k] = _in(c[k] + m * F.P29[k], U64, "fe_mulu reduction")
        assert c[0] & MASK == 0
        c[1] = _in(c[1] + (c[0] >> W), U64, "fe_mulu shift")
        c = c[1:] + [c[NL - 1]]
    r = [0] * NL
    for k in range(NL - 1):
        r[k] = c[k] & MASK
        carry = c[k] >> W
        if k < NL - 2:
            c[k + 1] = _in(c[k + 1] + carry, U64, "fe_mulu carry")
        else:
            r[NL - 1] = i32(carry)
    return r


def fe_mul(F, a, b):
    return fe_mul_impl(F, a, b)


def fe_sqr(F, a):
    return fe_mul_impl(F, a, a, True)


def fe_mulu(F, a, b):
    return fe_mulu_impl(F, a, b)


def fe_squ(F, a):
    return fe_mulu_impl(F, a, a, True)


# ---------------------------------------------------------------- Cols: sums of products with one reduction
def cols_zero():
    return [0] * (2 * NL - 1)


def cols_mac(s, a, b):
    for i in range(NL):
        for j in range(NL):
            s[i + j] = _in(s[i + j] + u32(a[i]) * u32(b[j]), U64, "cols_mac")


def cols_carry(s):
    for k in range(2 * NL - 2):
        s[k + 1] = _in(s[k + 1] + (s[k] >> W), U64, "cols_carry")
        s[k] &= MASK


def cols_reduce(F, s):
    s = list(s)
    for i in range(NL):
        m = (u32(s[i]) * F.NINV29) & MASK
        for k in range(NL):
            s[i + k] = _in(s[i + k] + m * F.P29[k], U64, "cols_reduce")
        assert s[i] & MASK == 0
        s[i + 1] = _in(s[i + 1] + (s[i] >> W), U64, "cols_reduce shift")
    r = [0] * NL
    for k in range(NL - 1):
        r[k] = s[NL + k] & MASK
        carry = s[NL + k] >> W
        if k < NL - 2:
            s[NL + k + 1] = _in(s[NL + k + 1] + carry, U64, "cols_reduce carry")
        else:
            r[NL - 1] = i32(carry)
    return r


# ---------------------------------------------------------------- canonicalisation, zero tests
def fe_reduce(F, a):
    return fe_mul(F, a, F.ONE29)


def fe_canon_small(F, x):
    x = [i32(v) for v in x]
    neg = U32 if x[NL - 1] < 0 else 0
    x = fe_norm([i32(x[k] + (F.P29[k] & neg)) for k in range(NL)])
    y = fe_norm([i32(x[k] - F.P29[k]) for k in range(NL)])
    keep = U32 if y[NL - 1] < 0 else 0
    return [i32((u32(x[k]) & keep) | (u32(y[k]) & ~keep & U32)) for k in range(NL)]


def fe_canon(F, a):
    return fe_canon_small(F, fe_reduce(F, a))


def fe_is_zero(F, a):
    return all(x == 0 for x in fe_canon(F, a))


def fe_eq(F, a, b):
    return fe_is_zero(F, fe_sub_lazy(fe_norm(a), fe_norm(b)))


def fe_maybe_zero(F, d):
    k = (u32(u32(d[0]) * F.PINV29) + 8) & MASK
    return k <= 16


# ---------------------------------------------------------------- the unsigned fast path: inflated multiples of p
def kp29(F, K, k):
    carry = t = 0
    for i in range(k + 1):
        t = K * F.P29[i] + carry
        carry = t >> W
    return u32(t) if k == NL - 1 else t & MASK


def bias29(F, K, J, k):
    if k == NL - 1:
        return u32(kp29(F, K, k) - J)
    return u32(kp29(F, K, k) + (J << W) - (J if k > 0 else 0))


def bias(F, K, J):
    return [bias29(F, K, J, k) for k in range(NL)]


def fe_subb(F, K, J, a, b):
    return [i32(u32(a[i] - b[i]) + bias29(F, K, J, i)) for i in range(NL)]


def fe_negb(F, K, b):
    return [i32(bias29(F, K, 1, i) - b[i]) for i in range(NL)]


# ---------------------------------------------------------------- fix-ups before a store
def fe_fix_nonneg(F, K, x):
    neg = U32 if i32(x[NL - 1]) < 0 else 0
    return fe_norm([i32(x[k] + (kp29(F, K, k) & neg)) for k in range(NL)])


def fe_fix_tab(F, x):
    P8 = F.P8
    top = i32(x[NL - 1])
    m1 = U32 if top < 0 else 0
    m2 = U32 if top + P8 < 0 else 0
    m3 = U32 if 2 * P8 + 1 - top < 0 else 0
    return fe_norm([i32(x[k] + (F.P29[k] & m1) + (F.P29[k] & m2) - ((2 * F.P29[k]) & m3)) for k in range(NL)])


def fe_is_canonical(F, w):
    return words_to_int(w) < F.p


# ---------------------------------------------------------------- preconditions, restating fp.cuh's comments
def pre_mul(a, b):
    """fe_mul: signed columns, 9 |a_k| |b_j| + 9 2^58 < 2^63"""
    ma, mb = max(abs(i32(x)) for x in a), max(abs(i32(x)) for x in b)
    return 9 * ma * mb + 9 * (1 << 58) < 1 << 63


def pre_sqr(a):
    return all(abs(i32(x)) < 1 << 29 for x in a)


def pre_mulu(a, b):
    """fe_mulu: non-negative limbs, 9 |a_k| |b_j| + 9 2^58 < 2^64"""
    if any(i32(x) < 0 for x in a + b):
        return False
    return 9 * max(a) * max(b) + 9 * (1 << 58) < 1 << 64


def pre_squ(a):
    return all(0 <= i32(x) < 1 << 30 for x in a)


def pre_subb(F, K, J, a, b):
    """fe_subb<K, J>: a normalised and non-negative; b the sum of up to J normalised non-negative values, below (K - 0.001) p"""
    if not (is_normalised(a) and to_int(a) >= 0):
        return False
    return all(0 <= i32(x) <= J * MASK for x in b[:NL - 1]) and 0 <= to_int(b) < (K - Fraction(1, 1000)) * F.p


REDUCE_TIGHT, REDUCE_WIDE = 13, 448


def pre_reduce(F, a, wide=False):
    """fe_reduce / fe_canon / fe_store / fe_is_zero, both lines of fp.cuh's contract.
    tight: |a| < 13 p -> (-0.1p, 1.1p).  wide: |a| < 448 p -> (-0.76p, 1.76p), still inside fe_canon_small's (-p, 2p).
    Either way the limbs must fit fe_mul's signed columns against ONE29 (a normalised value below 451 p does)."""
    return abs(to_int(a)) < (REDUCE_WIDE if wide else REDUCE_TIGHT) * F.p and pre_mul(a, F.ONE29)


def reduce_interval(F, a):
    """the interval fe_reduce(a) must land in, from the arithmetic alone: (a ONE + m p) / 2^261 with 0 <= m < 2^261"""
    lo = Fraction(to_int(a) * to_int(F.ONE29), RMONT)
    return lo, lo + F.p


def pre_canon_small(F, x):
    return is_normalised(x) and -F.p < to_int(x) < 2 * F.p


def pre_fix_tab(F, x):
    return is_normalised(x) and -2 * F.p < to_int(x) < Fraction(9, 2) * F.p


def pre_fix_nonneg(F, K, x):
    return is_normalised(x) and -K * F.p < to_int(x) < (1 << 256) - K * F.p


def pre_maybe_zero(F, d):
    return abs(to_int(d)) <= 8 * F.p          # k p with |k| <= 8


# ---------------------------------------------------------------- adversarial representatives
def rep_at(F, x, k):
    """the normalised limbs of x + k p (the residue of x at the k-th multiple of p)"""
    return from_int(x + k * F.p)


def top_at(F, top, low):
    """a normalised value whose top limb is `top` and whose lower 8 limbs all equal `low` (0 or 2^29 - 1 are the extremes)"""
    return [low] * (NL - 1) + [top]


def unnormalised(x, rng, lo=-(1 << 29), hi=1 << 29):
    """a non-normalised representation of the integer x: random limbs 0..7 in [lo, hi), the top limb takes the rest"""
    v = [rng.randrange(lo, hi) for _ in range(NL - 1)]
    rest = x - sum(v[k] << (W * k) for k in range(NL - 1))
    low = rest & ((1 << (W * (NL - 1))) - 1)
    for k in range(NL - 1):
        v[k] += (low >> (W * k)) & MASK
    top = (rest - low) >> (W * (NL - 1))
    v = v + [top]
    assert to_int(v) == x
    return [i32(t) for t in v]


# ---------------------------------------------------------------- g1.cuh, composed from the primitives above (Fq only)
# A point is a tuple of limb vectors (X, Y, ZZ, ZZZ); an affine point (x, y).  Infinity: ZZ all zero limbs / x = y = 0.
ONE_Q = FQ.ONE29
ZERO = [0] * NL


def is_zero_limbs(v):
    return all(x == 0 for x in v)


def xyzz_inf():
    return (ZERO, ZERO, ZERO, ZERO)


def xyzz_dbl_affine(x, y):
    F = FQ
    U = fe_dbl(y); V = fe_sqr(F, U); Wv = fe_mul(F, U, V); S = fe_mul(F, x, V)
    xx = fe_sqr(F, x); M3 = fe_add(fe_dbl(xx), xx)
    X = fe_sub(fe_sub(fe_sqr(F, M3), S), S)
    Y = fe_sub(fe_mul(F, M3, fe_sub(S, X)), fe_mul(F, Wv, y))
    return (fe_fix_nonneg(F, 4, X), fe_fix_nonneg(F, 2, Y), fe_fix_nonneg(F, 1, V), fe_fix_nonneg(F, 1, Wv)), (X, Y)


def xyzz_dbl(p):
    """returns (point, (X, Y) before the fix-ups: the signed values the comment bounds)"""
    F = FQ
    if is_zero_limbs(p[2]):
        return p, None
    U = fe_dbl(p[1]); V = fe_sqr(F, U); Wv = fe_mul(F, U, V); S = fe_mul(F, p[0], V)
    xx = fe_sqr(F, p[0]); M3 = fe_add(fe_dbl(xx), xx)
    X = fe_sub(fe_sub(fe_sqr(F, M3), S), S)
    Y = fe_sub(fe_mul(F, M3, fe_sub(S, X)), fe_mul(F, Wv, p[1]))
    return (fe_fix_nonneg(F, 4, X), fe_fix_nonneg(F, 2, Y), fe_fix_nonneg(F, 1, fe_mul(F, V, p[2])),
            fe_fix_nonneg(F, 1, fe_mul(F, Wv, p[3]))), (X, Y)


def xyzz_madd(acc, q, neg, trace=None):
    """acc + q (acc - q when neg); `trace`, if a dict, receives the intermediate values the comments bound"""
    F = FQ
    qx, qy0 = q
    if (qx[0] | qy0[0]) == 0 and is_zero_limbs(qx) and is_zero_limbs(qy0):
        return acc
    qy = fe_negb(F, 2, qy0) if neg else qy0
    X, Y, ZZ, ZZZ = acc
    if ZZ[0] == 0 and is_zero_limbs(ZZ):
        return (qx, fe_normu(qy), ONE_Q, ONE_Q)
    U2, S2 = fe_mulu(F, qx, ZZ), fe_mulu(F, qy, ZZZ)
    P = fe_normu(fe_subb(F, 6, 1, U2, X))
    R = fe_normu(fe_subb(F, 4, 1, S2, Y))
    if trace is not None:
        trace.update(U2=U2, S2=S2, P=P, R=R, qy=qy)
    if fe_maybe_zero(F, P) and fe_is_zero(F, P):
        if fe_is_zero(F, R):
            return xyzz_dbl_affine(qx, fe_normu(qy))[0]
        return xyzz_inf()
    PP = fe_squ(F, P); PPP = fe_mulu(F, P, PP); Q = fe_mulu(F, X, PP)
    RR = fe_squ(F, R)
    X3 = fe_normu(fe_subb(F, 4, 3, RR, fe_add_lazy(fe_add_lazy(PPP, Q), Q)))
    t1, t2 = fe_subb(F, 6, 1, Q, X3), fe_negb(F, 4, Y)
    cy = cols_zero()
    cols_mac(cy, R, t1)
    cols_mac(cy, PPP, t2)
    if trace is not None:
        trace.update(PP=PP, PPP=PPP, Q=Q, RR=RR, X3=X3, t1=t1, t2=t2)
    return (X3, cols_reduce(F, cy), fe_mulu(F, ZZ, PP), fe_mulu(F, ZZZ, PPP))


def xyzz_add_inl(a, b, trace=None):
    F = FQ
    if is_zero_limbs(a[2]):
        return b
    if is_zero_limbs(b[2]):
        return a
    U1, U2 = fe_mulu(F, a[0], b[2]), fe_mulu(F, b[0], a[2])
    S1, S2 = fe_mulu(F, a[1], b[3]), fe_mulu(F, b[1], a[3])
    P = fe_normu(fe_subb(F, 2, 1, U2, U1)); R = fe_normu(fe_subb(F, 2, 1, S2, S1))
    if trace is not None:
        trace.update(U1=U1, U2=U2, S1=S1, S2=S2, P=P, R=R)
    if fe_maybe_zero(F, P) and fe_is_zero(F, P):
        if fe_is_zero(F, R):
            return xyzz_dbl(a)[0]
        return xyzz_inf()
    PP = fe_squ(F, P); PPP = fe_mulu(F, P, PP); Q = fe_mulu(F, U1, PP)
    X3 = fe_normu(fe_subb(F, 4, 3, fe_squ(F, R), fe_add_lazy(fe_add_lazy(PPP, Q), Q)))
    t1, t2 = fe_subb(F, 6, 1, Q, X3), fe_negb(F, 2, S1)
    cy = cols_zero()
    cols_mac(cy, R, t1)
    cols_mac(cy, PPP, t2)
    if trace is not None:
        trace.update(PP=PP, PPP=PPP, Q=Q, X3=X3, t1=t1, t2=t2)
    return (X3, cols_reduce(F, cy), fe_mulu(F, fe_mulu(F, a[2], b[2]), PP), fe_mulu(F, fe_mulu(F, a[3], b[3]), PPP))


def xyzz_add_quad_y(a, b):
    """the quad form's Y3 (T1 - T2 + 2p, normalised): the one coordinate it computes differently from xyzz_add_inl"""
    F = FQ
    U1, U2 = fe_mulu(F, a[0], b[2]), fe_mulu(F, b[0], a[2])
    S1, S2 = fe_mulu(F, a[1], b[3]), fe_mulu(F, b[1], a[3])
    P = fe_normu(fe_subb(F, 2, 1, U2, U1)); R = fe_normu(fe_subb(F, 2, 1, S2, S1))
    PP = fe_squ(F, P); PPP = fe_mulu(F, P, PP); Q = fe_mulu(F, U1, PP)
    X3 = fe_normu(fe_subb(F, 4, 3, fe_mulu(F, R, R), fe_add_lazy(fe_add_lazy(PPP, Q), Q)))
    T1, T2 = fe_mulu(F, R, fe_subb(F, 6, 1, Q, X3)), fe_mulu(F, S1, PPP)
    return fe_normu(fe_subb(F, 2, 1, T1, T2))


def xyzz_store_load(p):
    """xyzz_store -> xyzz_load: the fix-ups, then the stored 256-bit integers read back as normalised limbs"""
    F = FQ
    out = []
    for v, K in zip(p, (4, 2, 1, 1)):
        x = to_int(fe_fix_nonneg(F, K, fe_norm(v)))
        assert 0 <= x < 1 << 256, "xyzz_store: a coordinate outside [0, 2^256)"
        out.append(from_int(x))
    return tuple(out)


def xyzz_affine(p):
    """the affine point (plain integers) of a device XYZZ point whose coordinates are in the Montgomery domain; None = infinity"""
    F = FQ
    if is_zero_limbs(p[2]):
        return None
    X, Y, ZZ, ZZZ = (F.unmont(to_int(v) % F.p) for v in p)
    return (X * pow(ZZ, -1, F.p) % F.p, Y * pow(ZZZ, -1, F.p) % F.p)


# ---------------------------------------------------------------- G1 test points at the edges of the XYZZ ranges
RANGES = {"X": 5.2, "Y": 3.2, "ZZ": 1.2, "ZZZ": 1.2}        # g1.cuh: X in [0, 5.2p), Y in [0, 3.2p), ZZ, ZZZ in [0, 1.2p)


def at_top(F, x, lim):
    """the largest representative x + k p (k >= 0) of a residue x in [0, p) that stays below lim * p"""
    k = int((lim * F.p - 1 - x) // F.p)
    while x + k * F.p >= lim * F.p:
        k -= 1
    return x + k * F.p


def xyzz_of(pt, lam, top=True):
    """the device XYZZ limbs of an affine point (plain ints; None = infinity) scaled by lam into (lam^2 x, lam^3 y, lam^2, lam^3),
    in the Montgomery domain, each coordinate moved to the top of its range (top=True) or left canonical"""
    F = FQ
    if pt is None:
        return xyzz_inf()
    vals = [lam * lam * pt[0], lam ** 3 * pt[1], lam * lam, lam ** 3]
    out = []
    for v, lim in zip(vals, RANGES.values()):
        v = F.mont(v % F.p)
        out.append(from_int(at_top(F, v, lim) if top else v))
    return tuple(out)


def affine_of(pt):
    """canonical Montgomery affine limbs (what the tables hold); infinity = (0, 0)"""
    if pt is None:
        return (ZERO, ZERO)
    return (from_int(FQ.mont(pt[0])), from_int(FQ.mont(pt[1])))


def ratio(F, v):
    """value / p as a float (for the range statistics)"""
    return to_int(v) / F.p
