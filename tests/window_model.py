"""Plain-integer model of the signed-window recoding every MSM / commitment path branches on (msm_host.hpp: make_shape;
msm_kernels.cuh: window_digit, window_digit_indep), and the scalars that sit on its seams for a given window width c.

Two recodings of k = sum_w d_w 2^(c w):
  sequential   (window_digit):        d = raw + carry_in; d >= 2^(c-1) -> d - 2^c and a carry out.    d in [-2^(c-1), 2^(c-1))
  independent  (window_digit_indep):  carry_in = bit (c w - 1) of k; raw >= 2^(c-1) -> raw + carry_in - 2^c.  d in [-2^(c-1), 2^(c-1)]
They differ on purpose at one corner: a raw window of 2^(c-1) - 1 that receives a carry.  The sequential rule turns it into -2^(c-1)
and carries on (the next window is one larger); the independent rule gives +2^(c-1) and no carry: the last entry of a lookup-table column.
"""
R = 0x30644e72e131a029b85045b68181585d2833e84879b9709143e1f593f0000001
GLV_HALF_BOUND = 0x6f4e << 112          # both GLV half-scalars stay below this (tests/test_glv_cpu.py: TOP)
COMB_C_MIN, COMB_C_MAX = 7, 17          # widths of the lookup table (comb_kernels.cuh)


class Shape:
    def __init__(self, c, W):
        self.c, self.W, self.nb = c, W, 1 << (c - 1)

    def __repr__(self):
        return "Shape(c=%d, W=%d)" % (self.c, self.W)


def make_shape(c, bits=254):
    """W windows of c bits cover `bits` bits; one more when the top window could reach 2^(c-1) with a carry"""
    W = (bits + c - 1) // c
    if bits - (W - 1) * c > c - 1:
        W += 1
    return Shape(c, W)


def bound_of(bits):
    return {254: R, 127: GLV_HALF_BOUND}[bits]


def raw_windows(k, c, W):
    return [(k >> (c * w)) & ((1 << c) - 1) for w in range(W)]


def recode_sequential(k, c, W):
    """-> (digits, carry out of the top window); the carry is 0 for every scalar the shape is made for"""
    half, carry, out = 1 << (c - 1), 0, []
    for raw in raw_windows(k, c, W):
        d = raw + carry
        if d >= half:
            carry = 1; d -= 1 << c
        else:
            carry = 0
        out.append(d)
    return out, carry


def recode_independent(k, c, W):
    out = []
    for w, raw in enumerate(raw_windows(k, c, W)):
        carry = (k >> (c * w - 1)) & 1 if w else 0
        d = raw + carry
        out.append(d - (1 << c) if raw >> (c - 1) else d)
    return out


def corner_windows(k, c, W):
    """windows whose raw value is 2^(c-1) - 1 and which receive a carry under the sequential rule: where the two rules part"""
    half, carry, out = 1 << (c - 1), 0, []
    for w, raw in enumerate(raw_windows(k, c, W)):
        if raw == half - 1 and carry:
            out.append(w)
        carry = 1 if raw + carry >= half else 0
    return out


def max_top_digit(c, bits=254):
    """the largest digit the top window takes over all scalars below the bound, under the sequential rule.  A recoding is a bijection
    between scalars and digit vectors, and the lower windows of a fixed top digit t cover one contiguous range of values above those of
    t - 1: the top digit never decreases as the scalar grows, so the largest scalar has the largest top digit."""
    s = make_shape(c, bits)
    return recode_sequential(bound_of(bits) - 1, c, s.W)[0][-1]


def carried_top_scalar(c, bits=254):
    """the top window one below its largest raw value, every lower window all ones: a carry that runs through the whole scalar into the top"""
    s = make_shape(c, bits); top = c * (s.W - 1)
    raw = (bound_of(bits) - 1) >> top
    return ((max(raw, 1) - 1) << top) | ((1 << top) - 1)


def _below(v, c, bound):
    """clear top windows until the value is below the bound"""
    while v >= bound:
        w = (v.bit_length() - 1) // c
        v &= (1 << (c * w)) - 1
    return v


def seam_scalars(c, bits=254):
    """scalars below the bound of `bits` that sit on every seam of the width-c recoding, without repeats, in a fixed order"""
    s = make_shape(c, bits); W, half, full = s.W, 1 << (c - 1), (1 << c) - 1
    bound = bound_of(bits)
    out = [0, 1, bound - 1, bound - 2]
    for w in range(W):
        out += [_below(1 << (c * w), c, bound), _below(1 << (c * w + c - 1), c, bound), _below((1 << (c * w + c)) - 1, c, bound)]
        out.append(_below((half - 1) << (c * w), c, bound))       # 2^(c-1) - 1 with no carry: the largest positive digit of the sequential rule
    for w in range(W - 1):                             # the corner: window w carries, window w + 1 holds 2^(c-1) - 1
        for low in (half, full):
            v = (low | ((half - 1) << c)) << (c * w)
            if v < bound:                              # (with the top window as w + 1 the value may not exist below the bound)
                out.append(v)
    out.append(carried_top_scalar(c, bits))
    out.append(_below(sum(half << (c * w) for w in range(W)), c, bound))
    out.append(_below((1 << (c * W)) - 1, c, bound))
    # a run of corners: every window above the lowest holds 2^(c-1) - 1, the carry started below runs through all of them
    out.append(_below(half | sum((half - 1) << (c * w) for w in range(1, W)), c, bound))
    seen, uniq = set(), []
    for v in out:
        if v not in seen:
            seen.add(v); uniq.append(v)
    return uniq


def corner_feasible(c, w, bits=254):
    """can window w (w >= 1) hold 2^(c-1) - 1 and receive a carry in a scalar below the bound?"""
    half = 1 << (c - 1)
    return w >= 1 and ((half | ((half - 1) << c)) << (c * (w - 1))) < bound_of(bits)


def lookup_need(npts, c):
    """bytes of the lookup table of npts points at width c (msm_host.hpp: bases_build_comb)"""
    s = make_shape(c)
    return npts * s.W * s.nb * 64


def lookup_width(npts, budget):
    """the width bases_build_comb takes for a budget: the widest whose table fits, or None when not even c = 7 does"""
    for c in range(COMB_C_MAX, COMB_C_MIN - 1, -1):
        if lookup_need(npts, c) <= budget:
            return c
    return None


def lookup_points(G_xy, h_xy=None):
    """points the handle of this generator set tabulates: with at least 10 % repeats among G and h the unique points and their sum
    (msm_host.hpp: bases_build_dedupe), else all of them"""
    pts = [G_xy[i:i + 64] for i in range(0, len(G_xy), 64)] + ([h_xy[:64]] if h_xy else [])
    U = len(set(pts))
    return U + 1 if U * 10 <= len(pts) * 9 else len(pts)
