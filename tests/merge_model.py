"""Limb-exact replay, on tests/fe_model.py, of the arithmetic of the equal-base scalar merge (csrc/msm_kernels.cuh: merged_load,
merge_small_body, merge_big_body) for canonical and table (`internal`) scalars.

Test infrastructure only.  The order of the fe_add calls, the cadence of the in-loop fe_reduce, the wave fold, the four-wave fold
and the final fe_store / fe_from_mont(fe_reduce(.)) are the kernel's; the index arithmetic is plain Python.  Every fe_reduce,
fe_mul and fe_canon_small asserts its precondition as fe_model states it (pre_reduce on its wide line, pre_mul, pre_canon_small),
and SITES records the largest |sum| that reached each reduction, in units of r.

The wave fold is replayed for the lanes that feed lane 0 only (lane l < d adds lane l + d at step d): the other lanes of the
device's __shfl_down tree hold values nobody reads."""
from fractions import Fraction

import fe_model as fm

F = fm.FR
MERGE_BIG = 64
BLOCK = 256
SITES = {}                      # site -> largest |value| / r seen


def note(site, v):
    x = Fraction(abs(fm.to_int(v)), F.p)
    if x > SITES.get(site, 0):
        SITES[site] = x


def fe_load(x):
    """fe_load: 32 bytes, a non-negative integer below 2^256, as normalised limbs"""
    assert 0 <= x < 1 << 256
    return fm.from_int(x)


def merged_load(Z_row, blind, R, col):
    if col < R:
        return fe_load(Z_row[col])
    if blind is not None:
        return fe_load(blind)
    return list(fm.ZERO)


def fe_reduce(site, a):
    note(site, a)
    assert fm.pre_reduce(F, a, wide=True), (site, float(Fraction(fm.to_int(a), F.p)))
    r = fm.fe_reduce(F, a)
    lo, hi = fm.reduce_interval(F, a)
    assert fm.is_normalised(r) and lo <= fm.to_int(r) < hi and (fm.to_int(r) - fm.to_int(a)) % F.p == 0, site
    return r


def fe_canon(site, a):
    r = fe_reduce(site, a)
    assert fm.pre_canon_small(F, r), site
    return fm.fe_canon_small(F, r)


def fe_from_mont(a):
    one = fm.from_int(1)
    assert fm.pre_mul(a, one)
    r = fm.fe_mul(F, a, one)
    assert fm.pre_canon_small(F, r)
    return fm.fe_canon_small(F, r)


def finish(site, acc, internal):
    """internal: fe_store_packed(fe_from_mont(fe_reduce(acc))); else fe_store(acc) -> the stored integer"""
    out = fe_from_mont(fe_reduce(site, acc)) if internal else fe_canon(site, acc)
    x = fm.to_int(out)
    assert fm.is_normalised(out) and 0 <= x < F.p, site
    return x


def merge_small(Z_row, blind, R, cols, internal):
    """one lane of merge_small_body on an ordinary row: the group's columns `cols` (csr_cols[a..b)), b - a <= MERGE_BIG"""
    assert 1 <= len(cols) <= MERGE_BIG
    acc = merged_load(Z_row, blind, R, cols[0])
    for c in cols[1:]:
        acc = fm.fe_add(acc, merged_load(Z_row, blind, R, c))
    return finish("small: store", acc, internal)


def merge_big(Z_row, blind, R, cols, internal):
    """one block of merge_big_body: 256 lanes, four scalars in flight, stride 1024"""
    b = len(cols)
    assert b > MERGE_BIG
    mask = 31 if internal else 127
    lanes = []
    for t in range(BLOCK):
        acc, cnt = list(fm.ZERO), 0
        for j in range(t, b, 4 * BLOCK):
            x = [merged_load(Z_row, blind, R, cols[j + k * BLOCK]) if j + k * BLOCK < b else list(fm.ZERO) for k in range(4)]
            acc = fm.fe_add(fm.fe_add(acc, x[0]), fm.fe_add(fm.fe_add(x[1], x[2]), x[3]))
            cnt += 4
            if cnt & mask == 0:
                acc = fe_reduce("big: in-loop reduce", acc)
        lanes.append(fe_reduce("big: lane reduce", acc))
    sm = []
    for wv in range(BLOCK // 64):
        w = lanes[64 * wv:64 * wv + 64]
        d = 32
        while d >= 1:
            for lane in range(d):
                w[lane] = fm.fe_add(w[lane], w[lane + d])
            d >>= 1
        sm.append(w[0])
    s = sm[0]
    for wv in range(1, 4):
        s = fm.fe_add(s, sm[wv])
    return finish("big: store", s, internal)


def merge(Z_row, blind, R, cols, internal):
    return (merge_small if len(cols) <= MERGE_BIG else merge_big)(Z_row, blind, R, cols, internal)


def expected(Z_row, blind, R, cols, internal):
    """the plain integer sum mod r (table values stand for T 2^-261)"""
    s = sum(Z_row[c] if c < R else (blind or 0) for c in cols)
    return s * pow(fm.RMONT, -1, F.p) % F.p if internal else s % F.p


TAB_MAX = (9 * F.p) // 2 - 1 - 2 * F.p          # the largest value fe_fix_tab leaves: (-2p, 4.5p) -> [0, 2.5p), 4.5p - 1 loses 2p
