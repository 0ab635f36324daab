"""CPU: the equal-base scalar merge (csrc/msm_kernels.cuh: merge_small_body, merge_big_body) replayed limb for limb on
tests/fe_model.py (tests/merge_model.py) at the operands that maximise every sum it takes: all canonical scalars r - 1, all table
scalars at the top of fe_fix_tab's output, groups at the small/big split and on both sides of the first in-loop fe_reduce.

Each run asserts fe_model's preconditions at every step (fe_reduce on the wide line of its contract, |a| < 448 p; fe_mul's
column bound; fe_canon_small's (-p, 2p)) and compares the result with the plain integer sum mod r.  The largest sum that reached
each reduction is collected per site and checked against the figure derived for it:
  small store           64 table values below 2.5 r                                         < 160 r
  big in-loop reduce    128 canonical (32 table) terms on top of a reduced value            < 128 r + 1.76 r  (80 r + 1.76 r)
  big lane reduce       at most the same
  big store             256 reduced lanes, each in (-p e, p + p e) with e = (in-loop bound) / 594    < 256 (1 + 130 / 594) r = 312.1 r"""
import os
import random
import re
from fractions import Fraction

import pytest

import fe_model as fm
import merge_model as mm

R_MOD = fm.FR.p
CS = os.path.join(fm.ROOT, "spartan-bn254_amd", "csrc")
SEEN = {}                                   # (site, kind) -> largest |sum| / r over the whole module


def run(vals, internal, blind=None, blind_in_group=False, shuffle_seed=None):
    """one group holding every column of `vals` (plus the blind column R when blind_in_group); returns the model's output"""
    R = len(vals)
    cols = list(range(R)) + ([R] if blind_in_group else [])
    if shuffle_seed is not None:
        random.Random(shuffle_seed).shuffle(cols)
    mm.SITES.clear()
    got = mm.merge(vals, blind, R, cols, internal)
    assert got == mm.expected(vals, blind, R, cols, internal), (R, internal, blind_in_group)
    kind = "table" if internal else "canonical"
    sites = dict(mm.SITES)
    for site, v in sites.items():
        SEEN[(site, kind)] = max(SEEN.get((site, kind), 0), v)
    return sites


def top(internal):
    return mm.TAB_MAX if internal else R_MOD - 1


def test_model_matches_the_kernel_source():
    """the constants the replay hard-codes are the kernel's"""
    k = open(os.path.join(CS, "msm_kernels.cuh")).read()
    body = k[k.index("void merge_big_body("):k.index("__global__ void __launch_bounds__(256) k_merge(")]
    assert re.search(r"static const uint32_t MERGE_BIG = (\d+);", open(os.path.join(CS, "ctx.hpp")).read()).group(1) == str(mm.MERGE_BIG)
    assert "j < b; j += 1024)" in body and [int(x) for x in re.findall(r"j \+ (\d+) < b \?", body)] == [256, 512, 768]
    assert "acc = fe_add(fe_add(acc, x0), fe_add(fe_add(x1, x2), x3));" in body
    assert "if (((cnt += 4) & (internal ? 31u : 127u)) == 0) acc = fe_reduce(acc);" in body
    assert "for (int d = 32; d >= 1; d >>= 1) acc = fe_add(acc, fe_shfl_down(acc, d));" in body
    assert "fe_from_mont(fe_reduce(s))); else fe_store<FrP>(" in body
    assert "__launch_bounds__(256) k_merge(" in k and mm.BLOCK == 256
    small = k[k.index("void merge_small_body("):k.index("void merge_big_body(")]
    assert "if (b - a > big_threshold) return;" in small
    assert "fe_from_mont(fe_reduce(acc))); else fe_store<FrP>(out + 8 * t, acc);" in small


def test_table_top_is_what_fix_tab_leaves():
    F = fm.FR
    x = fm.from_int((9 * F.p) // 2 - 1)
    assert fm.pre_fix_tab(F, x) and fm.to_int(fm.fe_fix_tab(F, x)) == mm.TAB_MAX
    assert Fraction(5, 2) * F.p - 2 < mm.TAB_MAX < Fraction(5, 2) * F.p < 1 << 256


@pytest.mark.parametrize("internal", [False, True], ids=["canonical", "table"])
@pytest.mark.parametrize("n", [1, 2, 63, 64])
def test_small_groups_at_the_top(n, internal):
    v = top(internal)
    sites = run([v] * n, internal)
    assert set(sites) == {"small: store"} and sites["small: store"] == Fraction(n * v, R_MOD)
    # the blind column as one more member (n + 1 <= 64), present and absent; and outside the group
    if n < mm.MERGE_BIG:
        assert run([v] * n, internal, blind=v, blind_in_group=True)["small: store"] == Fraction((n + 1) * v, R_MOD)
        assert run([v] * n, internal, blind=None, blind_in_group=True)["small: store"] == Fraction(n * v, R_MOD)
    run([v] * n, internal, blind=v, blind_in_group=False)


BIG = [(65, False), (65, True), (1024, False), (1024, True), (1025, True), (7168, True), (7169, True), (8192, True),
       (31744, False), (31745, False), (32768, False)]


@pytest.mark.parametrize("n,internal", BIG, ids=["%d-%s" % (n, "table" if t else "canonical") for n, t in BIG])
def test_big_groups_at_the_top(n, internal):
    v = top(internal)
    sites = run([v] * n, internal)
    # the in-loop fe_reduce runs exactly when lane 0 has taken 128 canonical / 32 table terms: ceil(n / 1024) * 4 >= 128 / 32
    fires = -(-n // 1024) * 4 >= (32 if internal else 128)
    assert ("big: in-loop reduce" in sites) == fires, sites
    assert fires == (n > (7168 if internal else 31744))
    per_lane = (32 if internal else 128) * Fraction(v, R_MOD)
    if fires:
        assert per_lane - 3 * Fraction(v, R_MOD) <= sites["big: in-loop reduce"] < per_lane + Fraction(176, 100)    # the last four may be one term + 3 zeros
        if n % 1024 == 0:
            assert sites["big: in-loop reduce"] >= per_lane
    assert sites["big: lane reduce"] < per_lane + Fraction(176, 100)
    assert sites["big: store"] < 256 * (1 + (per_lane + 2) / 594)
    # the blind column inside the group (absent and present), and a shuffled column list
    run([v] * (n - 1), internal, blind=v, blind_in_group=True, shuffle_seed=n)
    if n <= 8192:
        run([v] * (n - 1), internal, blind=None, blind_in_group=True)


def test_store_sum_at_its_top():
    """r - 1 everywhere does not maximise the LAST sum: every lane's fe_reduce then returns about 1.0 r (256 r in all).  fe_reduce(a)
    returns the representative of a in [a e, a e + p), e = ONE29 / 2^261, so a lane sum a = 123 r + d with d just below a e comes
    back as r + d = 1.2 r.  31 744 equal columns (124 per lane, no in-loop reduce) of x = ceil((123 r + 0.2 r) / 124) do that."""
    x = -(-(123 * R_MOD + R_MOD // 5) // 124)
    assert x < R_MOD and 124 * x - 123 * R_MOD < Fraction(124 * x * fm.to_int(fm.FR.ONE29), fm.RMONT)
    sites = run([x] * 31744, False)
    assert "big: in-loop reduce" not in sites
    assert Fraction(256 * 12, 10) < sites["big: store"] < 256 * (1 + Fraction(130, 594))


@pytest.mark.parametrize("internal", [False, True], ids=["canonical", "table"])
def test_random_values_and_scattered_columns(internal):
    """a row with several groups whose columns interleave; values random over the whole input range"""
    rng = random.Random(17 + internal)
    sizes = [1, 2, 63, 64, 65, 257, 1025]
    R = sum(sizes)
    order = list(range(R))
    rng.shuffle(order)
    Z = [rng.randrange(int(2.5 * R_MOD) if internal else R_MOD) for _ in range(R)]
    blind = rng.randrange(R_MOD)
    at = 0
    for i, n in enumerate(sizes):
        cols = order[at:at + n] + ([R] if i in (1, 5) else [])
        at += n
        for bl in (blind, None):
            assert mm.merge(Z, bl, R, cols, internal) == mm.expected(Z, bl, R, cols, internal), (n, bl is None)


def test_sums_stay_inside_the_wide_contract():
    """runs last in this module: the largest sum per site over every case above, against fe_reduce's wide line (448 p) with margin"""
    want = {(s, t) for s in ("small: store", "big: in-loop reduce", "big: lane reduce", "big: store") for t in ("canonical", "table")}
    if not set(SEEN) >= want:                       # selected alone: run the cases that carry the maxima
        for internal in (False, True):
            run([top(internal)] * 64, internal)
            run([top(internal)] * (8192 if internal else 32768), internal)
        test_store_sum_at_its_top()
    assert set(SEEN) >= want
    print("\nmerge model: largest |sum| / r that reached each reduction")
    for (site, kind), v in sorted(SEEN.items()):
        print(f"  {site:20s} {kind:9s} {float(v):8.2f} r")
    assert max(SEEN.values()) < 320 < fm.REDUCE_WIDE
    assert Fraction(159) < SEEN[("small: store", "table")] < 160
    assert Fraction(127) < SEEN[("big: in-loop reduce", "canonical")] < 130
    assert Fraction(79) < SEEN[("big: in-loop reduce", "table")] < 82
    assert Fraction(307) < SEEN[("big: store", "canonical")] < 313


def test_grouped_form_equals_commit_rows():
    """the expectation tests/test_gpu_merge_seams.py uses above R = 2049 (per-group integer sums mod r, then one MSM over the unique
    bases plus blind * h) equals the oracle's row commitments over the full matrix, at one small set with every kind of member:
    singletons, a group on each side of 64, the identity, a pair {P, -P}, h inside a group, shuffled columns"""
    import merge_sets as ms
    import oracle_lib as ol
    ps = ms.make_set(ol, [1, 2, 63, 65, 7, 3, 3], seed=5, pad_to=160, keys=[0, 1, 2, 3, "inf", 4, ("neg", 4)], h=("group", 3))
    assert ps.R == 160 and ps.unique() == 7 + 16 and len(ps.G) == 64 * 160
    rng = random.Random(6)
    L = 4
    Z = [rng.randrange(R_MOD) for _ in range(L * ps.R)]
    Z[160:320] = [R_MOD - 1] * 160
    Z[320:480] = [0] * 160
    for blinds in (None, [rng.randrange(R_MOD) for _ in range(L)]):
        want = ol.commit_rows(ms.pack(Z), ms.pack(blinds) if blinds else None, L, ps.R, ps.G, ps.h, 4)
        assert ms.grouped_rows(ps, Z, blinds, L) == want == ms.expected_rows(ps, Z, blinds, L)
        assert ms.inf_flags(want) == (bytes([0, 0, 1, 0]) if blinds is None else bytes(4))
