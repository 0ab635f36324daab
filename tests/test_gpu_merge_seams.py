"""GPU: the equal-base scalar merge (bases_build_dedupe in csrc/msm_host.hpp, k_row_const_flags / k_merge in csrc/msm_kernels.cuh)
at its group, lane and range seams, through sbn_commit_rows, sbn_commit_rows_dev and sbn_commit_table.

Point sets are laid out by explicit group-size lists over points of known discrete log (tests/merge_sets.py), the columns of a group
scattered over the row.  Expected values: oracle_lib.commit_rows on the full matrix for R <= 2049 (it knows nothing of groups), the
grouped form (Python integer sums mod r, then oracle_lib.msm_pippenger) above that; tests/test_merge_model_cpu.py shows the two
agree.  Every comparison is byte equality of the affine output and of the infinity flags.

The table for sbn_commit_table is a table of twice the length after sbn_bind_top, so its entries are the lazy representatives a
producer leaves; its expectation is computed from sbn_table_download.  L * R must be a power of two there, so sets are padded with
singleton columns to a power of two; where a case fixes R otherwise (tot = 20, R = 20, R = 33 000) the table call is left out and
the case says so."""
import random

import pytest

import merge_sets as ms
from merge_sets import R_MOD, pack, unpack

pytestmark = pytest.mark.gpu
_SETS = {}


def cached_set(ol, name, *a, **kw):
    if name not in _SETS:
        _SETS[name] = ms.make_set(ol, *a, **kw)
    return _SETS[name]


def rand_fr(rng, n):
    return [rng.getrandbits(256) % R_MOD for _ in range(n)]


def check(got, want):
    out, inf = got
    assert out == want, [i for i in range(len(want) // 64) if out[64 * i:64 * i + 64] != want[64 * i:64 * i + 64]]
    assert inf == ms.inf_flags(want)


def to_ark(vals):
    return [v * (1 << 256) % R_MOD for v in vals]


def run_rows(ctx, b, ps, Z, blinds, L, flags=0, want=None):
    """sbn_commit_rows and sbn_commit_rows_dev on the same matrix; returns the expected bytes"""
    want = want if want is not None else ms.expected_rows(ps, Z, blinds, L)
    Zin, bin_ = (to_ark(Z), to_ark(blinds) if blinds else None) if flags else (Z, blinds)
    Zb, bb = pack(Zin), pack(bin_) if bin_ else None
    check(ctx.commit_rows(b, Zb, bb, L, ps.R, flags), want)
    d = ctx.dev_alloc(max(len(Zb), 32)); db = 0
    try:
        ctx.dev_upload(d, Zb)
        if bb:
            db = ctx.dev_alloc(len(bb)); ctx.dev_upload(db, bb)
        check(ctx.commit_rows_dev(b, d, db, L, ps.R, flags), want)
    finally:
        ctx.dev_free(d)
        if db:
            ctx.dev_free(db)
    return want


def bound_table(ctx, lo, hi, r):
    """table_upload(lo || hi) then bind_top(r): lo + r (hi - lo), as the device's lazy representatives; -> (table, canonical values)"""
    t = ctx.table_upload(pack(lo + hi))
    ctx.bind_top(t, ms.sb(r))
    vals = unpack(ctx.table_download(t))
    assert len(vals) == len(lo) and all((a + r * (c - a)) % R_MOD == v for a, c, v in zip(lo[:64], hi[:64], vals[:64]))
    return t, vals


def run_table(ctx, b, ps, L, blinds, seed, lo=None, hi=None):
    rng = random.Random(seed)
    n = L * ps.R
    assert n & (n - 1) == 0
    t, vals = bound_table(ctx, lo or rand_fr(rng, n), hi or rand_fr(rng, n), rng.randrange(2, R_MOD))
    try:
        want = ms.expected_rows(ps, vals, blinds, L)
        check(ctx.commit_table(b, t, pack(blinds) if blinds else None, L, ps.R), want)
    finally:
        t.free()
    return vals, want


def upload(ctx, ps):
    return ctx.bases_upload(ps.G, ps.h)


# ---------------------------------------------------------------- group sizes
SIZE_SETS = {"1-2-63-64-65": ([1, 2, 63, 64, 65], 256), "256-257": ([256, 257], 1024), "512-513": ([512, 513], 2048),
             "768-769": ([768, 769], 2048), "1024-1025-2049": ([1024, 1025, 2049], 8192)}


@pytest.mark.parametrize("with_blinds", [False, True], ids=["noblind", "blinds"])
@pytest.mark.parametrize("name", list(SIZE_SETS))
def test_group_sizes(ctx, ol, name, with_blinds):
    """groups on both sides of MERGE_BIG = 64 (host big_list and the kernel's own test), several big groups in one set, and every
    guard of the four-in-flight loop: 256 | 257, 512 | 513, 768 | 769, 1024 | 1025, and a third trip of one term (2049)"""
    sizes, R = SIZE_SETS[name]
    ps = cached_set(ol, name, sizes, seed=len(name), pad_to=R)
    rng = random.Random(R + with_blinds)
    L = 3
    b = upload(ctx, ps)
    try:
        run_rows(ctx, b, ps, rand_fr(rng, L * R), rand_fr(rng, L) if with_blinds else None, L)
        run_table(ctx, b, ps, 2, rand_fr(rng, 2) if with_blinds else None, seed=R)
    finally:
        b.free()


def test_block_straddle(ctx, ol):
    """U + 1 = 100 merged columns, L = 3: the 300 (row, column) pairs of merge_small_body cross a 256-thread block inside row 2"""
    ps = cached_set(ol, "straddle", [3] * 79 + [1] * 19, seed=7, pad_to=256)
    assert ps.unique() + 1 == 100
    rng = random.Random(100)
    b = upload(ctx, ps)
    try:
        for bl in (None, rand_fr(rng, 3)):
            run_rows(ctx, b, ps, rand_fr(rng, 3 * 256), bl, 3)
        run_table(ctx, b, ps, 4, rand_fr(rng, 4), seed=101)
    finally:
        b.free()


# ---------------------------------------------------------------- where h sits
@pytest.mark.parametrize("kind", ["own", "in-small-group", "in-big-group", "no-h", "h-without-blinds"])
def test_h_position(ctx, ol, sbn, kind):
    """h as a unique base of its own, as a member of a 5-column group (the blind joins a small sum), as the base of a 300-column
    group (the blind is one term of merge_big_body), absent, and present with blinds = NULL (merged_load's zero)"""
    h = {"own": "own", "in-small-group": ("group", 0), "in-big-group": ("group", 1), "no-h": None, "h-without-blinds": ("group", 1)}[kind]
    ps = cached_set(ol, "h-" + str(h), [5, 300, 2], seed=11, pad_to=512, h=h)
    rng = random.Random(len(kind))
    L = 3
    blinds = None if kind in ("no-h", "h-without-blinds") else rand_fr(rng, L)
    Z = rand_fr(rng, L * 512)
    Z[512:1024] = [Z[512]] * 512                       # row 1 constant: the blind goes to h's merged column alone
    b = upload(ctx, ps)
    try:
        run_rows(ctx, b, ps, Z, blinds, L)
        run_table(ctx, b, ps, 2, blinds[:2] if blinds else None, seed=12)
        if kind == "no-h":
            with pytest.raises(sbn.SbnError, match="no h"):
                ctx.commit_rows(b, pack(Z), pack(rand_fr(rng, L)), L, 512)
            run_rows(ctx, b, ps, Z, None, L)
    finally:
        b.free()


# ---------------------------------------------------------------- row kinds
def row_kinds(rng, R):
    """(lo, hi) halves of a table whose bound rows are: constant, all zero, constant r - 1, constant except the last column"""
    c = rand_fr(rng, 5)
    lo = [c[0]] * R + [0] * R + [R_MOD - 1] * R + [c[2]] * (R - 1) + [c[3]]
    hi = [c[1]] * R + [0] * R + [R_MOD - 1] * R + [c[4]] * R
    return lo, hi


@pytest.mark.parametrize("with_blinds", [False, True], ids=["noblind", "blinds"])
@pytest.mark.parametrize("mode", ["canonical", "mont", "table"])
def test_row_kinds(ctx, ol, sbn, mode, with_blinds):
    """k_row_const_flags and the constant / zero branches of merge_small_body: a constant row goes to the sum-of-all-bases column,
    a zero row is the identity (blind * h with blinds), r - 1 is the largest constant, and one differing last column makes the row
    ordinary again.  Canonical scalars, ark-ff's Montgomery limbs, and table values."""
    R, L = 128, 4
    ps = cached_set(ol, "rows", [5, 70, 3], seed=3, pad_to=R, h=("group", 1))
    rng = random.Random(40 + with_blinds)
    blinds = rand_fr(rng, L) if with_blinds else None
    lo, hi = row_kinds(rng, R)
    b = upload(ctx, ps)
    try:
        if mode == "table":
            vals, want = run_table(ctx, b, ps, L, blinds, seed=41, lo=lo, hi=hi)
            assert len(set(vals[:R])) == 1 and vals[0] != 0 and vals[R:2 * R] == [0] * R and vals[2 * R:3 * R] == [R_MOD - 1] * R
            assert len(set(vals[3 * R:4 * R - 1])) == 1 and vals[4 * R - 1] != vals[3 * R]
        else:
            want = run_rows(ctx, b, ps, lo, blinds, L, flags=sbn.SBN_SCALARS_MONT if mode == "mont" else 0)
        if not with_blinds:
            assert want[64:128] == ms.INF                                  # the zero row
    finally:
        b.free()


@pytest.mark.parametrize("with_blinds", [False, True], ids=["noblind", "blinds"])
def test_single_column(ctx, ol, with_blinds):
    """R = 1 with h equal to the one base: every row is constant, U = 1"""
    ps = cached_set(ol, "R1", [1], seed=1, h=("group", 0))
    rng = random.Random(5)
    for L in (1, 3):
        b = upload(ctx, ps)
        try:
            Z = rand_fr(rng, L)
            Z[0] = 0
            run_rows(ctx, b, ps, Z, rand_fr(rng, L) if with_blinds else None, L)
        finally:
            b.free()
    b = upload(ctx, ps)
    try:
        run_table(ctx, b, ps, 2, rand_fr(rng, 2) if with_blinds else None, seed=6)
    finally:
        b.free()


# ---------------------------------------------------------------- the host's decisions
@pytest.mark.parametrize("unique", [18, 19])
def test_dedupe_decision(ctx, ol, unique):
    """tot = 20 points (19 + h): 18 unique ones are merged (U * 10 > tot * 9 is false), 19 are not; both give the reference value.
    (R = 19: no power of two, so no sbn_commit_table here.)"""
    ps = cached_set(ol, "tot20-%d" % unique, [3] + [1] * 16 if unique == 18 else [2] + [1] * 17, seed=unique)
    assert ps.R == 19 and ps.unique() == unique and (unique * 10 > 20 * 9) == (unique == 19)
    rng = random.Random(unique)
    b = upload(ctx, ps)
    try:
        Z = rand_fr(rng, 3 * 19)
        Z[19:38] = [Z[19]] * 19
        for bl in (None, rand_fr(rng, 3)):
            run_rows(ctx, b, ps, Z, bl, 3)
    finally:
        b.free()


@pytest.mark.parametrize("R", [20, 32])
def test_identity_sum(ctx, ol, R):
    """{P, -P} x 10: the extra column S = sum of all bases is the identity, so a constant row commits to the identity without
    blinds and to blind * h with them.  R = 20 as such (rows only); with {Q, -Q} x 6 more, R = 32 also goes through the table."""
    sizes, keys = ([10, 10], [0, ("neg", 0)]) if R == 20 else ([10, 10, 6, 6], [0, ("neg", 0), 1, ("neg", 1)])
    ps = cached_set(ol, "pm-%d" % R, sizes, seed=R, keys=keys, h="own")
    rng = random.Random(R)
    L = 4
    c = rng.randrange(1, R_MOD)
    Z = [c] * R + rand_fr(rng, R) + [0] * R + [R_MOD - 1] * R
    blinds = rand_fr(rng, L)
    b = upload(ctx, ps)
    try:
        want = run_rows(ctx, b, ps, Z, None, L)
        assert want[:64] == ms.INF and want[128:192] == ms.INF and want[192:256] == ms.INF and want[64:128] != ms.INF
        want = run_rows(ctx, b, ps, Z, blinds, L)
        assert want[:64] == ol.g1_mul(ps.h, ms.sb(blinds[0])) and want[128:192] == ol.g1_mul(ps.h, ms.sb(blinds[2]))
        if R == 32:
            lo = [c] * R + rand_fr(rng, R) + [0] * R + [R_MOD - 1] * R
            hi = [c] * R + rand_fr(rng, R) + [0] * R + [R_MOD - 1] * R
            for bl in (None, blinds):
                vals, want = run_table(ctx, b, ps, L, bl, seed=33, lo=lo, hi=hi)
                assert vals[:R] == [c] * R and (want[:64] == ms.INF) == (bl is None)
    finally:
        b.free()


@pytest.mark.parametrize("with_blinds", [False, True], ids=["noblind", "blinds"])
def test_identity_base(ctx, ol, with_blinds):
    """the most repeated base is the identity (64 zero bytes): a unique 'point' like any other for the merge, nothing for the sum"""
    R, L = 64, 4
    ps = cached_set(ol, "inf-base", [40, 5, 3], seed=9, pad_to=R, keys=["inf", 1, 2])
    assert ps.G.count(ms.INF) >= 1 and ps.cols.count("inf") == 40
    rng = random.Random(9 + with_blinds)
    Z = rand_fr(rng, L * R)
    Z[R:2 * R] = [Z[R]] * R
    blinds = rand_fr(rng, L) if with_blinds else None
    b = upload(ctx, ps)
    try:
        run_rows(ctx, b, ps, Z, blinds, L)
        run_table(ctx, b, ps, L, blinds, seed=10)
    finally:
        b.free()


# ---------------------------------------------------------------- the in-loop fe_reduce of merge_big_body
@pytest.mark.parametrize("group", [31744, 31745, 32768])
def test_reduce_branch_canonical(ctx, ol, group):
    """canonical scalars: lane 0 takes its 128th term, and with it the in-loop fe_reduce, from 31 745 columns on.  One row holds
    r - 1 in every column of the group (128 r per lane before the reduce, 307 r before the store), the other is random.
    R = 33 000 is no power of two: rows only."""
    R, L = 33000, 2
    ps = cached_set(ol, "red-%d" % group, [group], seed=group, pad_to=R)
    rng = random.Random(group)
    Z = rand_fr(rng, L * R)
    for j, k in enumerate(ps.cols):
        if k == 0:
            Z[j] = R_MOD - 1
    blinds = rand_fr(rng, L)
    b = upload(ctx, ps)
    try:
        run_rows(ctx, b, ps, Z, blinds, L)
    finally:
        b.free()


@pytest.mark.parametrize("group", [7168, 7169, 8192])
def test_reduce_branch_table(ctx, ol, group):
    """table scalars (lazy representatives below 2.5 r): the in-loop fe_reduce runs every 32 terms per lane, from 7 169 columns on"""
    R, L = 8192, 2
    ps = cached_set(ol, "tred-%d" % group, [group], seed=group, pad_to=R)
    rng = random.Random(group)
    b = upload(ctx, ps)
    try:
        run_table(ctx, b, ps, L, rand_fr(rng, L), seed=group)
        run_table(ctx, b, ps, L, None, seed=group + 1, lo=[R_MOD - 1] * (L * R), hi=[R_MOD - 1] * R + rand_fr(rng, R))
    finally:
        b.free()


# ---------------------------------------------------------------- the merged matrix through the lookup commit
@pytest.mark.parametrize("name", ["1-2-63-64-65", "h-in-big-group"])
def test_through_the_lookup(ctx, ol, sbn, name):
    """after sbn_bases_precompute the merged matrix goes through the fixed-base lookup commit, whose flagged rows read only
    col_value (the sum-of-all-bases column) and col_blind (the column h merged into)"""
    if name == "h-in-big-group":
        ps, R = cached_set(ol, "h-" + str(("group", 1)), [5, 300, 2], seed=11, pad_to=512, h=("group", 1)), 512
    else:
        ps, R = cached_set(ol, name, SIZE_SETS[name][0], seed=len(name), pad_to=SIZE_SETS[name][1]), SIZE_SETS[name][1]
    rng = random.Random(R + 1)
    b = upload(ctx, ps)
    try:
        assert ctx.bases_precompute(b, 64 << 20) >= 7
        for L in (4, 32):                                  # 4 rows: the lookup splits a row over blocks; 32 rows: one block per row + the flagged-row kernel
            lo, hi = row_kinds(rng, R)
            lo[:R] = rand_fr(rng, R)                       # rows: ordinary, zero, constant r - 1, constant but the last column, then ordinary ones
            lo += rand_fr(rng, (L - 4) * R); hi += rand_fr(rng, (L - 4) * R)
            for bl in (None, rand_fr(rng, L)):
                run_rows(ctx, b, ps, lo, bl, L)
                run_table(ctx, b, ps, L, bl, seed=R + L, lo=lo, hi=hi)
            run_rows(ctx, b, ps, lo, rand_fr(rng, L), L, flags=sbn.SBN_SCALARS_MONT)
    finally:
        b.free()


# ---------------------------------------------------------------- rejected input
def test_noncanonical_input(ctx, ol, sbn):
    """a scalar >= r in the last column of the last row, or in the blinds, of a merged set: SBN_EINVAL from both entry points, and
    the next valid call gives the reference value"""
    name = "1-2-63-64-65"
    ps = cached_set(ol, name, SIZE_SETS[name][0], seed=len(name), pad_to=256)
    rng = random.Random(77)
    L, R = 3, 256
    Z, blinds = rand_fr(rng, L * R), rand_fr(rng, L)
    b = upload(ctx, ps)
    d = ctx.dev_alloc(32 * L * R); db = ctx.dev_alloc(32 * L)
    try:
        for bad in (R_MOD, (1 << 256) - 1):
            badZ = pack(Z[:-1]) + bad.to_bytes(32, "little")
            badB = pack(blinds[:-1]) + bad.to_bytes(32, "little")
            for zb, bb in ((badZ, pack(blinds)), (pack(Z), badB), (badZ, None)):
                with pytest.raises(sbn.SbnError, match="rc=-1.*canonical"):
                    ctx.commit_rows(b, zb, bb, L, R)
                ctx.dev_upload(d, zb)
                if bb:
                    ctx.dev_upload(db, bb)
                with pytest.raises(sbn.SbnError, match="rc=-1.*canonical"):
                    ctx.commit_rows_dev(b, d, db if bb else 0, L, R)
                run_rows(ctx, b, ps, Z, blinds, L)
    finally:
        ctx.dev_free(d); ctx.dev_free(db)
        b.free()


def test_unknown_flags_rejected(ctx, ol, sbn):
    """sbn_commit_rows / sbn_commit_rows_dev and their group forms admit SBN_SCALARS_MONT only: the private table flag 0x10000 and
    an unknown bit are SBN_EINVAL, the context stays usable, and sbn_commit_table still reaches the table path"""
    name = "1-2-63-64-65"
    ps = cached_set(ol, name, SIZE_SETS[name][0], seed=len(name), pad_to=256)
    rng = random.Random(78)
    L, R = 2, 256
    Z, blinds = rand_fr(rng, L * R), rand_fr(rng, L)
    b = upload(ctx, ps)
    d = ctx.dev_alloc(32 * L * R)
    g = sbn.Group([0])
    gb = None
    try:
        ctx.dev_upload(d, pack(Z))
        gb = g.bases_upload(ps.G, ps.h)
        for flags in (0x10000, 4, 0x10001):
            with pytest.raises(sbn.SbnError, match="rc=-1.*flags"):
                ctx.commit_rows(b, pack(Z), pack(blinds), L, R, flags)
            with pytest.raises(sbn.SbnError, match="rc=-1.*flags"):
                ctx.commit_rows_dev(b, d, 0, L, R, flags)
            with pytest.raises(sbn.SbnError, match="rc=-1"):
                g.commit_rows(gb, pack(Z), pack(blinds), L, R, flags)
            with pytest.raises(sbn.SbnError, match="rc=-1"):
                g.commit_rows_dev(gb, [d], None, L, R, flags)
        want = run_rows(ctx, b, ps, Z, blinds, L)
        check(g.commit_rows(gb, pack(Z), pack(blinds), L, R), want)
        run_table(ctx, b, ps, L, blinds, seed=79)
    finally:
        if gb:
            gb.free()
        g.close()
        ctx.dev_free(d)
        b.free()
