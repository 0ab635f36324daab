"""GPU parity tests of the MSM / commitment path, all through the C ABI (include/sbn254.h).
Bit-exact bar: integer work — the 64-byte canonical affine output must equal the oracle's byte for byte."""
import numpy as np
import pytest
import acc_model
import window_model
from conftest import golden, rand_scalars

pytestmark = pytest.mark.gpu
H = bytes.fromhex
R_MONT_FR = (1 << 256)


def tiled_bases(ol, n, distinct, seed):
    """n bases made of `distinct` points with known discrete logs, tiled (duplicates exercise P+P in the buckets)"""
    dl = rand_scalars(distinct, seed)
    pts = ol.g1_mul_gen_batch(dl, 16)
    reps = (n + distinct - 1) // distinct
    return (pts * reps)[:64 * n], (dl * reps)[:32 * n]


def expect_from_dlogs(ol, pr, scalars, dlogs):
    return ol.g1_mul(pr.point_to_xy(pr.G), ol.fr_dot(scalars, dlogs))


def assert_acc_geometry(ctx, scalars=None, env=None):
    """the accumulate / reduction geometry the most recent single MSM ran with is the one the model of run_bucket_job gives
    (tests/acc_model.py), and, given the job's scalars (plain windows), its segment counters are the ones their bucket loads give"""
    job, acc = ctx.prof_last_job(), ctx.prof_last_acc()
    rec = job["slots"] // job["W"]                           # terms, or twice the terms under GLV
    assert acc_model.geometry_of(acc) == acc_model.geometry(acc_model.SINGLE, rec, job["W"], rec, job["c"], env), (job, acc)
    if scalars is not None:
        assert rec * 32 == len(scalars)
        loads = acc_model.loads_of_bytes(scalars, job["c"], job["W"])
        assert (acc["extra_count"], acc["big_count"]) == acc_model.expected_counters(loads, acc["SEG"]), (job, acc)
    return acc


def test_golden_msm_cases(ctx):
    for case in golden("msm_kat.json")["cases"]:
        s = b"".join(H(x) for x in case["scalars"]); p = b"".join(H(x) for x in case["points"])
        out, inf = ctx.msm(s, p)
        assert out == H(case["expected"]), case["note"]
        assert inf == (out == bytes(64))


def test_empty_msm_is_identity(ctx):
    out, inf = ctx.msm(b"", b"")          # group.rs:173 msm of empty slices = default()
    assert inf and out == bytes(64)


@pytest.mark.parametrize("n", [1, 2, 3, 31, 32, 33, 255, 1000, 8193, 1 << 14, (1 << 16) + 1])
def test_msm_vs_oracle(ctx, ol, pr, n):
    sc = rand_scalars(n, n)
    pts, dl = tiled_bases(ol, n, min(n, 4096), 77 + n)
    out, inf = ctx.msm(sc, pts)
    assert out == expect_from_dlogs(ol, pr, sc, dl) and not inf
    if n <= 8193:
        assert out == ol.msm_pippenger(sc, pts, 8)          # the arkworks-style CPU path itself


def test_msm_montgomery_inputs(ctx, ol, pr, sbn):
    """SBN_SCALARS_MONT / SBN_POINTS_MONT: ark-ff's in-memory limbs (value * 2^256 mod modulus)"""
    n = 300
    sc = rand_scalars(n, 1); pts, dl = tiled_bases(ol, n, n, 2)
    want = expect_from_dlogs(ol, pr, sc, dl)
    rq = ((1 << 256) % pr.P).to_bytes(32, "little"); rr = ((1 << 256) % pr.R).to_bytes(32, "little")
    sc_m = b"".join(ol.fe_op("mul", 1, sc[32 * i:32 * i + 32], rr) for i in range(n))
    pts_m = b"".join(ol.fe_op("mul", 0, pts[32 * i:32 * i + 32], rq) for i in range(2 * n))
    assert ctx.msm(sc_m, pts, sbn.SBN_SCALARS_MONT)[0] == want
    assert ctx.msm(sc, pts_m, sbn.SBN_POINTS_MONT)[0] == want
    assert ctx.msm(sc_m, pts_m, sbn.SBN_SCALARS_MONT | sbn.SBN_POINTS_MONT)[0] == want


def test_skewed_inputs(ctx, ol, pr):
    n = 6000
    pts, dl = tiled_bases(ol, n, 2048, 3)
    G = pr.point_to_xy(pr.G)
    one_scalar = rand_scalars(1, 4) * n                       # every scalar equal: W buckets hold all n points
    assert ctx.msm(one_scalar, pts)[0] == expect_from_dlogs(ol, pr, one_scalar, dl)
    sc = rand_scalars(n, 5)
    assert ctx.msm(sc, G * n)[0] == ol.g1_mul(G, ol.fr_dot(sc, (1).to_bytes(32, "little") * n))   # all bases == G
    half = n // 2                                             # P and -P pairs with equal scalars cancel exactly
    pn = b"".join(ol.g1_neg(pts[64 * i:64 * i + 64]) for i in range(half))
    out, inf = ctx.msm(sc[:32 * half] * 2, pts[:64 * half] + pn)
    assert inf and out == bytes(64)
    top = (pr.R - 1).to_bytes(32, "little") * n               # scalar r-1 everywhere (max signed-digit carries)
    assert ctx.msm(top, pts)[0] == expect_from_dlogs(ol, pr, top, dl)
    small = b"".join(int(i % 3).to_bytes(32, "little") for i in range(n))   # digits only in the lowest window, many zeros
    assert ctx.msm(small, pts)[0] == expect_from_dlogs(ol, pr, small, dl)


def test_resident_bases_and_prefix(ctx, ol, pr):
    n = 5000
    pts, dl = tiled_bases(ol, n, n, 9)
    b = ctx.bases_upload(pts)
    try:
        assert len(b) == n
        for m in (n, 1234, 1):
            sc = rand_scalars(m, m)
            assert ctx.msm_bases(b, sc)[0] == expect_from_dlogs(ol, pr, sc, dl[:32 * m])
        with pytest.raises(Exception):
            ctx.msm_bases(b, rand_scalars(n + 1, 1))
    finally:
        b.free()


def test_msm_jacobian_points(ctx, ol, pr):
    """vartime_multiscalar_mul (group.rs:143-158): projective inputs, including Z != 1 representatives and the identity"""
    n = 200
    sc = rand_scalars(n, 31); pts, dl = tiled_bases(ol, n, n, 32)
    zs = rand_scalars(n, 33)
    xyz = bytearray()
    for i in range(n):
        x, y = (int.from_bytes(pts[64 * i + 32 * j:64 * i + 32 * j + 32], "little") for j in (0, 1))
        z = int.from_bytes(zs[32 * i:32 * i + 32], "little") % pr.P or 1
        if i == 7:
            xyz += (1).to_bytes(32, "little") + (1).to_bytes(32, "little") + bytes(32)     # identity: Z = 0
            continue
        xyz += (x * z * z % pr.P).to_bytes(32, "little") + (y * z * z * z % pr.P).to_bytes(32, "little") + z.to_bytes(32, "little")
    dl7 = bytearray(dl); dl7[32 * 7:32 * 8] = bytes(32)                                    # point 7 contributes nothing
    out, inf = ctx.msm_jacobian(sc, bytes(xyz))
    assert out == expect_from_dlogs(ol, pr, sc, bytes(dl7)) and not inf


def test_bases_split_and_scale(ctx, ol, pr):
    """MultiCommitGens::split_at / scale (commitments.rs:64-98), as DotProductProofGens::new uses them (nizk/mod.rs:412-415)"""
    n = 40
    b, gxy = ctx.gens_new(n, b"gens_r1cs_sat")
    left, right = ctx.bases_split_at(b, 25)
    assert len(left) == 25 and len(right) == 15
    assert ctx.bases_download(left, 0, 26) == gxy[:64 * 25] + gxy[64 * n:]                # G[..mid] + h
    assert ctx.bases_download(right, 0, 16) == gxy[64 * 25:]                                # G[mid..] + h
    sc = rand_scalars(15, 1); bl = rand_scalars(1, 2)
    assert ctx.commit_rows(right, sc, bl, 1, 15)[0] == ol.commit(sc, bl, gxy[64 * 25:64 * n], gxy[64 * n:])
    s = rand_scalars(1, 3)
    scaled = ctx.bases_scale(b, s)
    want = b"".join(ol.g1_mul(gxy[64 * i:64 * i + 64], s) for i in range(n)) + gxy[64 * n:]   # h unchanged
    assert ctx.bases_download(scaled, 0, n + 1) == want
    for x in (left, right, scaled, b):
        x.free()


def test_gens_new_matches_golden_and_oracle(ctx, ol):
    g = golden("gens_kat.json")
    for label, row in g.items():
        n = row["n"]
        b, xy = ctx.gens_new(n, label.encode())
        try:
            for i, p in enumerate(row["first_points"]):
                assert xy[64 * i:64 * i + 64] == H(p)
            assert xy == ol.gens_new(n, label.encode())[0]
            G = bytes([1]) + bytes(31) + bytes([2]) + bytes(31)
            assert sum(1 for i in range(n + 1) if xy[64 * i:64 * i + 64] == G) == row["count_equal_to_G_incl_h"]
        finally:
            b.free()


def test_commit_golden(ctx, pr):
    """Pedersen / Hyrax commitments over the reference's own generator sets (66 % of them equal to G)"""
    for case in golden("commit_kat.json")["cases"]:
        R, L = case["R"], case["L"]
        b, _ = ctx.gens_new(R, case["label"].encode(), want_points=False)
        try:
            Z = pr.prng_scalars(L * R, case["seed"])
            if case["zero_row"] is not None:
                Z[R:2 * R] = [0] * R
                Z[2 * R:3 * R] = [Z[2 * R]] * R
            Zb = b"".join(pr.scalar_to_bytes(v) for v in Z)
            bl = b"".join(pr.scalar_to_bytes(v) for v in pr.prng_scalars(L, case["seed"] + 1)) if case["with_blinds"] else None
            out, infs = ctx.commit_rows(b, Zb, bl, L, R)
            assert out == b"".join(H(x) for x in case["expected_rows"]), case
            for i in range(L):
                assert infs[i] == (out[64 * i:64 * i + 64] == bytes(64))
        finally:
            b.free()


@pytest.mark.parametrize("L,R", [(1, 1), (2, 3), (5, 64), (7, 1000), (3, 8192)])
def test_commit_rows_vs_oracle(ctx, ol, L, R):
    gx, _ = ol.gens_new(R, b"gens_r1cs_eval")
    Z = bytearray(rand_scalars(L * R, L * 7 + R))
    if L >= 3:
        Z[32 * R:64 * R] = bytes(32 * R)
        Z[64 * R:96 * R] = Z[64 * R:64 * R + 32] * R
    Z = bytes(Z); bl = rand_scalars(L, 99)
    b = ctx.bases_upload(gx[:64 * R], gx[64 * R:])
    try:
        assert ctx.commit_rows(b, Z, bl, L, R)[0] == ol.commit_rows(Z, bl, L, R, gx[:64 * R], gx[64 * R:], 16)
        out, infs = ctx.commit_rows(b, Z, None, L, R)
        assert out == ol.commit_rows(Z, None, L, R, gx[:64 * R], gx[64 * R:], 16)
        if L >= 3:
            assert infs[1] == 1
    finally:
        b.free()


def test_commit_rows_host_chunked_pipeline(ctx, ol):
    """host-pointer commit of a matrix large enough (> 96 MB) to take the chunked path: row chunks cross PCIe while the
    previous chunk is committed; results must equal the device-resident path and the oracle on sampled rows"""
    import numpy as np
    L, R = 5300, 1024                                     # 166 MB -> chunks of 4096 rows: 2 chunks, the last one ragged
    gx, _ = ol.gens_new(R, b"gens_r1cs_sat")
    rng = np.random.default_rng(11)
    Z = rng.integers(0, 2**32, size=(L * R, 8), dtype=np.uint32); Z[:, 7] &= 0x0fffffff
    Z[5 * R:6 * R] = 0
    bl = rand_scalars(L, 12)
    b = ctx.bases_upload(gx[:64 * R], gx[64 * R:])
    try:
        out_h, inf_h = ctx.commit_rows(b, Z, bl, L, R)
        d = ctx.dev_alloc(Z.nbytes); ctx.dev_upload(d, Z)
        db = ctx.dev_alloc(len(bl)); ctx.dev_upload(db, bl)
        out_d, inf_d = ctx.commit_rows_dev(b, d, db, L, R)
        assert out_h == out_d and inf_h == inf_d
        Zb = Z.tobytes()
        for i in (0, 5, 4095, 4096, L - 1):
            assert out_h[64 * i:64 * i + 64] == ol.commit(Zb[32 * R * i:32 * R * (i + 1)], bl[32 * i:32 * i + 32], gx[:64 * R], gx[64 * R:])
        out_n, inf_n = ctx.commit_rows(b, Z, None, L, R)
        assert inf_n[5] == 1 and out_n[64 * 5:64 * 6] == bytes(64)
        ctx.dev_free(d); ctx.dev_free(db)
    finally:
        b.free()


def test_two_contexts_concurrently(sbn, ol, pr):
    """two contexts (two HIP streams + workspaces) driven from two host threads against ONE resident base table, as bench.py's
    steps-in-flight mode and a multi-threaded caller do"""
    import threading
    n = 1 << 15
    c1, c2 = sbn.Context(0), sbn.Context(0)
    b = c1.bases_synthetic(n, 0, S0.to_bytes(32, "little"), DSTEP.to_bytes(32, "little"))
    dl = _arith_dlogs(pr, 0, n)
    ks = [rand_scalars(n, 40 + i) for i in range(6)]
    want = [ol.g1_mul(pr.point_to_xy(pr.G), ol.fr_dot(k, dl)) for k in ks]
    got = [None] * 6

    def work(cx, idxs):
        for i in idxs:
            got[i] = cx.msm_bases(b, ks[i])[0]
    t1 = threading.Thread(target=work, args=(c1, [0, 2, 4])); t2 = threading.Thread(target=work, args=(c2, [1, 3, 5]))
    t1.start(); t2.start(); t1.join(); t2.join()
    assert got == want
    b.free(); c1.close(); c2.close()


def test_one_context_from_many_host_threads(ctx, ol, pr):
    """B1 swapped alone is entered from Rayon workers (hyrax.rs:259-261 -> commitments.rs:152 -> group.rs:171): many host threads,
    ONE context.  Calls serialise on the context's mutex; every thread must get its own result back."""
    import threading
    n = 3000
    pts, _ = ol.gens_new(n, b"threads")
    b = ctx.bases_upload(pts[:64 * n], pts[64 * n:])
    ks = [rand_scalars(n, 700 + i) for i in range(16)]
    want = [ol.msm_pippenger(k, pts[:64 * n], threads=4) for k in ks]
    got = [None] * 16
    tabs = [ctx.table_upload(rand_scalars(256, 800 + i)) for i in range(16)]
    dots = [None] * 16

    def work(i):
        got[i] = ctx.msm_bases(b, ks[i])[0] if i % 2 else ctx.msm(ks[i], pts[:64 * n])[0]
        dots[i] = ctx.table_dot(tabs[i], tabs[(i + 1) % 16])
    th = [threading.Thread(target=work, args=(i,)) for i in range(16)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert got == want
    hs = [rand_scalars(256, 800 + i) for i in range(16)]
    assert dots == [ol.fr_dot(hs[i], hs[(i + 1) % 16]) for i in range(16)]
    for t in tabs:
        t.free()
    b.free()


def test_shared_generators_first_commit_from_two_threads(sbn, ol):
    """two contexts commit against ONE freshly created generator set at the same time: the lazily built window table of the
    set must be built once and seen by both"""
    import threading
    R, L = 512, 6
    c1, c2 = sbn.Context(0), sbn.Context(0)
    b, gxy = c1.gens_new(R, b"gens_r1cs_sat")
    Z1, Z2 = rand_scalars(L * R, 70), rand_scalars(L * R, 71)
    got = {}

    def work(name, cx, Z):
        got[name] = cx.commit_rows(b, Z, None, L, R)[0]
    t1 = threading.Thread(target=work, args=("a", c1, Z1)); t2 = threading.Thread(target=work, args=("b", c2, Z2))
    t1.start(); t2.start(); t1.join(); t2.join()
    assert got["a"] == ol.commit_rows(Z1, None, L, R, gxy[:64 * R], gxy[64 * R:], 4)
    assert got["b"] == ol.commit_rows(Z2, None, L, R, gxy[:64 * R], gxy[64 * R:], 4)
    b.free(); c1.close(); c2.close()


def test_fuzz_random_shapes(ctx, ol, pr, sbn):
    """seeded fuzz over shapes / flags / degenerate patterns, every result against the oracle: ragged sizes around the internal
    thresholds (64-bucket chunks, 32-term window rule, LDS ranges), duplicated and opposite bases, zero / tiny / r-1 scalars,
    Montgomery-form inputs, blinds on and off."""
    import random
    rnd = random.Random(20260404)
    G = pr.point_to_xy(pr.G)
    pool_dl = rand_scalars(600, 555)
    pool_pts = ol.g1_mul_gen_batch(pool_dl, 16)
    rr = ((1 << 256) % pr.R).to_bytes(32, "little")

    def pick_scalar():
        m = rnd.randrange(8)
        if m == 0:
            return 0
        if m == 1:
            return rnd.randrange(1, 16)
        if m == 2:
            return pr.R - 1 - rnd.randrange(4)
        if m == 3:
            return 1 << rnd.randrange(1, 253)
        return rnd.randrange(pr.R)

    for it in range(40):
        n = rnd.choice([1, 2, 31, 32, 33, 63, 64, 65, 127, 200, 513, rnd.randrange(1, 600)])
        idx = [rnd.randrange(600) if rnd.random() < 0.7 else rnd.randrange(8) for _ in range(n)]      # many repeated bases
        pts = bytearray(); dls = []
        for i in idx:
            p = pool_pts[64 * i:64 * i + 64]; d = int.from_bytes(pool_dl[32 * i:32 * i + 32], "little")
            if rnd.random() < 0.15:
                p = ol.g1_neg(p); d = (-d) % pr.R
            if rnd.random() < 0.03:
                p = bytes(64); d = 0                                                                   # a base at infinity
            pts += p; dls.append(d)
        ks = [pick_scalar() for _ in range(n)]
        kb = b"".join(k.to_bytes(32, "little") for k in ks)
        want = ol.g1_mul(G, (sum(k * d for k, d in zip(ks, dls)) % pr.R).to_bytes(32, "little"))
        flags = 0
        if rnd.random() < 0.3:
            kb = b"".join(ol.fe_op("mul", 1, kb[32 * i:32 * i + 32], rr) for i in range(n)); flags |= sbn.SBN_SCALARS_MONT
        out, inf = ctx.msm(kb, bytes(pts), flags)
        assert out == want, (it, n)
        assert inf == (want == bytes(64))
    for it in range(25):
        L = rnd.choice([1, 2, 3, 5, 17]); R = rnd.choice([1, 2, 7, 64, 65, 300, rnd.randrange(1, 400)])
        label = rnd.choice([b"gens_r1cs_eval", b"gens_r1cs_sat", b"fuzz%d" % it])
        gx, _ = ol.gens_new(R, label)
        Z = bytearray(b"".join(pick_scalar().to_bytes(32, "little") for _ in range(L * R)))
        if L > 1 and rnd.random() < 0.5:
            row = rnd.randrange(L); Z[32 * R * row:32 * R * (row + 1)] = Z[32 * R * row:32 * R * row + 32] * R   # constant row
        Z = bytes(Z)
        bl = rand_scalars(L, 900 + it) if rnd.random() < 0.5 else None
        with_h = bl is not None or rnd.random() < 0.5
        b = ctx.bases_upload(gx[:64 * R], gx[64 * R:] if with_h else None)
        got = ctx.commit_rows(b, Z, bl, L, R)[0]
        b.free()
        assert got == ol.commit_rows(Z, bl, L, R, gx[:64 * R], gx[64 * R:], 8), (it, L, R, label)


def test_commit_argument_errors(ctx, ol, sbn):
    gx, _ = ol.gens_new(8, b"x")
    b = ctx.bases_upload(gx[:64 * 8], gx[64 * 8:])
    nb = ctx.bases_upload(gx[:64 * 8])
    try:
        with pytest.raises(sbn.SbnError):          # commitments.rs:146 assert_eq!(gens_n.n, self.len())
            ctx.commit_rows(b, rand_scalars(7, 1), None, 1, 7)
        with pytest.raises(sbn.SbnError):          # blinds need h
            ctx.commit_rows(nb, rand_scalars(8, 1), rand_scalars(1, 2), 1, 8)
    finally:
        b.free(); nb.free()


S0 = 0x1234567890abcdef1234567890abcdef
DSTEP = 0x0fedcba987654321


def _arith_dlogs(pr, first, n):
    return b"".join(((S0 + (first + i) * DSTEP) % pr.R).to_bytes(32, "little") for i in range(n))


@pytest.mark.parametrize("L,R", [(1, 20000), (3, 3000), (2, 9000)])
def test_commit_rows_distinct_bases_paths(ctx, ol, pr, L, R):
    """rows with DISTINCT bases (no merging of equal bases): the generic chunked sort (1 x 20000: one problem, many
    entries), the fused per-row sort with a constant row (one bucket per window holds every column: staging overflow
    path) and a row of tiny scalars."""
    b = ctx.bases_synthetic(R, 5, S0.to_bytes(32, "little"), DSTEP.to_bytes(32, "little"))
    try:
        dl = _arith_dlogs(pr, 5, R)
        assert ctx.bases_download(b, 0, 3) == ol.g1_mul_gen_batch(dl[:96], 1)
        Z = bytearray(rand_scalars(L * R, 1000 + R))
        if L >= 2:
            Z[32 * R:64 * R] = Z[32 * R:32 * R + 32] * R                                   # constant row
        if L >= 3:
            Z[64 * R:96 * R] = b"".join(int(i % 5).to_bytes(32, "little") for i in range(R))  # tiny scalars
        Z = bytes(Z)
        out, infs = ctx.commit_rows(b, Z, None, L, R)
        G = pr.point_to_xy(pr.G)
        for i in range(L):
            assert out[64 * i:64 * i + 64] == ol.g1_mul(G, ol.fr_dot(Z[32 * R * i:32 * R * (i + 1)], dl)), i
    finally:
        b.free()


def test_msm_large_skew(ctx, ol, pr):
    """2^17 terms, every scalar equal: each window has ONE bucket with 131072 entries (segments + wave merges at scale)"""
    n = 1 << 17
    b = ctx.bases_synthetic(n, 0, S0.to_bytes(32, "little"), DSTEP.to_bytes(32, "little"))
    try:
        dl = _arith_dlogs(pr, 0, n)
        k = rand_scalars(1, 3) * n
        assert ctx.msm_bases(b, k)[0] == ol.g1_mul(pr.point_to_xy(pr.G), ol.fr_dot(k, dl))
        acc = assert_acc_geometry(ctx, k)
        assert acc["big_count"] <= ctx.prof_last_job()["W"] and acc["extra_count"] >= acc["big_count"] * (n // acc["SEG"] - 1)
        two = rand_scalars(2, 4)
        k2 = (two[:32] * (n // 2)) + (two[32:] * (n // 2))                                  # two distinct values
        assert ctx.msm_bases(b, k2)[0] == ol.g1_mul(pr.point_to_xy(pr.G), ol.fr_dot(k2, dl))
        assert_acc_geometry(ctx, k2)
    finally:
        b.free()


def test_msm_large_skew_two_level_sort(ctx, ol, pr):
    """2^21 terms through the two-level sort with degenerate digit distributions: every scalar equal (one partition and one bucket
    per window hold everything: 128 level-2 sub-chunks on one LDS counter, then 2^21-entry buckets cut into segments), and half
    of the scalars zero / the other half r - 1 (every digit of r - 1, zero digits never enter the sort)"""
    import torch
    n = 1 << 21
    b = ctx.bases_synthetic(n, 7, S0.to_bytes(32, "little"), DSTEP.to_bytes(32, "little"))
    try:
        one = rand_scalars(1, 31)
        for blob in (one * n, (bytes(32) + pr.scalar_to_bytes(pr.R - 1)) * (n // 2)):
            k = torch.frombuffer(bytearray(blob), dtype=torch.uint8).cuda()
            out, inf = ctx.msm_bases_dev(b, k.data_ptr(), n)
            assert ctx.prof_last_job()["c"] > 16                                             # the two-level path (c = 17 at this size)
            assert_acc_geometry(ctx, blob if ctx.prof_last_job()["slots"] == n * ctx.prof_last_job()["W"] else None)
            assert out == ol.g1_mul(pr.point_to_xy(pr.G), _dot_arith(pr, blob, 7, n)) and not inf
    finally:
        b.free()


def _dev_scalars(torch, n, seed, ctx=None):
    """n scalars uniform in Fr, FULL width (bits 252 / 253 set on ~3/4 of them), generated on the device by sbn_scalars_synthetic
    (SplitMix64 reduced mod r) as an (n, 8) int32 tensor"""
    x = torch.empty((n, 8), dtype=torch.int32, device="cuda")
    _CTX[0].scalars_synthetic(0x5BA27A2B4E254 + seed, 0, n, x.data_ptr())
    return x


_CTX = [None]


@pytest.fixture(autouse=True)
def _remember_ctx(ctx):
    _CTX[0] = ctx


def _add_mod_r(torch, pr, k1, k2):
    """(k1 + k2) mod r on (n, 8) int32 limb tensors of canonical values"""
    n = k1.shape[0]
    ks = (k1.to(torch.int64) & 0xffffffff) + (k2.to(torch.int64) & 0xffffffff)
    carry = torch.zeros(n, dtype=torch.int64, device=k1.device)
    for j in range(8):
        v = ks[:, j] + carry; ks[:, j] = v & 0xffffffff; carry = v >> 32
    rl = [(pr.R >> (32 * j)) & 0xffffffff for j in range(8)]
    ge = torch.ones(n, dtype=torch.bool, device=k1.device); decided = torch.zeros(n, dtype=torch.bool, device=k1.device)
    for j in range(7, -1, -1):
        gt = (ks[:, j] > rl[j]) & ~decided; lt = (ks[:, j] < rl[j]) & ~decided
        ge = torch.where(lt, torch.zeros_like(ge), ge); decided |= gt | lt
    borrow = torch.zeros(n, dtype=torch.int64, device=k1.device)
    for j in range(8):
        v = ks[:, j] - torch.where(ge, torch.full_like(borrow, rl[j]), torch.zeros_like(borrow)) - borrow
        borrow = (v < 0).to(torch.int64); ks[:, j] = v & 0xffffffff
    return ks.to(torch.int32).contiguous()          # values >= 2^31 wrap to the same 32 raw bits


def test_full_size_properties_2p20(ctx, ol, pr):
    """BASELINE config 2 size (2^20), checked through size-independent properties: discrete-log identity, linearity in the
    scalars, and additivity over base-point ranges (the multi-GPU decomposition)."""
    import torch
    n = 1 << 20
    pts, dl = tiled_bases(ol, n, 1 << 14, 21)
    b = ctx.bases_upload(pts)
    try:
        k1 = _dev_scalars(torch, n, 1); k2 = _dev_scalars(torch, n, 2)
        torch.cuda.synchronize()
        o1, _ = ctx.msm_bases_dev(b, k1.data_ptr(), n)
        o2, _ = ctx.msm_bases_dev(b, k2.data_ptr(), n)
        k1b = k1.cpu().numpy().tobytes(); k2b = k2.cpu().numpy().tobytes()
        assert o1 == expect_from_dlogs(ol, pr, k1b, dl)
        assert o2 == expect_from_dlogs(ol, pr, k2b, dl)
        # linearity: MSM(k1 + k2 mod r) == MSM(k1) + MSM(k2)
        ks32 = _add_mod_r(torch, pr, k1, k2)
        assert (np.frombuffer(k1b, dtype=np.uint32).reshape(n, 8)[:, 7] >> 28).max() >= 2          # full width: bits 252/253 are in use
        torch.cuda.synchronize()                         # the library runs on its own stream, not torch's
        os_, _ = ctx.msm_bases_dev(b, ks32.data_ptr(), n)
        assert os_ == ol.g1_add(o1, o2)
        # additivity over base ranges == the sharded path
        half = n // 2
        bl = ctx.bases_upload(pts[:64 * half]); bh = ctx.bases_upload(pts[64 * half:])
        pl, _ = ctx.msm_bases_dev(bl, k1.data_ptr(), half)
        ph, _ = ctx.msm_bases_dev(bh, k1.data_ptr() + 32 * half, half)
        from spartan_bn254_amd import binding
        assert binding.g1_sum(pl + ph)[0] == o1
        bl.free(); bh.free()
    finally:
        b.free()


def _dot_arith(pr, scalars, first, n):
    """sum_i k_i * (S0 + (first+i)*DSTEP) mod r, vectorised on 16-bit digits so every numpy partial sum stays below 2^64"""
    k16 = np.frombuffer(scalars, dtype=np.uint16).reshape(n, 16).astype(np.uint64)
    idx = np.arange(n, dtype=np.uint64)
    ilo, ihi = idx & np.uint64(0xFFFF), idx >> np.uint64(16)
    sum_k = 0; sum_ik = 0
    for j in range(16):
        col = k16[:, j]
        sum_k += int(col.sum(dtype=np.uint64)) << (16 * j)
        sum_ik += (int((col * ilo).sum(dtype=np.uint64)) + (int((col * ihi).sum(dtype=np.uint64)) << 16)) << (16 * j)
    return ((S0 * sum_k + DSTEP * (sum_ik + first * sum_k)) % pr.R).to_bytes(32, "little")


@pytest.mark.parametrize("logn", [22, 23, 24, 26])
def test_large_msm_dlog_identity(ctx, ol, pr, logn):
    """upper part of the BASELINE size range (2^23 = one GPU's share of config 4, 2^26 = all of it on one GPU): the two-level sort
    with windows of 17 and 20 bits, long bucket chains, the short top window; checked exactly through the discrete-log identity"""
    import torch
    n = 1 << logn
    first = 12345
    b = ctx.bases_synthetic(n, first, S0.to_bytes(32, "little"), DSTEP.to_bytes(32, "little"))
    try:
        k = _dev_scalars(torch, n, logn)
        torch.cuda.synchronize()
        out, inf = ctx.msm_bases_dev(b, k.data_ptr(), n)
        kb = k.cpu().numpy().tobytes()
        assert out == ol.g1_mul(pr.point_to_xy(pr.G), _dot_arith(pr, kb, first, n)) and not inf
    finally:
        b.free()


@pytest.mark.parametrize("budget_gib,want_c", [(100, 16), (200, 17)])
def test_hyrax_derefs_shape_properties(ctx, ol, pr, sbn, record_property, budget_gib, want_c):
    """BASELINE config 3: the derefs commitment shape 4096 x 8192 over the reference's generator set, rows
    3072.. zero (hyrax.rs:245).  Checked on sampled rows against single-row commits of the oracle + structure.
    Two cases, each asserting the window of the lookup table it tested: c = 16 (94 GB) and c = 17 (177 GB: what bench.py and the
    prove-stages harness use).  The c = 17 case SKIPS (with the reason, and a warning in the summary) when the box cannot give 177 GB."""
    import torch
    import warnings
    L, R = 4096, 8192
    bases, gxy = ctx.gens_new(R, b"gens_r1cs_eval")
    try:
        Z = _dev_scalars(torch, L * R, 33)          # uniform in Fr, full width (254-bit eq-table values)
        Z[3072 * R:] = 0
        Z[5 * R:6 * R] = Z[5 * R]                 # one constant row (repeated mem[0], sparse_mlpoly_full.rs:89-101)
        torch.cuda.synchronize()
        assert int(((Z[:3072 * R, 7].to(torch.int64) & 0xffffffff) >> 28).max()) >= 2
        out, infs = ctx.commit_rows_dev(bases, Z.data_ptr(), 0, L, R)
        assert all(infs[i] == 1 for i in range(3072, 4096)) and out[64 * 3072:] == bytes(64 * 1024)
        assert not any(infs[:3072])
        for i in (0, 5, 1000, 3071):
            row = Z[i * R:(i + 1) * R].cpu().numpy().tobytes()
            assert out[64 * i:64 * i + 64] == ol.commit(row, bytes(32), gxy[:64 * R], gxy[64 * R:])
        # rows are independent: a 2-row slice gives the same commitments (row-sharded multi-GPU path)
        o2, _ = ctx.commit_rows_dev(bases, Z.data_ptr() + 32 * R * 1000, 0, 2, R)
        assert o2 == out[64 * 1000:64 * 1002]
        # fixed-base lookup table in HBM (sbn_bases_precompute): a different algorithm (no buckets), the same 4096 points
        # the table bench.py and the prove-stages harness use: c = 17, 177 GB for the 2814 unique points of this set; when the box cannot
        # give that much HBM right now, the c = 16 table (94 GB) is what gets tested
        try:
            cw = ctx.bases_precompute(bases, budget_gib << 30)
        except sbn.SbnError as e:
            if want_c == 17:
                warnings.warn(f"lookup table c = 17 NOT tested: {budget_gib} GiB not available on this box ({e})")
                pytest.skip(f"the c = 17 lookup table needs 177 GB of HBM: {e}")
            raise
        record_property("lookup_window_bits", cw)
        assert cw == want_c, f"lookup table built with c = {cw}, this case is the c = {want_c} table"
        out3, infs3 = ctx.commit_rows_dev(bases, Z.data_ptr(), 0, L, R)
        assert out3 == out and infs3 == infs
        o4, _ = ctx.commit_rows_dev(bases, Z.data_ptr() + 32 * R * 1000, 0, 2, R)       # few rows: several blocks per row
        assert o4 == out[64 * 1000:64 * 1002]
    finally:
        bases.free()


@pytest.mark.parametrize("R,label,budget_mb", [(64, b"gens_r1cs_eval", 8), (100, b"distinct", 64), (1024, b"gens_r1cs_sat", 512)])
def test_commit_rows_with_lookup_table_vs_oracle(ctx, ol, pr, R, label, budget_mb):
    """sbn_bases_precompute: every row commitment by table lookup must equal the oracle's (and the bucket path's), with and
    without blinds, for zero / constant / ordinary rows and edge scalars, at several row counts (1 block .. 16 blocks per row)."""
    gx, _ = ol.gens_new(R, label)
    if label == b"distinct":                      # all-distinct bases: no merged columns
        gx = ol.g1_mul_gen_batch(rand_scalars(R + 1, 4242))
    b = ctx.bases_upload(gx[:64 * R], gx[64 * R:])
    try:
        for L in (1, 2, 9, 40):
            Z = bytearray(rand_scalars(L * R, L * 13 + R))
            if L >= 9:
                Z[32 * R:64 * R] = bytes(32 * R)                                  # zero row
                Z[64 * R:96 * R] = Z[64 * R:64 * R + 32] * R                      # constant row
                edge = [0, 1, pr.R - 1, pr.R - 2, 1 << 253, (1 << 128) - 1, 1 << 15, (1 << 16) - 1]
                Z[96 * R:96 * R + 32 * len(edge)] = b"".join(pr.scalar_to_bytes(v) for v in edge)
            Z = bytes(Z); bl = rand_scalars(L, 5 + L)
            want_b = ol.commit_rows(Z, bl, L, R, gx[:64 * R], gx[64 * R:], 16)
            want_0 = ol.commit_rows(Z, None, L, R, gx[:64 * R], gx[64 * R:], 16)
            if L == 1:
                before = ctx.commit_rows(b, Z, bl, L, R)[0]
                assert before == want_b
                cw = ctx.bases_precompute(b, budget_mb << 20)
                assert cw == window_model.lookup_width(window_model.lookup_points(gx[:64 * R], gx[64 * R:]), budget_mb << 20)   # the widest table the budget buys
            assert ctx.commit_rows(b, Z, bl, L, R)[0] == want_b, (L, "blinds")
            out, infs = ctx.commit_rows(b, Z, None, L, R)
            assert out == want_0, (L, "no blinds")
            if L >= 9:
                assert infs[1] == 1
    finally:
        b.free()


def test_precompute_budget_errors(ctx, ol, sbn):
    gx, _ = ol.gens_new(16, b"x")
    b = ctx.bases_upload(gx[:64 * 16], gx[64 * 16:])
    try:
        with pytest.raises(sbn.SbnError):
            ctx.bases_precompute(b, 1024)             # not even the smallest table fits
        assert ctx.bases_precompute(b, 1 << 20) >= 7
        assert ctx.bases_precompute(b, 1 << 20) >= 7  # idempotent
    finally:
        b.free()
    # a budget the device cannot honour: the allocation fails, the call reports it, and the handle keeps working (bucket method)
    n = 1 << 16
    big = ctx.bases_synthetic(n, 0, S0.to_bytes(32, "little"), DSTEP.to_bytes(32, "little"))
    try:
        with pytest.raises(sbn.SbnError):
            ctx.bases_precompute(big, 1 << 42)        # c = 16 would need 2.2 TB
        k = rand_scalars(n, 77)
        dl = _arith_dlogs(pr_mod(), 0, n)
        out, _ = ctx.commit_rows(big, k, None, 1, n)
        assert out == ol.g1_mul(pr_mod().point_to_xy(pr_mod().G), ol.fr_dot(k, dl))
    finally:
        big.free()


def pr_mod():
    import pyref
    return pyref


def test_fuzz_lookup_table_commits(ctx, ol, pr):
    """random shapes / window sizes / row patterns through sbn_bases_precompute + commit: R not a power of two, 1..70 rows (every
    blocks-per-row setting), blinds on and off, zero / constant / sparse rows, duplicate and infinite generators"""
    import random
    rng = random.Random(20260)
    for case in range(14):
        R = rng.choice([1, 2, 3, 17, 64, 100, 255, 300])
        L = rng.choice([1, 2, 3, 8, 31, 70])
        gx = bytearray(ol.g1_mul_gen_batch(rand_scalars(R + 1, 9000 + case)))
        if R >= 3 and case % 3 == 0:
            gx[64:128] = gx[0:64]                          # duplicate generator
            gx[128:192] = bytes(64)                        # generator at infinity
        gx = bytes(gx)
        Z = bytearray(rand_scalars(L * R, 9100 + case))
        for i in range(L):
            kind = rng.randrange(5)
            if kind == 0:
                Z[32 * R * i:32 * R * (i + 1)] = bytes(32 * R)
            elif kind == 1:
                Z[32 * R * i:32 * R * (i + 1)] = Z[32 * R * i:32 * R * i + 32] * R
            elif kind == 2:
                for j in range(R):
                    if rng.random() < 0.8:
                        Z[32 * (R * i + j):32 * (R * i + j + 1)] = bytes(32)
        Z = bytes(Z); bl = rand_scalars(L, 9200 + case)
        b = ctx.bases_upload(gx[:64 * R], gx[64 * R:])
        try:
            budget = rng.choice([64, 128, 512]) << 20
            cw = ctx.bases_precompute(b, budget)
            assert cw == window_model.lookup_width(window_model.lookup_points(gx[:64 * R], gx[64 * R:]), budget)   # the widest table the budget buys
            use_bl = case % 2 == 0
            got, infs = ctx.commit_rows(b, Z, bl if use_bl else None, L, R)
            want = ol.commit_rows(Z, bl if use_bl else None, L, R, gx[:64 * R], gx[64 * R:], 8)
            assert got == want, (case, R, L, cw, use_bl)
            assert all((infs[i] == 1) == (want[64 * i:64 * i + 64] == bytes(64)) for i in range(L))
        finally:
            b.free()


# ---- round 2 ---------------------------------------------------------------------------------------------------------
def test_scalars_synthetic_matches_host_twin(ctx, pr):
    """sbn_scalars_synthetic (device) == bench.splitmix_scalars (numpy) == the definition in SURVEY 8d config 2; canonical, full width"""
    import torch
    import bench
    n, first, seed = 5000, 12345, 0x5BA27A2B4E254
    x = torch.empty(32 * n, dtype=torch.uint8, device="cuda")
    ctx.scalars_synthetic(seed, first, n, x.data_ptr())
    got = x.cpu().numpy().tobytes()
    assert got == bench.splitmix_scalars(n, seed, first)
    M64 = (1 << 64) - 1

    def sm(idx):
        z = (seed + idx * 0x9E3779B97F4A7C15) & M64
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
        return z ^ (z >> 31)
    for t in (0, 1, 4999):
        limbs = [sm(4 * (first + t) + j + 1) for j in range(4)]
        limbs[3] &= (1 << 62) - 1
        v = sum(l << (64 * j) for j, l in enumerate(limbs))
        assert int.from_bytes(got[32 * t:32 * t + 32], "little") == (v - pr.R if v >= pr.R else v)
    vals = [int.from_bytes(got[32 * t:32 * t + 32], "little") for t in range(n)]
    assert max(vals) < pr.R and max(vals) >> 253 == 1 and sum(1 for v in vals if v >> 252) > n // 2


def test_noncanonical_scalars_rejected(ctx, ol, pr, sbn):
    """a scalar >= r (Scalar::from_bytes returns None for it, scalar.rs:87-95) must come back as an error from every entry point
    that reads caller scalars — never as a wrong point with SBN_OK — and must leave the context usable"""
    R = 64
    gx, _ = ol.gens_new(R, b"gens_r1cs_eval")                       # duplicates: the merge path
    gd, _ = ol.gens_new(R, b"distinct-set")                         # no duplicates: digits straight from the input
    good = rand_scalars(3 * R, 7)
    for badval in (pr.R, pr.R + 5, (1 << 256) - 1):
        bad = bytearray(good); bad[32 * (R + 3):32 * (R + 4)] = badval.to_bytes(32, "little"); bad = bytes(bad)
        pts = gd[:64 * R]
        with pytest.raises(sbn.SbnError, match="canonical"):
            ctx.msm(bad[:32 * 2 * R], (pts * 2))
        for gens in (gx, gd):
            b = ctx.bases_upload(gens[:64 * R], gens[64 * R:])
            try:
                with pytest.raises(sbn.SbnError, match="canonical"):
                    ctx.commit_rows(b, bad, None, 3, R)
                with pytest.raises(sbn.SbnError, match="canonical"):                       # a bad blind
                    ctx.commit_rows(b, good, bad[32 * R:32 * (R + 3)][:64] + badval.to_bytes(32, "little"), 3, R)
                ctx.bases_precompute(b, 8 << 20)                                             # lookup path
                with pytest.raises(sbn.SbnError, match="canonical"):
                    ctx.commit_rows(b, bad, None, 3, R)
                assert ctx.commit_rows(b, good, None, 3, R)[0] == ol.commit_rows(good, None, 3, R, gens[:64 * R], gens[64 * R:], 4)
            finally:
                b.free()
    # r - 1 is canonical and must work (top window full)
    top = (pr.R - 1).to_bytes(32, "little") * 4
    pts4 = gd[:64 * 4]
    assert ctx.msm(top, pts4)[0] == ol.msm_naive(top, pts4)


@pytest.mark.parametrize("variant", ["plain", "mont", "blinds", "dedupe", "lookup"])
def test_commit_rows_chunked_forced(ctx, ol, pr, sbn, variant, monkeypatch):
    """the chunked host path of sbn_commit_rows (two staging buffers, copy stream, copied / consumed events), forced onto a small
    matrix: 7 chunks of 3 rows + a ragged last one.  Must equal the device-resident path and the oracle in every launch branch."""
    L, R = 23, 96
    label = b"gens_r1cs_eval" if variant in ("dedupe", "lookup") else b"chunk-distinct"
    gx, _ = ol.gens_new(R, label)
    Z = rand_scalars(L * R, 900)
    Z = Z[:32 * R * 4] + bytes(32 * R) + Z[32 * R * 5:]                   # one zero row
    bl = rand_scalars(L, 901) if variant in ("blinds", "lookup") else None
    want = ol.commit_rows(Z, bl, L, R, gx[:64 * R], gx[64 * R:], 4)
    flags = 0; Zin, blin = Z, bl
    if variant == "mont":
        rr = ((1 << 256) % pr.R).to_bytes(32, "little")
        Zin = b"".join(ol.fe_op("mul", 1, Z[32 * i:32 * i + 32], rr) for i in range(L * R)); flags = sbn.SBN_SCALARS_MONT
    b = ctx.bases_upload(gx[:64 * R], gx[64 * R:])
    try:
        if variant == "lookup":
            ctx.bases_precompute(b, 16 << 20)
        monkeypatch.setenv("SBN_COMMIT_CHUNK_BYTES", str(3 * R * 32))
        out_c, inf_c = ctx.commit_rows(b, Zin, blin, L, R, flags)
        monkeypatch.delenv("SBN_COMMIT_CHUNK_BYTES")
        out_1, inf_1 = ctx.commit_rows(b, Zin, blin, L, R, flags)          # one piece
        d = ctx.dev_alloc(len(Zin)); ctx.dev_upload(d, Zin)
        db = 0
        if blin:
            db = ctx.dev_alloc(len(blin)); ctx.dev_upload(db, blin)
        out_d, inf_d = ctx.commit_rows_dev(b, d, db, L, R, flags)
        ctx.dev_free(d)
        if db:
            ctx.dev_free(db)
        assert out_c == want and out_1 == want and out_d == want
        assert inf_c == inf_1 == inf_d
        if not bl:
            assert inf_c[4] == 1
    finally:
        b.free()


def test_zero_size_calls_leave_no_error(ctx, ol, sbn):
    """L = 0 / n = 0 with the Montgomery flag and blinds used to launch zero-size grids (a sticky HIP error for the next call)"""
    R = 8
    gx, _ = ol.gens_new(R, b"zs")
    b = ctx.bases_upload(gx[:64 * R], gx[64 * R:])
    try:
        d = ctx.dev_alloc(64)
        assert ctx.commit_rows_dev(b, d, d, 0, R, sbn.SBN_SCALARS_MONT)[0] == b""
        out, inf = ctx.msm_bases_dev(b, d, 0, sbn.SBN_SCALARS_MONT)
        assert inf and out == bytes(64)
        Z = rand_scalars(R, 1)
        assert ctx.commit_rows(b, Z, None, 1, R)[0] == ol.commit_rows(Z, None, 1, R, gx[:64 * R], gx[64 * R:], 1)
        ctx.dev_free(d)
    finally:
        b.free()


@pytest.mark.parametrize("L,R,rows", [(2048, 2048, (0, 1, 777, 2047)), (8192, 8192, (0, 4095, 8191))])
def test_encode_time_commitment_shapes(ctx, ol, L, R, rows):
    """the encode-time commitments of SparseMatPolyCommitment (sparse_mlpoly_full.rs:183-184): comb_mem is 2048 x 2048,
    comb_ops 8192 x 8192 at keyless size, both over prefixes of the gens_r1cs_eval stream.  Uniform Fr scalars, sampled rows
    against the oracle, bucket method and lookup table."""
    import torch
    bases, gxy = ctx.gens_new(R, b"gens_r1cs_eval")
    try:
        Z = torch.empty(32 * L * R, dtype=torch.uint8, device="cuda")
        ctx.scalars_synthetic(77, 0, L * R, Z.data_ptr())
        out, infs = ctx.commit_rows_dev(bases, Z.data_ptr(), 0, L, R)
        assert not any(infs)
        Zv = Z.view(L, R * 32)
        for i in rows:
            assert out[64 * i:64 * i + 64] == ol.commit(Zv[i].cpu().numpy().tobytes(), bytes(32), gxy[:64 * R], gxy[64 * R:])
        ctx.bases_precompute(bases, 100 << 30)
        out2, infs2 = ctx.commit_rows_dev(bases, Z.data_ptr(), 0, L, R)
        assert out2 == out and infs2 == infs
    finally:
        bases.free()


@pytest.fixture()
def ctx_sort2(sbn, monkeypatch):
    """a context whose single MSMs take the two-level sort (sort2_kernels.cuh) from 1024 terms on instead of from 2^21"""
    monkeypatch.setenv("SBN_SORT2_MIN", "1024")
    c = sbn.Context(0)
    yield c
    c.close()


@pytest.mark.parametrize("c_bits,n", [(13, 1024), (13, 9000), (14, 2500), (16, 8192), (17, 8193), (19, 20000), (20, 30011), (21, 6000), (22, 5000)])
def test_two_level_sort_vs_oracle(ctx_sort2, ol, pr, monkeypatch, c_bits, n):
    """the large-MSM sort path at small sizes, across the window widths it is built for (2 .. 1024 partitions per window; chunks of 8192
    scalars: one partial chunk, exactly one, one + 1, several): bit-exact vs the discrete-log identity and the CPU Pippenger.
    (15 and 18 run in the tests below; test_gpu_window_widths.py runs every width 13 .. 22 on the seam scalars of that width)"""
    monkeypatch.setenv("SBN_MSM_C", str(c_bits))
    sc = rand_scalars(n, 900 + n + c_bits)
    pts, dl = tiled_bases(ol, n, min(n, 4096), 5 + n)
    out, inf = ctx_sort2.msm(sc, pts)
    assert ctx_sort2.prof_last_job()["c"] == c_bits                  # the window asked for was the window used
    assert out == expect_from_dlogs(ol, pr, sc, dl) and not inf
    if n <= 9000:
        assert out == ol.msm_pippenger(sc, pts, 8)


@pytest.mark.parametrize("spt", [2, 8])
def test_two_level_sort_both_block_sizes(ctx_sort2, ol, pr, monkeypatch, spt):
    """level 1 of the two-level sort with 2048 and with 8192 scalars per block (the automatic choice switches at 2^21 terms): partial last block,
    exactly one block, several; bit-exact vs the discrete-log identity"""
    monkeypatch.setenv("SBN_SORT2_SPT", str(spt))
    monkeypatch.setenv("SBN_MSM_C", "15")            # (small single MSMs would take c = 7 and with it the one-level sort)
    for n in (1500, 2048, 8192, 8193, 50000):
        sc = rand_scalars(n, 7000 + n + spt)
        pts, dl = tiled_bases(ol, n, min(n, 4096), 11 + n)
        out, inf = ctx_sort2.msm(sc, pts)
        assert out == expect_from_dlogs(ol, pr, sc, dl) and not inf, (spt, n)


def test_two_level_sort_skew_and_edges(ctx_sort2, ol, pr, sbn, monkeypatch):
    """skewed scalars (one partition of one window holds everything), zero scalars, r - 1, powers of two at the window seams, and
    a non-canonical scalar (rejected, scalar.rs:87-95) on the two-level path"""
    monkeypatch.setenv("SBN_MSM_C", "18")
    n = 12000
    pts, dl = tiled_bases(ol, n, 2048, 11)
    vals = [7] * 6000 + [0] * 1000 + [pr.R - 1] * 1000 + [1 << (18 * (i % 14)) for i in range(1000)] + [(1 << (18 * (i % 14) + 17)) for i in range(1000)] + [(1 << (18 * (i % 13) + 18)) - 1 for i in range(2000)]
    sc = b"".join(pr.scalar_to_bytes(v % pr.R) for v in vals)
    out, inf = ctx_sort2.msm(sc, pts)
    assert out == expect_from_dlogs(ol, pr, sc, dl)
    bad = bytearray(sc); bad[32 * 5000:32 * 5000 + 32] = pr.R.to_bytes(32, "little")
    with pytest.raises(sbn.SbnError):
        ctx_sort2.msm(bytes(bad), pts)
    assert ctx_sort2.msm(sc, pts)[0] == out                          # and the context is usable afterwards


def test_two_level_sort_matches_one_level(ctx, ctx_sort2, ol, monkeypatch):
    """same inputs, same window: both sorts feed the same accumulation -> identical bytes (2^17 terms, c = 15 and c = 16)"""
    n = 1 << 17
    sc = rand_scalars(n, 4242); pts, _ = tiled_bases(ol, n, 4096, 4243)
    for c_bits in (15, 16):
        monkeypatch.setenv("SBN_MSM_C", str(c_bits))
        assert ctx.msm(sc, pts) == ctx_sort2.msm(sc, pts)


@pytest.mark.parametrize("n", [511, 512, 700, 1024, 4096, 4097])
def test_small_single_msm_rule(ctx, ol, pr, n):
    """512 .. 4096 terms take the narrowest windows (c = 8 / 7) with segments of 8 points (choose_shape / run_bucket_job): the sizes on both sides of
    the rule's edges, with repeated points and edge scalars so that buckets overflow their first segment; vs the oracle's Pippenger"""
    sc = bytearray(rand_scalars(n, 8100 + n))
    for i, v in enumerate([0, 1, pr.R - 1, 1 << 253, (1 << 7) - 1, 1 << 6]):
        sc[32 * i:32 * i + 32] = pr.scalar_to_bytes(v % pr.R)
    for i in range(40, 40 + n // 4):                         # a quarter of the scalars equal: one bucket per window takes n / 4 entries
        sc[32 * i:32 * i + 32] = sc[32 * 40:32 * 41]
    sc = bytes(sc)
    pts, dl = tiled_bases(ol, n, min(n, 256), 9 + n)
    out, inf = ctx.msm(sc, pts)
    assert ctx.prof_last_job()["c"] == (7 if 512 < n <= 4096 else 8 if n == 512 else ctx.prof_last_job()["c"])
    acc = assert_acc_geometry(ctx, sc)
    assert (acc["SEG"] == 8) == (512 <= n <= 4096) and acc["big_count"] >= 1
    assert out == ol.msm_pippenger(sc, pts, 8) and not inf


@pytest.mark.parametrize("L", [1, 3, 5, 7, 11, 33])
def test_bucket_reduction_any_buckets_per_lane(ctx, ol, pr, monkeypatch, L):
    """k_reduce_l1 with L buckets per lane, L not a power of two: the last chunk of a window is ragged (buckets past the end count as
    the identity), the cross-lane weight is L * lane and the combine levels weigh a chunk with L * 64^k.  Window widths whose bucket
    counts are one lane-row (c = 7: 64 buckets, every L > 1 leaves most lanes past the end), not a multiple of 64 L, and large (c = 15, two
    combine levels at small L); plus a shared-bucket-set row commit.  Bit-exact vs the discrete-log identity / the oracle."""
    monkeypatch.setenv("SBN_RED_L", str(L))
    for c_bits, n in [(7, 100), (8, 300), (10, 3000), (13, 9000), (15, 40000)]:
        monkeypatch.setenv("SBN_MSM_C", str(c_bits))
        sc = rand_scalars(n, 31 * L + c_bits)
        pts, dl = tiled_bases(ol, n, min(n, 4096), 3 + n)
        out, inf = ctx.msm(sc, pts)
        assert ctx.prof_last_job()["c"] == c_bits
        acc = assert_acc_geometry(ctx, sc, {"SBN_RED_L": str(L)})
        assert acc["L"] == L and acc["SEG"] == (8 if n == 3000 else 32)
        assert out == expect_from_dlogs(ol, pr, sc, dl) and not inf, (L, c_bits, n)
    monkeypatch.delenv("SBN_MSM_C")
    Lr, R = 5, 1000
    gx, _ = ol.gens_new(R, b"gens_r1cs_sat", 8)
    Z = rand_scalars(Lr * R, 77 + L); bl = rand_scalars(Lr, 78 + L)
    b = ctx.bases_upload(gx[:64 * R], gx[64 * R:])
    assert ctx.commit_rows(b, Z, bl, Lr, R)[0] == ol.commit_rows(Z, bl, Lr, R, gx[:64 * R], gx[64 * R:], 8)
    job, acc = ctx.prof_last_job(), ctx.prof_last_acc()
    assert job["buckets"] == Lr << (job["c"] - 1) and job["slots"] % (Lr * job["W"]) == 0
    cols = job["slots"] // (Lr * job["W"])                  # R + 1, or the unique bases of a merged set and their sum
    assert acc_model.geometry_of(acc) == acc_model.geometry(acc_model.ROWS, cols, Lr, cols * job["W"], job["c"], {"SBN_RED_L": str(L)}) and acc["L"] == L
    b.free()
