"""GPU: sbn_polyeval_prove / sbn_joint_opening_prove against the literal model of the reference (tests/polyeval_model.py), against the
round-by-round loop through the calls that existed before them, and their failure behaviour and launch counts."""
import random

import pytest

import polyeval_model as pm
from polyeval_model import R_MOD, Transcript

pytestmark = pytest.mark.gpu
LABEL = b"gens_polyeval_test"


def _sbs(xs):
    return b"".join(pm.sb(x) for x in xs)


_GENS = {}


def _gens(ctx, n):
    """one handle per size for the whole module: the derived set and its lookup table are built once per handle"""
    if n not in _GENS:
        bases, xy = ctx.gens_new(n + 1, LABEL)
        _GENS[n] = (bases, pm.split_gens(xy, n))
    return _GENS[n]


@pytest.fixture(scope="module", autouse=True)
def _free_gens():
    yield
    for bases, _ in _GENS.values():
        bases.free()
    _GENS.clear()


def _small_case(ell, with_blinds, seed, zero_left=False, zero_rnd=False):
    rng = random.Random(seed)
    ml, mr = pm.factored_lens(ell)
    Z = [rng.randrange(R_MOD) for _ in range(1 << ell)]
    if zero_left:                                           # the left half of every row: L*Z has a zero left half, so L_0 = MSM(a_L, G_R) + 0 + 0
        Rs = 1 << mr
        Z = [0 if (i % Rs) < Rs // 2 else z for i, z in enumerate(Z)]
    r = [rng.randrange(R_MOD) for _ in range(ell)]
    blinds = [rng.randrange(R_MOD) for _ in range(1 << ml)] if with_blinds else None
    blind_Zr = rng.randrange(R_MOD) if with_blinds else None
    rnd = [0 if zero_rnd else rng.randrange(R_MOD) for _ in range(3 + 2 * mr)]
    return Z, r, blinds, blind_Zr, rnd, pm.dot(Z, pm.eq_evals(r))


def _check_against_model(ctx, sbn, ell, with_blinds, seed, **kw):
    ml, mr = pm.factored_lens(ell)
    bases, gens = _gens(ctx, 1 << mr)
    Z, r, blinds, blind_Zr, rnd, Zr = _small_case(ell, with_blinds, seed, **kw)
    tm = Transcript(b"polyeval gpu")
    want, want_Cy, want_Cx = pm.prove(tm, gens, Z, blinds, r, Zr, blind_Zr, rnd)
    t = ctx.table_upload(_sbs(Z))
    tr = sbn.Transcript(b"polyeval gpu")
    try:
        proof, Cx, Cy = ctx.polyeval_prove(bases, t, _sbs(r), pm.sb(Zr), _sbs(rnd), tr, blinds=_sbs(blinds) if blinds else None,
                                           blind_Zr=pm.sb(blind_Zr) if blind_Zr is not None else None)
        assert Cx == want_Cx and Cy == want_Cy
        assert proof == pm.proof_bytes(want)
        assert tr.state() == tm.state()
        assert ctx.table_download(t) == _sbs(Z)              # Z is only read
    finally:
        t.free()
    return want


@pytest.mark.parametrize("with_blinds", [False, True])
@pytest.mark.parametrize("ell", range(1, 10))
def test_polyeval_prove_is_bit_exact_against_the_model(ctx, sbn, ell, with_blinds):
    _check_against_model(ctx, sbn, ell, with_blinds, 300 + ell)


def test_polyeval_prove_compresses_an_infinity_L(ctx, sbn, ol):
    """all-zero rnd and a Z whose rows have a zero left half: a_L = 0, c_L = 0 and blind_L = 0, so round 0's L is the identity"""
    want = _check_against_model(ctx, sbn, 4, False, 17, zero_left=True, zero_rnd=True)
    assert want["L"][0] == pm.INF and ol.g1_compress(pm.INF)[31] == 0x40


def _loop_through_the_existing_abi(ctx, sbn, bases, gens_xy, Zt, blinds, r, Zr, blind_Zr, rnd, tr):
    """PolyEvalProof::prove assembled by the caller from the calls that existed before sbn_polyeval_prove, the transcript on the host"""
    ell = len(r)
    ml, mr = pm.factored_lens(ell)
    n, lg = 1 << mr, mr
    _, Qb, H = gens_xy
    Gn, G1 = ctx.bases_split_at(bases, n)
    Lt, Rt = ctx.eq_evals(_sbs(r[:ml])), ctx.eq_evals(_sbs(r[ml:]))
    LZ = ctx.table_bound(Zt, Lt)
    st = None
    try:
        Lv = [pm.ib(ctx.table_download(Lt)[32 * i:32 * i + 32]) for i in range(1 << ml)]
        blind_x = pm.dot(blinds, Lv) if blinds else 0
        by = blind_Zr or 0
        tr.append_message(b"protocol-name", b"polynomial evaluation proof")
        tr.append_message(b"protocol-name", b"dot product proof (log)")
        Cx = ctx.commit_table(Gn, LZ, pm.sb(blind_x), 1, n)[0]
        Cy = ctx.msm(pm.sb(Zr) + pm.sb(by), Qb + H)[0]
        tr.append_message(b"Cx", sbn.g1_compress(Cx)); tr.append_message(b"Cy", sbn.g1_compress(Cy))
        Rb = ctx.table_download(Rt)
        for i in range(n):
            tr.append_message(b"a", Rb[32 * i:32 * i + 32])
        rq = pm.ib(tr.challenge_scalar(b"r"))
        blind_G = (blind_x + rq * by) % R_MOD
        st, _ = ctx.bullet_begin_scaled(Gn, Qb, pm.sb(rq), LZ, Rt, want_gamma=False)
        Ls, Rs = [], []
        u = ui = None
        for j in range(lg):
            bl, br = rnd[3 + 2 * j], rnd[4 + 2 * j]
            if j == 0:
                Lxy, _, Rxy, _, _, _ = ctx.bullet_cross(st, pm.sb(bl), pm.sb(br))
            else:
                Lxy, _, Rxy, _, _, _ = ctx.bullet_fold_cross(st, pm.sb(u), pm.sb(ui), pm.sb(bl), pm.sb(br))
            tr.append_message(b"L", sbn.g1_compress(Lxy)); tr.append_message(b"R", sbn.g1_compress(Rxy))
            u = pm.ib(tr.challenge_scalar(b"u")); ui = pow(u, -1, R_MOD)
            blind_G = (u * u * bl + blind_G + ui * ui * br) % R_MOD
            Ls.append(sbn.g1_compress(Lxy)); Rs.append(sbn.g1_compress(Rxy))
        ctx.bullet_fold(st, pm.sb(u), pm.sb(ui))
        ah, bh, g_hat = ctx.bullet_finish(st)
        d, r_delta, r_beta = rnd[0], rnd[1], rnd[2]
        delta = ctx.msm(pm.sb(d) + pm.sb(r_delta), g_hat + H)[0]
        beta = ctx.msm(pm.sb(d * rq) + pm.sb(r_beta), Qb + H)[0]
        tr.append_message(b"delta", sbn.g1_compress(delta)); tr.append_message(b"beta", sbn.g1_compress(beta))
        c = pm.ib(tr.challenge_scalar(b"c"))
        x_hat, a_hat = pm.ib(ah), pm.ib(bh)
        z1 = (d + c * x_hat * a_hat) % R_MOD
        z2 = (a_hat * (c * blind_G + r_beta) + r_delta) % R_MOD
        return b"".join(Ls) + b"".join(Rs) + sbn.g1_compress(delta) + sbn.g1_compress(beta) + pm.sb(z1) + pm.sb(z2), Cx, Cy, Gn
    finally:
        if st is not None:
            st.free()
        for t in (Lt, Rt, LZ):
            t.free()
        G1.free()


@pytest.mark.parametrize("ell,with_blinds", [(20, False), (21, True), (25, False)])      # R_size 1024, 2048, 8192 (ell = 26 - 1: a 1 GiB table)
def test_polyeval_prove_at_prover_sizes(ctx, sbn, ell, with_blinds):
    """the model's verifier accepts the device's proof, and the bytes are those of the loop through the earlier ABI with the host transcript"""
    rng = random.Random(ell)
    ml, mr = pm.factored_lens(ell)
    n = 1 << mr
    bases, gens = _gens(ctx, n)
    N = 1 << ell
    mem = ctx.dev_alloc(32 * N)
    ctx.scalars_synthetic(0x9e1e + ell, 0, N, mem)
    Zt = ctx.table_from_dev(mem, N)
    r = [rng.randrange(R_MOD) for _ in range(ell)]
    blinds = [rng.randrange(R_MOD) for _ in range(1 << ml)] if with_blinds else None
    blind_Zr = rng.randrange(R_MOD) if with_blinds else None
    rnd = [rng.randrange(R_MOD) for _ in range(3 + 2 * mr)]
    Zr = pm.ib(ctx.table_evaluate(Zt, _sbs(r)))
    tr, tl = sbn.Transcript(b"polyeval gpu"), sbn.Transcript(b"polyeval gpu")
    Gn = None
    try:
        proof, Cx, Cy = ctx.polyeval_prove(bases, Zt, _sbs(r), pm.sb(Zr), _sbs(rnd), tr, blinds=_sbs(blinds) if blinds else None,
                                           blind_Zr=pm.sb(blind_Zr) if blind_Zr is not None else None)
        loop_proof, loop_Cx, loop_Cy, Gn = _loop_through_the_existing_abi(ctx, sbn, bases, gens, Zt, blinds, r, Zr, blind_Zr, rnd, tl)
        assert (proof, Cx, Cy) == (loop_proof, loop_Cx, loop_Cy)
        assert tr.state() == tl.state()
        comm_xy, _ = ctx.commit_table(Gn, Zt, _sbs(blinds) if blinds else None, 1 << ml, n)
        comm = [comm_xy[64 * i:64 * i + 64] for i in range(1 << ml)]
        tv = Transcript(b"polyeval gpu")
        assert pm.verify(tv, pm.proof_from_bytes(proof), gens, r, Cy, comm)
        assert tv.state() == tr.state()
    finally:
        if Gn is not None:
            Gn.free()
        Zt.free(); ctx.dev_free(mem)


LABEL_SETS = [(b"evals_ops_val", b"challenge_combine_n_to_one", b"joint_claim_eval"),          # sparse_mlpoly_full.rs:384-397
              (b"claim_evals_ops", b"challenge_combine_n_to_one", b"joint_claim_eval_ops"),    # :986-999
              (b"claim_evals_mem", b"challenge_combine_two_to_one", b"joint_claim_eval_mem")]  # :1013-1025


@pytest.mark.parametrize("count,labels", [(2, LABEL_SETS[2]), (8, LABEL_SETS[0]), (32, LABEL_SETS[1]), (2, LABEL_SETS[0]), (8, LABEL_SETS[1]), (32, LABEL_SETS[2])])
def test_joint_opening_prove_against_the_model(ctx, sbn, count, labels):
    rng = random.Random(count)
    ell_r = 3
    lc = count.bit_length() - 1
    ell = lc + ell_r
    n = 1 << pm.factored_lens(ell)[1]
    bases, gens = _gens(ctx, n)
    polys = [[rng.randrange(R_MOD) for _ in range(1 << ell_r)] for _ in range(count)]
    r = [rng.randrange(R_MOD) for _ in range(ell_r)]
    evals = [pm.dot(p, pm.eq_evals(r)) for p in polys]
    Z = [x for p in polys for x in p]
    rnd = [rng.randrange(R_MOD) for _ in range(3 + 2 * (n.bit_length() - 1))]
    tm = Transcript(b"joint gpu")
    ch, claim, want, want_Cy, want_Cx = pm.prove_single(tm, gens, Z, r, evals, rnd, labels)
    t = ctx.table_upload(_sbs(Z))
    tr = sbn.Transcript(b"joint gpu")
    try:
        got_ch, got_claim, proof, Cx, Cy = ctx.joint_opening_prove(bases, t, _sbs(evals), labels, _sbs(r), _sbs(rnd), tr)
        assert got_ch == _sbs(ch) and got_claim == pm.sb(claim)
        assert proof == pm.proof_bytes(want) and Cx == want_Cx and Cy == want_Cy
        assert tr.state() == tm.state()
    finally:
        t.free()


def test_a_failed_call_leaves_the_transcript_unchanged(ctx, sbn):
    ell = 4
    n = 1 << pm.factored_lens(ell)[1]
    bases, _ = _gens(ctx, n)
    short, _ = ctx.gens_new(n, LABEL)                        # one generator too few
    Gn, G1 = ctx.bases_split_at(bases, n)
    noh = ctx.bases_upload(ctx.bases_download(bases, 0, n + 1))      # the right length, no h
    Z, r, _, _, rnd, Zr = _small_case(ell, False, 5)
    t = ctx.table_upload(_sbs(Z))
    tr = sbn.Transcript(b"polyeval gpu")
    before = tr.state()
    bad = pm.sb(0)[:-1] + b"\xff"                            # >= r
    try:
        for kw in (dict(gens=short), dict(gens=noh), dict(gens=Gn), dict(rnd=_sbs(rnd[:-1]) + bad), dict(r=_sbs(r[:-1]) + bad), dict(Zr=bad),
                   dict(r=_sbs(r[:-1])), dict(r=b""), dict(blinds=_sbs([1] * ((1 << (ell // 2)) - 1)) + bad)):
            a = dict(gens=bases, r=_sbs(r), Zr=pm.sb(Zr), rnd=_sbs(rnd), blinds=None)
            a.update(kw)
            with pytest.raises(sbn.SbnError):
                ctx.polyeval_prove(a["gens"], t, a["r"], a["Zr"], a["rnd"], tr, blinds=a["blinds"])
            assert tr.state() == before
        with pytest.raises(sbn.SbnError):
            ctx.joint_opening_prove(short, t, _sbs([1, 2]), LABEL_SETS[0], _sbs(r[:3]), _sbs(rnd), tr)
        assert tr.state() == before
        ctx.polyeval_prove(bases, t, _sbs(r), pm.sb(Zr), _sbs(rnd), tr)      # and the good call moves it
        assert tr.state() != before
    finally:
        t.free()
        for b in (short, Gn, G1, noh):
            b.free()


def test_one_opening_is_lg_n_plus_two_row_commits(ctx, sbn):
    """Cx + Cy, one per round, delta + beta: lg n + 2 two-row commits — no commit for Gamma, none for g_hat"""
    ell = 12
    ml, mr = pm.factored_lens(ell)
    bases, _ = _gens(ctx, 1 << mr)
    rng = random.Random(3)
    Z = _sbs([rng.randrange(R_MOD) for _ in range(1 << ell)])
    r = _sbs([rng.randrange(R_MOD) for _ in range(ell)])
    rnd = _sbs([rng.randrange(R_MOD) for _ in range(3 + 2 * mr)])
    t = ctx.table_upload(Z)
    try:
        ctx.polyeval_prove(bases, t, r, pm.sb(1), rnd, sbn.Transcript(b"warm"))      # builds the derived set and its lookup table
        ctx.prof_enable(True); ctx.prof_reset()
        ctx.polyeval_prove(bases, t, r, pm.sb(1), rnd, sbn.Transcript(b"counted"))
        prof = ctx.prof_get()
    finally:
        ctx.prof_enable(False)
        t.free()
    launches = {k: v[1] for k, v in prof.items()}
    assert launches["k_points_to_host"] == mr + 2            # one hand-over per two-row commit
    assert launches["k_comb_rows"] == mr + 2                 # the lookup path's row kernel, once per commit
    assert launches["k_bullet_prep"] == mr and launches["k_polyeval_front"] == 1 and launches["k_polyeval_close"] == 1
    assert not any(k.startswith("k_xyzz_to_affine") or k in ("k_dot", "k_scalars_from_mont", "k_bucket_acc") for k in launches), launches
