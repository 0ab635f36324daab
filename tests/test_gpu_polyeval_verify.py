"""GPU: sbn_polyeval_verify / sbn_joint_opening_verify against the literal verifier of the reference (tests/polyeval_model.py,
tests/sparse_eval_model.joint_verify): accepted and refused proofs, the transcript afterwards, malformed input, misuse, the edges of the two
MSMs, the openings inside the one-call provers' proofs, prover sizes and the number of host waits."""
import ctypes as C
import random

import pytest

import dense_model as dm
import oracle_lib as ol
import polyeval_model as pm
import polyeval_verify_model as pvm
import r1cs_proof_model as rpm
import sparse_eval_model as sem
from polyeval_model import R_MOD, Transcript

pytestmark = pytest.mark.gpu
LABEL, OTHER_LABEL = b"gens_polyeval_verify", b"gens_polyeval_verify_other"
TR = b"polyeval verify gpu"
_GENS = {}


def _sbs(xs):
    return b"".join(pm.sb(x) for x in xs)


def _gens(ctx, n, label=LABEL):
    """one handle per size and label for the whole module -> (handle, (G, Q_base, h))"""
    if (n, label) not in _GENS:
        bases, xy = ctx.gens_new(n + 1, label)
        _GENS[(n, label)] = (bases, pm.split_gens(xy, n))
    return _GENS[(n, label)]


@pytest.fixture(scope="module", autouse=True)
def _free_gens():
    yield
    for bases, _ in _GENS.values():
        bases.free()
    _GENS.clear(); _CASES.clear()


_CASES = {}


def _case(ctx, ell, with_blinds, seed, Z=None, r=None):
    """a good opening, proved once per key by the model (the reference of every test that uses it) -> dict"""
    key = (ell, with_blinds, seed, Z is not None, r is not None)
    if key not in _CASES:
        rng = random.Random(seed)
        ml, mr = pm.factored_lens(ell)
        bases, gens = _gens(ctx, 1 << mr)
        Z = [rng.randrange(R_MOD) for _ in range(1 << ell)] if Z is None else Z
        r = [rng.randrange(R_MOD) for _ in range(ell)] if r is None else r
        blinds = [rng.randrange(R_MOD) for _ in range(1 << ml)] if with_blinds else None
        blind_Zr = rng.randrange(R_MOD) if with_blinds else None
        rnd = [rng.randrange(R_MOD) for _ in range(3 + 2 * mr)]
        Zr = pm.dot(Z, pm.eq_evals(r))
        tp = Transcript(TR)
        proof, C_Zr, Cx = pm.prove(tp, gens, Z, blinds, r, Zr, blind_Zr, rnd)
        _CASES[key] = dict(ell=ell, bases=bases, gens=gens, Z=Z, r=r, blinds=blinds, blind_Zr=blind_Zr, rnd=rnd, Zr=Zr, proof=proof, C_Zr=C_Zr, Cx=Cx,
                           comm=pm.commit_poly(gens, Z, blinds, ell), state=tp.state())
    return _CASES[key]


def _device_proof(ctx, sbn, k):
    t = ctx.table_upload(_sbs(k["Z"]))
    tr = sbn.Transcript(TR)
    try:
        proof, _, Cy = ctx.polyeval_prove(k["bases"], t, _sbs(k["r"]), pm.sb(k["Zr"]), _sbs(k["rnd"]), tr, blinds=_sbs(k["blinds"]) if k["blinds"] else None,
                                          blind_Zr=pm.sb(k["blind_Zr"]) if k["blind_Zr"] is not None else None)
        return proof, Cy, tr.state()
    finally:
        t.free()


def _verify(ctx, sbn, bases, comm_pts, r, proof_bytes, start=None, compressed=False, **kw):
    """-> (accepted, state before, state after); comm by upload or from compressed bytes"""
    comm = ctx.bases_from_compressed(b"".join(ol.g1_compress(p) for p in comm_pts)) if compressed else ctx.bases_upload(b"".join(comm_pts))
    tr = sbn.Transcript(TR) if start is None else sbn.Transcript.from_state(start)
    before = tr.state()
    try:
        return ctx.polyeval_verify(bases, comm, _sbs(r), proof_bytes, tr, **kw), before, tr.state()
    finally:
        comm.free()


# ---- accept ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("with_blinds", [False, True])
@pytest.mark.parametrize("ell", range(1, 10))
def test_accepts_the_provers_and_the_models_proof(ctx, sbn, ell, with_blinds):
    k = _case(ctx, ell, with_blinds, 700 + ell)
    tv = Transcript(TR)
    assert pm.verify(tv, k["proof"], k["gens"], k["r"], k["C_Zr"], k["comm"])
    dev_proof, dev_Cy, dev_state = _device_proof(ctx, sbn, k)
    assert dev_state == tv.state() == k["state"]
    for proof, C_Zr in ((dev_proof, dev_Cy), (pm.proof_bytes(k["proof"]), k["C_Zr"])):
        for compressed in (False, True):
            acc, before, after = _verify(ctx, sbn, k["bases"], k["comm"], k["r"], proof, compressed=compressed, C_Zr_xy=C_Zr)
            assert acc and before != after
            assert after == tv.state()                       # the model verifier's and the prover's, byte for byte
            if not with_blinds:                              # blind_Zr = 0: C_Zr = Zr * gens_1.G[0], verify_plain (hyrax.rs:139-151)
                acc, _, after = _verify(ctx, sbn, k["bases"], k["comm"], k["r"], proof, compressed=compressed, Zr=pm.sb(k["Zr"]))
                assert acc and after == tv.state()
    if not with_blinds:
        tp = Transcript(TR)
        assert pm.verify_plain(tp, k["proof"], k["gens"], k["r"], k["Zr"], k["comm"]) and tp.state() == tv.state()


# ---- reject ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("ell", [1, 2, 5])
def test_rejects_every_single_replacement_and_leaves_the_transcript(ctx, sbn, ell):
    k = _case(ctx, ell, True, 720 + ell)
    other_bases, other = _gens(ctx, 1 << pm.factored_lens(ell)[1], OTHER_LABEL)
    names = pvm.tamperings(ell)
    assert len(names) == 2 * pm.factored_lens(ell)[1] + 7 + (ell >= 2)
    for what in names:
        proof, r, C_Zr, comm, gens = pvm.tamper(what, k["proof"], k["r"], k["C_Zr"], k["comm"], k["gens"], other)
        assert not pm.verify(Transcript(TR), proof, gens, r, C_Zr, comm), what
        acc, before, after = _verify(ctx, sbn, other_bases if what == "gens" else k["bases"], comm, r, pm.proof_bytes(proof), C_Zr_xy=C_Zr)
        assert not acc and after == before, what


@pytest.mark.parametrize("ell", [1, 2, 5])
def test_verify_plain_rejects_another_Zr(ctx, sbn, ell):
    k = _case(ctx, ell, False, 740 + ell)
    bad = (k["Zr"] + 1) % R_MOD
    assert not pm.verify_plain(Transcript(TR), k["proof"], k["gens"], k["r"], bad, k["comm"])
    acc, before, after = _verify(ctx, sbn, k["bases"], k["comm"], k["r"], pm.proof_bytes(k["proof"]), Zr=pm.sb(bad))
    assert not acc and after == before
    acc, _, after = _verify(ctx, sbn, k["bases"], k["comm"], k["r"], pm.proof_bytes(k["proof"]), Zr=pm.sb(k["Zr"]))
    assert acc and after == k["state"]


# ---- malformed: what an adversary controls is SBN_OK with accepted = 0 ------------------------------------------------------------

def _refused_x(comp):
    x = int.from_bytes(comp, "little") & ((1 << 254) - 1)
    while True:
        x += 1
        c = x.to_bytes(32, "little")
        if ol.g1_decompress(c) is None:
            return c


@pytest.mark.parametrize("what", ["L_0 does not decompress", "z1 = r", "z2 = r", "beta has x >= p"])
def test_malformed_proofs_are_refused_not_errors(ctx, sbn, what):
    k = _case(ctx, 5, True, 725)
    good = pm.proof_bytes(k["proof"])
    lg = pm.factored_lens(5)[1]
    if what.startswith("L_0"):
        bad = _refused_x(good[:32]) + good[32:]
    elif what.startswith("beta"):
        q = 0x30644e72e131a029b85045b68181585d97816a916871ca8d3c208c16d87cfd47
        bad = good[:64 * lg + 32] + (q + 1).to_bytes(32, "little") + good[64 * lg + 64:]
    elif what.startswith("z1"):
        bad = good[:64 * lg + 64] + R_MOD.to_bytes(32, "little") + good[64 * lg + 96:]
    else:
        bad = good[:64 * lg + 96] + R_MOD.to_bytes(32, "little")
    assert len(bad) == len(good)
    if not what.startswith("z"):
        assert pm.proof_from_bytes(bad) is None             # the reference's deserialisation fails
    acc, before, after = _verify(ctx, sbn, k["bases"], k["comm"], k["r"], bad, C_Zr_xy=k["C_Zr"])
    assert not acc and after == before
    assert _verify(ctx, sbn, k["bases"], k["comm"], k["r"], good, C_Zr_xy=k["C_Zr"])[0]


# ---- edges of the two MSMs ------------------------------------------------------------------------------------------------------

def test_identity_commitments_of_zero_rows(ctx, sbn):
    ell = 4
    rng = random.Random(31)
    Z = [0 if (i >> 2) in (1, 2) else rng.randrange(R_MOD) for i in range(16)]      # rows 1 and 2 of the 4 x 4 view are zero, no blinds
    k = _case(ctx, ell, False, 31, Z=Z)
    assert k["comm"][1] == pm.INF and k["comm"][2] == pm.INF and k["comm"][0] != pm.INF
    for compressed in (False, True):
        acc, _, after = _verify(ctx, sbn, k["bases"], k["comm"], k["r"], pm.proof_bytes(k["proof"]), compressed=compressed, C_Zr_xy=k["C_Zr"])
        assert acc and after == k["state"]


def test_the_all_zero_polynomial(ctx, sbn):
    """Cx is the identity and is absorbed as sbn_g1_compress writes it"""
    ell = 4
    k = _case(ctx, ell, False, 32, Z=[0] * 16)
    assert k["Cx"] == pm.INF and k["Zr"] == 0 and set(k["comm"]) == {pm.INF}
    assert pm.verify(Transcript(TR), k["proof"], k["gens"], k["r"], k["C_Zr"], k["comm"])
    dev_proof, dev_Cy, dev_state = _device_proof(ctx, sbn, k)
    for compressed in (False, True):
        acc, _, after = _verify(ctx, sbn, k["bases"], k["comm"], k["r"], dev_proof, compressed=compressed, C_Zr_xy=dev_Cy)
        assert acc and after == k["state"] == dev_state
        acc, _, after = _verify(ctx, sbn, k["bases"], k["comm"], k["r"], dev_proof, compressed=compressed, Zr=pm.sb(0))
        assert acc and after == k["state"]


@pytest.mark.parametrize("ell", [3, 6])
def test_a_point_with_coordinates_zero_and_one(ctx, sbn, ell):
    """zero eq scalars on both sides: L and R are unit-like vectors"""
    rng = random.Random(33 + ell)
    r = [(0, 1, rng.randrange(R_MOD))[i % 3] for i in range(ell)]
    k = _case(ctx, ell, True, 33 + ell, r=r)
    assert pm.verify(Transcript(TR), k["proof"], k["gens"], k["r"], k["C_Zr"], k["comm"])
    acc, _, after = _verify(ctx, sbn, k["bases"], k["comm"], k["r"], pm.proof_bytes(k["proof"]), C_Zr_xy=k["C_Zr"])
    assert acc and after == k["state"]
    bad = dict(k["proof"], z2=(k["proof"]["z2"] + 1) % R_MOD)
    assert not _verify(ctx, sbn, k["bases"], k["comm"], k["r"], pm.proof_bytes(bad), C_Zr_xy=k["C_Zr"])[0]


def test_gens_with_and_without_a_precomputed_table(ctx, sbn):
    """the caller's handle with its own lookup table (sbn_bases_precompute) and a fresh one without: same verdicts, same transcript"""
    ell = 6
    k = _case(ctx, ell, True, 36)
    n = 1 << pm.factored_lens(ell)[1]
    good, bad = pm.proof_bytes(k["proof"]), pm.proof_bytes(dict(k["proof"], z1=(k["proof"]["z1"] + 1) % R_MOD))
    for precompute in (False, True):
        bases, xy = ctx.gens_new(n + 1, LABEL)
        try:
            assert pm.split_gens(xy, n) == k["gens"]
            if precompute:
                assert ctx.bases_precompute(bases, 64 << 20) >= 7
            acc, _, after = _verify(ctx, sbn, bases, k["comm"], k["r"], good, C_Zr_xy=k["C_Zr"])
            assert acc and after == k["state"]
            acc, before, after = _verify(ctx, sbn, bases, k["comm"], k["r"], bad, C_Zr_xy=k["C_Zr"])
            assert not acc and after == before
        finally:
            bases.free()


def test_the_glv_msm_over_a_commitment_with_identity_rows(ctx, sbn, monkeypatch):
    """a context whose single MSMs take the GLV path from 1024 half-scalars on: C_LZ over 512 row commitments, two of them the identity
    (phi of the identity stays the identity in the GLV table); the generator handle is shared with the session's context"""
    monkeypatch.setenv("SBN_MSM_GLV", "1"); monkeypatch.setenv("SBN_SORT2_MIN", "1024"); monkeypatch.delenv("SBN_MSM_C", raising=False)
    g = sbn.Context(0)
    monkeypatch.delenv("SBN_MSM_GLV"); monkeypatch.delenv("SBN_SORT2_MIN")
    ell = 19
    ml, mr = pm.factored_lens(ell)
    n, N = 1 << mr, 1 << ell
    bases, _ = _gens(ctx, n)
    rng = random.Random(19)
    r = _sbs([rng.randrange(R_MOD) for _ in range(ell)])
    rnd = _sbs([rng.randrange(R_MOD) for _ in range(3 + 2 * mr)])
    mem = g.dev_alloc(32 * N)
    Zt = Gn = G1 = comm = None
    try:
        g.scalars_synthetic(0x61f, 0, N, mem)
        g.dev_upload(mem + 32 * n * 3, bytes(32 * n * 2))      # rows 3 and 4 are zero
        Zt = g.table_from_dev(mem, N)
        Zr = g.table_evaluate(Zt, r)
        tr = sbn.Transcript(TR)
        proof, _, Cy = g.polyeval_prove(bases, Zt, r, Zr, rnd, tr)
        Gn, G1 = g.bases_split_at(bases, n)
        comm_xy, comm_inf = g.commit_table(Gn, Zt, None, 1 << ml, n)
        assert [i for i in range(1 << ml) if comm_inf[i]] == [3, 4] and comm_xy[64 * 3:64 * 5] == bytes(128)
        comm = g.bases_upload(comm_xy)
        bad = proof[:64 * mr + 64] + pm.sb((pm.ib(proof[64 * mr + 64:64 * mr + 96]) + 1) % R_MOD) + proof[64 * mr + 96:]
        g.prof_enable(True); g.prof_reset()
        tv = sbn.Transcript(TR)
        assert g.polyeval_verify(bases, comm, r, proof, tv, Zr=Zr) and tv.state() == tr.state()
        launches = {name: v[1] for name, v in g.prof_get().items()}
        g.prof_enable(False)
        assert launches["k_glv_split"] == 1 and launches["k_points_to_host"] == 2      # the MSM over comm, not the 2 lg n + 4 points of the proof
        tb = sbn.Transcript(TR)
        assert not g.polyeval_verify(bases, comm, r, bad, tb, C_Zr_xy=Cy) and tb.state() == sbn.Transcript(TR).state()
        td = sbn.Transcript(TR)                                # and the session's context, plain windows: the same verdict and transcript
        comm_d = ctx.bases_upload(comm_xy)
        try:
            assert ctx.polyeval_verify(bases, comm_d, r, proof, td, C_Zr_xy=Cy) and td.state() == tr.state()
        finally:
            comm_d.free()
    finally:
        g.prof_enable(False)
        for b in (Gn, G1, comm):
            if b is not None:
                b.free()
        if Zt is not None:
            Zt.free()
        g.dev_free(mem)
        g.close()


# ---- misuse: SBN_EINVAL, the transcript unchanged ---------------------------------------------------------------------------------

def test_misuse_is_an_error_and_leaves_the_transcript(ctx, sbn):
    ell = 4
    k = _case(ctx, ell, False, 41)
    ml, mr = pm.factored_lens(ell)
    n = 1 << mr
    bases = k["bases"]
    short, _ = ctx.gens_new(n, LABEL)                        # one generator too few
    noh = ctx.bases_upload(ctx.bases_download(bases, 0, n + 1))      # the right length, no h
    comm = ctx.bases_upload(b"".join(k["comm"]))
    comm_short = ctx.bases_upload(b"".join(k["comm"][:-1]))
    proof = pm.proof_bytes(k["proof"])
    r = _sbs(k["r"])
    tr = sbn.Transcript(TR)
    before = tr.state()
    bad = pm.sb(0)[:-1] + b"\xff"                            # >= r
    off_curve = k["C_Zr"][:32] + pm.sb(1)
    try:
        for kw in (dict(gens=short), dict(gens=noh), dict(comm=comm_short), dict(r=b""), dict(r=_sbs([1] * 41)), dict(r=r[:-32] + bad), dict(r=r[:-32]),
                   dict(Zr=pm.sb(k["Zr"])), dict(C_Zr_xy=None), dict(C_Zr_xy=None, Zr=bad), dict(C_Zr_xy=off_curve)):
            a = dict(gens=bases, comm=comm, r=r, C_Zr_xy=k["C_Zr"], Zr=None)
            a.update(kw)
            with pytest.raises(sbn.SbnError):
                ctx.polyeval_verify(a["gens"], a["comm"], a["r"], proof, tr, C_Zr_xy=a["C_Zr_xy"], Zr=a["Zr"])
            assert tr.state() == before, kw
        L = sbn.lib()
        acc = C.c_int(5)
        buf = lambda b: (C.c_uint8 * len(b)).from_buffer_copy(b)      # noqa: E731
        args = [ctx.h, bases.h, comm.h, buf(r), C.c_size_t(ell), buf(k["C_Zr"]), None, buf(proof), tr.h, C.byref(acc)]
        for null_at in (0, 1, 2, 3, 7, 8, 9):
            a = list(args); a[null_at] = None
            assert L.sbn_polyeval_verify(*a) == -1 and tr.state() == before, null_at
        with pytest.raises(sbn.SbnError):
            ctx.joint_opening_verify(short, comm, _sbs([1, 2]), LABEL_SETS[0], r[:96], proof, tr)
        with pytest.raises(sbn.SbnError):
            ctx.joint_opening_verify(bases, comm, _sbs([1, 2, 3]), LABEL_SETS[0], r[:64], proof, tr)      # not a power of two
        assert tr.state() == before
        assert ctx.polyeval_verify(bases, comm, r, proof, tr, C_Zr_xy=k["C_Zr"]) and tr.state() == k["state"] != before      # and the good call moves it
    finally:
        for b in (short, noh, comm, comm_short):
            b.free()


# ---- two host waits ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("plain", [False, True])
def test_one_verification_is_two_host_waits(ctx, sbn, plain):
    """the transcript needs C_LZ, the verdict needs the folded sum: two hand-overs, one commit for -z1 s (and one for Zr * G1 in verify_plain),
    no point leaves the device as affine coordinates and no other MSM result is waited for"""
    ell = 8
    k = _case(ctx, ell, False, 50)
    proof = pm.proof_bytes(k["proof"])
    comm = ctx.bases_upload(b"".join(k["comm"]))
    kw = dict(Zr=pm.sb(k["Zr"])) if plain else dict(C_Zr_xy=k["C_Zr"])
    try:
        assert ctx.polyeval_verify(k["bases"], comm, _sbs(k["r"]), proof, sbn.Transcript(TR), **kw)      # builds the derived set and its lookup table
        ctx.prof_enable(True); ctx.prof_reset()
        assert ctx.polyeval_verify(k["bases"], comm, _sbs(k["r"]), proof, sbn.Transcript(TR), **kw)
        prof = ctx.prof_get()
    finally:
        ctx.prof_enable(False)
        comm.free()
    launches = {name: v[1] for name, v in prof.items()}
    assert launches["k_points_to_host"] == 2                 # one hand-over per host wait
    assert launches["k_comb_rows"] == (2 if plain else 1)    # the lookup path's row kernel, once per one-row commit
    assert launches["k_g1_decompress"] == 1 and launches["k_polyeval_verify_row"] == 1 and launches["k_polyeval_eq"] == 1
    assert launches["k_acc_first"] == 2                      # the MSM over comm and the MSM over the proof's points
    assert not any(name.startswith("k_xyzz_to_affine") for name in launches), launches


# ---- the n-to-1 reduction in front --------------------------------------------------------------------------------------------------

LABEL_SETS = [sem.DEREFS_LABELS, sem.OPS_LABELS, sem.MEM_LABELS]
assert LABEL_SETS == [(b"evals_ops_val", b"challenge_combine_n_to_one", b"joint_claim_eval"), (b"claim_evals_ops", b"challenge_combine_n_to_one", b"joint_claim_eval_ops"),
                      (b"claim_evals_mem", b"challenge_combine_two_to_one", b"joint_claim_eval_mem")]      # the three of tests/test_gpu_polyeval.py


def _challenges(evals, labels):
    t = Transcript(b"joint verify gpu")
    sem.append_scalars(t, labels[0], evals)
    return [t.challenge_scalar(labels[1]) for _ in range(len(evals).bit_length() - 1)]


@pytest.mark.parametrize("count,labels", [(2, LABEL_SETS[2]), (8, LABEL_SETS[0]), (32, LABEL_SETS[1]), (2, LABEL_SETS[0]), (8, LABEL_SETS[1]), (32, LABEL_SETS[2])])
def test_joint_opening_verify_against_the_model(ctx, sbn, count, labels):
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
    tp = Transcript(b"joint verify gpu")
    ch, _, proof, _, _ = pm.prove_single(tp, gens, Z, r, evals, rnd, labels)
    comm_pts = pm.commit_poly(gens, Z, None, ell)
    tampered = list(evals); tampered[count // 2] = (tampered[count // 2] + 1) % R_MOD
    comm = ctx.bases_upload(b"".join(comm_pts))
    try:
        for ev, want in ((evals, True), (tampered, False)):
            tm = Transcript(b"joint verify gpu")
            assert sem.joint_verify(tm, proof, gens, r, ev, comm_pts, labels) == want
            tr = sbn.Transcript(b"joint verify gpu")
            before = tr.state()
            acc, got_ch = ctx.joint_opening_verify(bases, comm, _sbs(ev), labels, _sbs(r), pm.proof_bytes(proof), tr)
            assert acc == want
            assert got_ch == _sbs(_challenges(ev, labels)) and (not want or got_ch == _sbs(ch))
            assert tr.state() == (tm.state() if want else before)
            assert not want or tr.state() == tp.state()
    finally:
        comm.free()


# ---- in place: the openings inside the one-call provers' proofs ------------------------------------------------------------------------

def _device_joint_verify(ctx, sbn, handles):
    """sparse_eval_model.joint_verify with the device behind it: the model's transcript goes in and comes out through its state record"""
    def joint_verify(tr, proof, gens, r, evals, comm_C, labels):
        kind = {sem.DEREFS_LABELS: "derefs", sem.OPS_LABELS: "ops", sem.MEM_LABELS: "mem"}[labels]
        comm = ctx.bases_from_compressed(b"".join(ol.g1_compress(c) for c in comm_C))
        dt = sbn.Transcript.from_state(tr.state())
        try:
            acc, _ = ctx.joint_opening_verify(handles[kind], comm, _sbs(evals), labels, _sbs(r), pm.proof_bytes(proof), dt)
            tr.s = Transcript.from_state(dt.state()).s
            return acc
        finally:
            comm.free()
    return joint_verify


def test_in_place_in_a_sparse_eval_proof(ctx, sbn, monkeypatch):
    """sparse_eval_model.verify on a proof of sbn_sparse_eval_prove, its three joint_verify calls replaced by the device call"""
    shape_key = sem.SHAPES[0]
    nx, ny, _ = shape_key
    mats, rx, ry, evals, rnd = sem.instance(shape_key)
    shape = sem.Shape(nx, ny, dm.num_ops(mats), len(mats))
    made = {kd: ctx.gens_new(shape.R(kd) + 1, LABEL + b"_" + kd.encode()) for kd in ("ops", "mem", "derefs")}
    handles = {kd: made[kd][0] for kd in made}
    gens = sem.make_gens({kd: made[kd][1] for kd in made}, shape)
    dense = ctx.dense_build(nx, ny, [(r_, c_, _sbs(v)) for r_, c_, v in mats])
    try:
        tr = sbn.Transcript(b"sparse eval verify")
        proof_b = ctx.sparse_eval_prove(dense, _sbs(rx), _sbs(ry), _sbs(evals), handles["ops"], handles["mem"], handles["derefs"], _sbs(rnd), tr)
        md = dm.Dense(nx, ny, mats)
        proof, comm = sem.proof_from_bytes(proof_b, shape), sem.commit_dense(md, gens, shape)
        tm = Transcript(b"sparse eval verify")
        assert sem.verify(tm, proof, comm, md.N, md.cells, rx, ry, evals, gens)      # the all-model run
        calls = []
        dev = _device_joint_verify(ctx, sbn, handles)
        monkeypatch.setattr(sem, "joint_verify", lambda *a: calls.append(a[-1]) or dev(*a))
        td = Transcript(b"sparse eval verify")
        assert sem.verify(td, proof, comm, md.N, md.cells, rx, ry, evals, gens)
        assert calls == [sem.DEREFS_LABELS, sem.OPS_LABELS, sem.MEM_LABELS]
        assert td.state() == tm.state() == tr.state()
    finally:
        dense.free()
        for h in handles.values():
            h.free()


def test_in_place_in_an_r1cs_proof(ctx, sbn, monkeypatch):
    """r1cs_proof_model.verify on a proof of sbn_r1cs_proof_prove, the opening checked by the device: comm_vars from the proof's bytes,
    comm_vars_at_ry as C_Zr"""
    nc, nv, n_in = 8, 4, 3
    R = 1 << pm.factored_lens(rpm.log2(nv))[1]
    pc, pc_xy = ctx.gens_new(R + 1, LABEL + b"_pc")
    g3, g3_xy = ctx.gens_new(3, LABEL + b"_sc")
    g4, g4_xy = ctx.gens_new(4, LABEL + b"_sc")
    gens = rpm.make_gens(pc_xy, R, g3_xy, g4_xy)
    mats, vars_, inputs = rpm.satisfying_instance(nc, nv, n_in, 77)
    rnd = rpm.random_rnd(nc, nv, 78)
    import r1cs_model as rm
    inst = ctx.r1cs_upload(nc, nv, [(r_, c_, rm.to_bytes(v)) for r_, c_, v in mats])
    vt = ctx.table_upload(_sbs(vars_))
    try:
        tr = sbn.Transcript(b"r1cs verify")
        proof_b, _, _ = ctx.r1cs_proof_prove(inst, vt, _sbs(inputs), pc, g3, g4, _sbs(rnd), tr)
        proof = rpm.proof_from_bytes(proof_b, nc, nv)
        tm = Transcript(b"r1cs verify")
        assert rpm.verify_instance(tm, proof, nc, nv, mats, inputs, gens) is not None       # the all-model run
        lo, hi = rpm.field_spans(nc, nv)["comm_vars"]
        calls = []

        def device_verify(t, opening, gens_pc, r, C_Zr, comm_C):
            calls.append(len(comm_C))
            comm = ctx.bases_from_compressed(proof_b[lo:hi])
            dt = sbn.Transcript.from_state(t.state())
            try:
                assert ctx.bases_download(comm, 0, len(comm_C)) == b"".join(comm_C)
                acc = ctx.polyeval_verify(pc, comm, _sbs(r), pm.proof_bytes(opening), dt, C_Zr_xy=C_Zr)
                t.s = Transcript.from_state(dt.state()).s
                return acc
            finally:
                comm.free()
        monkeypatch.setattr(rpm.pm, "verify", device_verify)
        td = Transcript(b"r1cs verify")
        assert rpm.verify_instance(td, proof, nc, nv, mats, inputs, gens) is not None
        assert calls == [hi // 32 - lo // 32]
        assert td.state() == tm.state() == tr.state()
    finally:
        vt.free(); inst.free()
        for b in (pc, g3, g4):
            b.free()


# ---- prover sizes ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("ell,with_blinds", [(20, False), (25, True)])      # R_size 1024 and 8192, L_size 1024 and 4096
def test_polyeval_verify_at_prover_sizes(ctx, sbn, ell, with_blinds):
    """built as test_polyeval_prove_at_prover_sizes builds them: a synthetic table on the device, the commitment by the device's row commit"""
    rng = random.Random(ell)
    ml, mr = pm.factored_lens(ell)
    n = 1 << mr
    bases, _ = _gens(ctx, n)
    N = 1 << ell
    mem = ctx.dev_alloc(32 * N)
    ctx.scalars_synthetic(0x9e1e + ell, 0, N, mem)
    Zt = ctx.table_from_dev(mem, N)
    r = _sbs([rng.randrange(R_MOD) for _ in range(ell)])
    blinds = _sbs([rng.randrange(R_MOD) for _ in range(1 << ml)]) if with_blinds else None
    blind_Zr = pm.sb(rng.randrange(R_MOD)) if with_blinds else None
    rnd = _sbs([rng.randrange(R_MOD) for _ in range(3 + 2 * mr)])
    Zr = ctx.table_evaluate(Zt, r)
    tr, tv = sbn.Transcript(TR), sbn.Transcript(TR)
    Gn = G1 = comm = None
    try:
        proof, _, Cy = ctx.polyeval_prove(bases, Zt, r, Zr, rnd, tr, blinds=blinds, blind_Zr=blind_Zr)
        Gn, G1 = ctx.bases_split_at(bases, n)
        comm_xy, _ = ctx.commit_table(Gn, Zt, blinds, 1 << ml, n)
        comm = ctx.bases_upload(comm_xy)
        before = tv.state()
        z1 = (pm.ib(proof[64 * mr + 64:64 * mr + 96]) + 1) % R_MOD
        bad = proof[:64 * mr + 64] + pm.sb(z1) + proof[64 * mr + 96:]
        assert not ctx.polyeval_verify(bases, comm, r, bad, tv, C_Zr_xy=Cy) and tv.state() == before
        assert ctx.polyeval_verify(bases, comm, r, proof, tv, C_Zr_xy=Cy)
        assert tv.state() == tr.state()
        if not with_blinds:
            tp = sbn.Transcript(TR)
            assert ctx.polyeval_verify(bases, comm, r, proof, tp, Zr=Zr) and tp.state() == tr.state()
    finally:
        for b in (Gn, G1, comm):
            if b is not None:
                b.free()
        Zt.free(); ctx.dev_free(mem)
