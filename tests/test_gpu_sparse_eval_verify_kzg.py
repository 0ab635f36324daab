"""GPU: sbn_sparse_eval_verify_kzg — the KZG build's SparseMatPolyEvalProof::verify (sparse_mlpoly_full.rs:1815-1845 with DerefsEvalProof::verify,
:552-595) in one call — against the literal verifier of tests/sparse_eval_kzg_model.py: what it accepts (the device prover's bytes with and without a
derefs key, the model's bytes) with the transcript's end state; what it refuses, field by field, with the transcript untouched and the honest proof
accepted behind it; wrong verifier inputs; misuse; launches; a larger proof.  The SRS comes from the fixture's tau, so the model's KZG step is the
G1 relation; where a KZG field is tampered with, the pairing model (tests/pairing_model.py) is asked as well and must agree."""
import ctypes as C

import numpy as np
import pytest

from conftest import golden
import dense_model as dm
import oracle_lib as ol
import pairing_model as pmod
import polyeval_model as pm
import r1cs_model as rm
import sparse_eval_loop as loop
import sparse_eval_kzg_model as skm
import sparse_eval_model as sem
from sparse_eval_model import R, Transcript

pytestmark = pytest.mark.gpu
KAT = golden("pairing_kat.json")
TAU = int(KAT["tau"], 16)
LABEL = b"gens_sparse_verify_kzg_gpu"
TR_LABEL = b"sparse verify kzg gpu"
KINDS = skm.KINDS
TAMPER_SHAPES = [(2, 3, (3, 4, 1)), (2, 2, (4, 4, 4, 4))]
_GENS, _CASES, _SRS = {}, {}, {}


def _sbs(xs):
    return b"".join(pm.sb(x) for x in xs)


def _gens(ctx, shape, label=LABEL, points=True):
    key = (tuple(shape.lg[k] for k in KINDS), label)
    if key not in _GENS:
        made = {k: ctx.gens_new(shape.R(k) + 1, label + b"_" + k.encode(), want_points=points) for k in KINDS}
        _GENS[key] = ({k: made[k][0] for k in KINDS}, {k: pm.split_gens(made[k][1], shape.R(k)) for k in KINDS} if points else None)
    return _GENS[key]


def _srs(ctx, n):
    if n not in _SRS:
        _SRS[n] = ctx.kzg_srs_from_tau(_sbs([TAU]), n)
    return _SRS[n]


@pytest.fixture(scope="module")
def g2h(ctx):
    hs = {k: ctx.g2_prepare(bytes.fromhex(KAT["g2"][k])) for k in ("gen", "tau", "tau1")}
    yield hs
    for h in hs.values():
        h.free()


@pytest.fixture(scope="module", autouse=True)
def _free_handles():
    yield
    for handles, _ in _GENS.values():
        for h in handles.values():
            h.free()
    for c in _CASES.values():
        for h in c["comm_h"]:
            h.free()
    for s in _SRS.values():
        s.free()
    _GENS.clear(); _CASES.clear(); _SRS.clear()


def case(ctx, shape_key, seed=0):
    """one honest model proof per (shape, seed) for the whole module"""
    key = (shape_key, seed)
    if key not in _CASES:
        nx, ny, _ = shape_key
        mats, rx, ry, evals, rnd = skm.instance(shape_key, seed)
        dense = dm.Dense(nx, ny, mats)
        shape = sem.Shape(nx, ny, dense.N, dense.batch)
        handles, gens = _gens(ctx, shape)
        srs_n = (1 << shape.ell["derefs"]) + 1
        tp = Transcript(TR_LABEL)
        data = skm.proof_bytes(skm.prove(tp, nx, ny, mats, rx, ry, evals, gens, skm.Srs(TAU, srs_n), rnd))
        comm = (pm.commit_poly(gens["ops"], dense.comb_ops, None, shape.ell["ops"]), pm.commit_poly(gens["mem"], dense.comb_mem, None, shape.ell["mem"]))
        _CASES[key] = dict(nx=nx, ny=ny, mats=mats, rx=rx, ry=ry, evals=evals, rnd=rnd, shape=shape, handles=handles, gens=gens, data=data, state=tp.state(),
                           dense=dense, srs_n=srs_n, comm=comm, comm_h=[ctx.bases_upload(b"".join(comm[0])), ctx.bases_upload(b"".join(comm[1]))])
    return _CASES[key]


def device_verify(ctx, sbn, g2h, c, data=None, rx=None, evals=None, comm_h=None, g2="gen", tau_g2="tau"):
    """-> (accepted, the transcript's state behind the call, its state before)"""
    s, h, ch = c["shape"], c["handles"], comm_h or c["comm_h"]
    tr = sbn.Transcript(TR_LABEL)
    before = tr.state()
    ok = ctx.sparse_eval_verify_kzg(c["nx"], c["ny"], s.N, s.cells, s.b, ch[0], ch[1], _sbs(c["rx"] if rx is None else rx), _sbs(c["ry"]), _sbs(c["evals"] if evals is None else evals),
                                    h["ops"], h["mem"], g2h[g2], g2h[tau_g2], c["data"] if data is None else data, tr)
    return ok, tr.state(), before


def model_verify(c, data=None, rx=None, evals=None, comm=None, tau=TAU, pairing=False):
    """the literal verdict on bytes -> (accepted, state).  pairing: every KZG step is also put to the pairing model, which must agree"""
    proof = skm.proof_from_bytes(c["data"] if data is None else data, c["shape"])
    if proof is None:
        return False, None
    tv = Transcript(TR_LABEL)
    g1_rel = skm.kzg_verify
    if pairing:
        def both(Cb, z, y, pi, srs):
            want = g1_rel(Cb, z, y, pi, srs)
            pt = pmod.g1_from_bytes
            assert pmod.kzg_check(pt(Cb), z, y, pt(pi), pmod.G2, pmod.g2_mul(pmod.G2, srs.tau), pmod.schedule_naf()) == want
            return want
        skm.kzg_verify = both
    try:
        s = c["shape"]
        ok = skm.verify(tv, proof, comm or c["comm"], s.N, s.cells, c["rx"] if rx is None else rx, c["ry"], c["evals"] if evals is None else evals, c["gens"], skm.Srs(tau, c["srs_n"]))
    finally:
        skm.kzg_verify = g1_rel
    return ok, tv.state()


@pytest.mark.parametrize("shape_key", sem.SHAPES)
def test_accepts_the_provers_and_the_models_bytes(ctx, sbn, g2h, shape_key):
    c = case(ctx, shape_key)
    want = model_verify(c, pairing=shape_key == sem.SHAPES[0])
    assert want == (True, c["state"])
    assert device_verify(ctx, sbn, g2h, c)[:2] == want
    srs = _srs(ctx, c["srs_n"])
    dense = ctx.dense_build(c["nx"], c["ny"], [(r, cc, _sbs(v)) for r, cc, v in c["mats"]])
    try:
        for with_key in (False, True):
            key = ctx.derefs_key_build(dense, srs) if with_key else None
            tp = sbn.Transcript(TR_LABEL)
            try:
                proof = ctx.sparse_eval_prove_kzg(dense, _sbs(c["rx"]), _sbs(c["ry"]), _sbs(c["evals"]), c["handles"]["ops"], c["handles"]["mem"], srs, key, _sbs(c["rnd"]), tp)
            finally:
                if key is not None:
                    key.free()
            assert proof == c["data"]
            assert device_verify(ctx, sbn, g2h, c, data=proof)[:2] == (True, tp.state()) and tp.state() == c["state"]
    finally:
        dense.free()


def _bad_point(comp):
    """a compressed point near `comp` that does not decompress"""
    flags = comp[31] & 0x80
    x = int.from_bytes(comp, "little") & ((1 << 254) - 1)
    while True:
        x += 1
        cand = bytearray(x.to_bytes(32, "little")); cand[31] |= flags
        if ol.g1_decompress(bytes(cand)) is None:
            return bytes(cand)


KZG_FIELDS = ("comm_derefs", "hash.proof_derefs")


def tamperings(c):
    """{name: (data, a KZG field?)} — every change of the proof's bytes the check must refuse"""
    data, sp = c["data"], skm.field_spans(c["shape"])
    out = {}
    for f in skm.FIELDS:                                            # the lowest byte of the field's last element (comm_derefs: of its point; proof_derefs: of eval)
        lo, hi = sp[f]
        b = bytearray(data); b[hi - 32] ^= 1
        out["flipped byte in " + f] = (bytes(b), f in KZG_FIELDS)
    lo, hi = sp["hash.proof_derefs"]
    b = bytearray(data); b[lo] ^= 1
    out["flipped byte in the point of hash.proof_derefs"] = (bytes(b), True)
    for f in ("prod.proof_ops", "prod.proof_mem", "hash.eval_row", "hash.proof_ops", "hash.proof_mem", "hash.proof_derefs"):
        lo, hi = sp[f]
        b = bytearray(data); b[hi - 32:hi] = R.to_bytes(32, "little")
        out["scalar = r in " + f] = (bytes(b), False)
    spots = {"comm_derefs": sp["comm_derefs"][0], "pi of hash.proof_derefs": sp["hash.proof_derefs"][0]}
    for f in ("hash.proof_ops", "hash.proof_mem"):
        spots["L[0] of " + f] = sp[f][0]
        spots["beta of " + f] = sp[f][1] - 96
    for name, at in spots.items():
        b = bytearray(data); b[at:at + 32] = _bad_point(data[at:at + 32])
        out["no point at " + name] = (bytes(b), False)
    return out


@pytest.mark.parametrize("shape_key", TAMPER_SHAPES)
def test_refuses_what_the_literal_verdict_refuses_and_then_accepts_again(ctx, sbn, g2h, shape_key):
    c = case(ctx, shape_key)
    honest = (True, c["state"])
    t = tamperings(c)
    assert len(t) == 13 + 1 + 6 + 6
    for name, (data, kzg_field) in t.items():
        assert model_verify(c, data=data, pairing=kzg_field)[0] is False, name
        ok, state, before = device_verify(ctx, sbn, g2h, c, data=data)
        assert ok is False and state == before, name
        assert device_verify(ctx, sbn, g2h, c)[:2] == honest, name


@pytest.mark.parametrize("shape_key", TAMPER_SHAPES)
def test_refuses_wrong_inputs_of_the_verifier(ctx, sbn, g2h, shape_key):
    c = case(ctx, shape_key)
    other = case(ctx, shape_key, seed=1)
    honest = (True, c["state"])
    trials = []
    for i in range(c["shape"].b):
        wrong = list(c["evals"]); wrong[i] = (wrong[i] + 1) % R
        trials.append(("evals[%d]" % i, dict(evals=wrong), dict(evals=wrong)))
    wrx = list(c["rx"]); wrx[0] = (wrx[0] + 1) % R
    trials.append(("rx[0]", dict(rx=wrx), dict(rx=wrx)))
    trials.append(("comm_ops of another instance", dict(comm_h=[other["comm_h"][0], c["comm_h"][1]]), dict(comm=(other["comm"][0], c["comm"][1]))))
    trials.append(("comm_mem of another instance", dict(comm_h=[c["comm_h"][0], other["comm_h"][1]]), dict(comm=(c["comm"][0], other["comm"][1]))))
    trials.append(("the SRS of tau + 1", dict(tau_g2="tau1"), dict(tau=(TAU + 1) % R)))
    for name, dev, mod in trials:
        assert model_verify(c, **mod)[0] is False, name
        ok, state, before = device_verify(ctx, sbn, g2h, c, **dev)
        assert ok is False and state == before, name
        assert device_verify(ctx, sbn, g2h, c)[:2] == honest, name
    # the two G2 handles swapped: e(L, tau g2) e(-pi, g2) is one only by accident
    ok, state, before = device_verify(ctx, sbn, g2h, c, g2="tau", tau_g2="gen")
    assert ok is False and state == before
    assert device_verify(ctx, sbn, g2h, c)[:2] == honest


def test_misuse_is_einval_and_launches_nothing(ctx, sbn, g2h):
    c = case(ctx, (2, 3, (3, 4, 1)))
    s, h, ch = c["shape"], c["handles"], c["comm_h"]
    L = sbn.lib()
    tr = sbn.Transcript(TR_LABEL)
    before = tr.state()
    rx, ry, ev = _sbs(c["rx"]), _sbs(c["ry"]), _sbs(c["evals"])
    no_h = ctx.bases_upload(ol.gens_new(s.R("ops") + 1, b"no h")[0][:64 * (s.R("ops") + 1)])
    big = R.to_bytes(32, "little")
    fresh = sbn.Context(0)
    foreign = fresh.g2_prepare(bytes.fromhex(KAT["g2"]["gen"]))
    seen = []

    def call(nx=c["nx"], ny=c["ny"], N=s.N, cells=s.cells, b=s.b, co=ch[0].h, cm=ch[1].h, rx=rx, ry=ry, ev=ev, go=h["ops"].h, gm=h["mem"].h, g2=g2h["gen"].h, tg2=g2h["tau"].h,
             proof=c["data"], t=tr.h, acc=True):
        a = C.c_int(7)
        p = lambda x: None if x is None else (C.c_uint8 * len(x)).from_buffer_copy(x)      # noqa: E731
        rc = L.sbn_sparse_eval_verify_kzg(ctx.h, C.c_size_t(nx), C.c_size_t(ny), C.c_size_t(N), C.c_size_t(cells), C.c_size_t(b), co, cm, p(rx), p(ry), p(ev), go, gm, g2, tg2, p(proof), t,
                                          C.byref(a) if acc else None)
        seen.append(a.value)
        return rc
    ctx.prof_enable(True)
    try:
        ctx.prof_reset()
        bad = [dict(co=None), dict(cm=None), dict(rx=None), dict(ry=None), dict(ev=None), dict(go=None), dict(gm=None), dict(g2=None), dict(tg2=None), dict(proof=None), dict(t=None),
               dict(acc=False), dict(b=0), dict(b=5), dict(N=1), dict(N=3), dict(N=0), dict(cells=2 * s.cells), dict(cells=s.cells // 2),
               dict(co=ch[1].h), dict(cm=ch[0].h), dict(go=h["mem"].h), dict(gm=h["ops"].h), dict(go=no_h.h), dict(g2=foreign.h), dict(tg2=foreign.h),
               dict(rx=big + rx[32:]), dict(ry=ry[:-32] + big), dict(ev=big + ev[32:])]
        assert len(ch[0]) != len(ch[1]) and len(h["mem"]) != len(h["ops"])
        for kw in bad:
            assert call(**kw) == -1, kw
        assert set(seen) == {7}, "a refused call wrote its verdict"
        assert ctx.prof_get() == {}, "a refused call launched something"
        assert tr.state() == before
    finally:
        ctx.prof_enable(False)
        no_h.free(); foreign.free(); fresh.close()
    assert device_verify(ctx, sbn, g2h, c)[:2] == (True, c["state"])


@pytest.mark.parametrize("shape_key", [(1, 1, (2, 2, 2)), (2, 3, (3, 4, 1)), (2, 2, (4, 4, 4, 4))])
def test_launch_counts(ctx, sbn, g2h, shape_key):
    """what the header states: one decompress launch and three hand-overs for the two Hyrax openings and their final equations, then the two KZG
    points' decompression, the G1 sum's launch and hand-over, and one pairing launch: six host waits"""
    c = case(ctx, shape_key)
    device_verify(ctx, sbn, g2h, c)                                 # (the derived sets are built by now)
    ctx.prof_enable(True)
    try:
        ctx.prof_reset()
        assert device_verify(ctx, sbn, g2h, c)[0]
        prof = {k: v[1] for k, v in ctx.prof_get().items()}
    finally:
        ctx.prof_enable(False)
    assert prof["k_g1_decompress"] == 2 and prof["k_window_sums"] == 4 and prof["k_sums_to_host"] == 4 and prof["k_pairing_products"] == 1
    assert prof["k_polyeval_eq"] == 2 and prof["k_polyeval_verify_row"] == 2 and "k_points_to_host" not in prof and "k_pow2_table" not in prof


def test_accepts_a_proof_of_the_device_prover_at_lg_n_10(ctx, sbn, g2h):
    lg_n = 10
    nx = ny = lg_n
    N, b = 1 << lg_n, 3
    shape = sem.Shape(nx, ny, N, b)
    handles, _ = _gens(ctx, shape, LABEL + b"_big", points=False)
    srs = _srs(ctx, 1 << shape.ell["derefs"])
    rng = np.random.default_rng(lg_n)
    dense = ctx.dense_build(nx, ny, loop.random_mats(nx, ny, N, b, 70 + lg_n))
    rx, ry = rm.random_vals(rng, nx).tobytes(), rm.random_vals(rng, ny).tobytes()
    rnd = rm.random_vals(rng, skm.sizes(nx, ny, N, b)[0]).tobytes()
    comm_h, splits = [], []
    try:
        evals = loop.evals_of(sbn, ctx, dense, rx, ry)
        tp = sbn.Transcript(TR_LABEL)
        proof = ctx.sparse_eval_prove_kzg(dense, rx, ry, evals, handles["ops"], handles["mem"], srs, None, rnd, tp)
        for kind, tab in (("ops", dense.comb_ops), ("mem", dense.comb_mem)):
            Gn, G1 = ctx.bases_split_at(handles[kind], shape.R(kind))
            splits += [Gn, G1]
            xy, _ = ctx.commit_table(Gn, tab, None, 1 << pm.factored_lens(shape.ell[kind])[0], shape.R(kind))
            comm_h.append(ctx.bases_upload(xy))
        args = (nx, ny, N, 1 << nx, b, comm_h[0], comm_h[1], rx, ry, evals, handles["ops"], handles["mem"], g2h["gen"], g2h["tau"])
        tv = sbn.Transcript(TR_LABEL)
        assert ctx.sparse_eval_verify_kzg(*args, proof, tv)
        assert tv.state() == tp.state()
        bad = bytearray(proof); bad[-32] ^= 1                       # eval of the derefs opening: only the pairing product can tell
        tb = sbn.Transcript(TR_LABEL)
        assert not ctx.sparse_eval_verify_kzg(*args, bytes(bad), tb)
        assert tb.state() == sbn.Transcript(TR_LABEL).state()
    finally:
        for h in comm_h + splits:
            h.free()
        dense.free()
