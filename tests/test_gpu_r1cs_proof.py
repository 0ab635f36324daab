"""GPU: sbn_r1cs_proof_prove — R1CSProof::prove (r1csproof.rs:241-459) in one call — against the literal model of the reference
(tests/r1cs_proof_model.py), against the same proof assembled from the entry points that existed before it (tests/r1cs_proof_loop.py), and its
edge cases, state and refusals.  Every comparison is bit-exact."""
import ctypes as C
import random

import numpy as np
import pytest

import polyeval_model as pm
import r1cs_model as rm
import r1cs_proof_loop as loop
import r1cs_proof_model as rpm
import zk_sumcheck_model as zm
from r1cs_proof_model import R_MOD, Transcript

pytestmark = pytest.mark.gpu
SHAPES = [(2, 2, 0), (2, 2, 1), (4, 4, 1), (8, 4, 3), (4, 8, 0), (64, 4, 2), (2, 64, 5), (16, 16, 15)]
LABEL = b"gens_r1cs_proof_gpu"
TR_LABEL = b"r1cs proof gpu"
_GENS = {}


def _sbs(xs):
    return b"".join(zm.sb(x) for x in xs)


def _R(nv):
    return 1 << pm.factored_lens(rpm.log2(nv))[1]


def _gens(ctx, R, label=LABEL, points=True):
    """(gens_pc, gens_3, gens_4 handles, the model's gens dict) per size and label for the whole module: the derived sets are built once"""
    key = (R, label)
    if key not in _GENS:
        pc, pc_xy = ctx.gens_new(R + 1, label + b"_pc")
        g3, g3_xy = ctx.gens_new(3, label + b"_sc")
        g4, g4_xy = ctx.gens_new(4, label + b"_sc")
        _GENS[key] = (pc, g3, g4, rpm.make_gens(pc_xy, R, g3_xy, g4_xy))
    return _GENS[key]


@pytest.fixture(scope="module", autouse=True)
def _free_gens():
    yield
    for pc, g3, g4, _ in _GENS.values():
        pc.free(); g3.free(); g4.free()
    _GENS.clear()


def _upload(ctx, nc, nv, mats):
    return ctx.r1cs_upload(nc, nv, [(r, c, rm.to_bytes(v)) for r, c, v in mats])


def _device(ctx, sbn, nc, nv, mats, vars_, inputs, handles, rnd, label=TR_LABEL):
    """-> ((proof, rx, ry), transcript state); asserts that vars is left as it was"""
    pc, g3, g4 = handles
    inst = _upload(ctx, nc, nv, mats)
    vt = ctx.table_upload(_sbs(vars_))
    tr = sbn.Transcript(label)
    try:
        out = ctx.r1cs_proof_prove(inst, vt, _sbs(inputs), pc, g3, g4, _sbs(rnd), tr)
        assert len(vt) == nv and ctx.table_download(vt) == _sbs(vars_)
        return out, tr.state()
    finally:
        vt.free(); inst.free()


_MODEL = {}


def _model(shape, gens, seed=0, mats_vars_inputs=None, rnd=None):
    key = (shape, seed)
    if key not in _MODEL:
        nc, nv, n_in = shape
        mats, vars_, inputs = mats_vars_inputs or rpm.satisfying_instance(nc, nv, n_in, 2000 + 64 * nc + nv + seed)
        rnd = rnd if rnd is not None else rpm.random_rnd(nc, nv, 7 * nc + nv + seed)
        tm = Transcript(TR_LABEL)
        proof, rx, ry = rpm.prove(tm, nc, nv, mats, vars_, inputs, gens, rnd)
        _MODEL[key] = (mats, vars_, inputs, rnd, rpm.proof_bytes(proof), _sbs(rx), _sbs(ry), tm.state())
    return _MODEL[key]


@pytest.mark.parametrize("shape", SHAPES)
def test_bit_exact_against_the_model(ctx, sbn, shape):
    """(2,2,*): ell = 1, L = 1; ell even and odd; num_cons far above and far below 2 num_vars; zero, one and num_vars - 1 inputs"""
    nc, nv, n_in = shape
    pc, g3, g4, gens = _gens(ctx, _R(nv))
    mats, vars_, inputs, rnd, want, want_rx, want_ry, want_state = _model(shape, gens)
    (proof, rx, ry), state = _device(ctx, sbn, nc, nv, mats, vars_, inputs, (pc, g3, g4), rnd)
    assert rx == want_rx and ry == want_ry
    assert proof == want
    assert state == want_state
    tv = Transcript(TR_LABEL)
    got = rpm.verify_instance(tv, rpm.proof_from_bytes(proof, nc, nv), nc, nv, mats, inputs, gens)
    assert got is not None and (_sbs(got[0]), _sbs(got[1])) == (rx, ry) and tv.state() == state


# phase 1 starts at length num_cons, phase 2 at 2 num_vars: 2^10 .. 2^12 lie on both sides of the 2^9 | 2^10 | 2^11 switches of the fused round
# (q = len / 4, tests/test_gpu_zk_sumcheck.py); (2^16, 2^15) reaches the streaming k_sc_bind_eval_pf and a witness commit of 128 x 256
@pytest.mark.parametrize("nc,nv,n_in", [(1 << 11, 1 << 10, 3), (1 << 10, 1 << 11, 0), (1 << 16, 1 << 15, 5)])
def test_equals_the_loop_through_the_calls_that_existed_before(ctx, sbn, nc, nv, n_in):
    R = _R(nv)
    pc, g3, g4, _ = _gens(ctx, R)
    rng = np.random.default_rng(nc + nv)
    mats = loop.random_instance(nc, nv, nc * 3 + nv)
    vars_b = rm.random_vals(rng, nv).tobytes()
    input_b = rm.random_vals(rng, n_in).tobytes() if n_in else b""
    rnd = rm.random_vals(rng, rpm.sizes(nc, nv)[0]).tobytes()
    inst = ctx.r1cs_upload(nc, nv, mats)
    vt = ctx.table_upload(vars_b)
    lg = loop.LoopGens(ctx, pc, R)
    try:
        t1, t2 = sbn.Transcript(TR_LABEL), sbn.Transcript(TR_LABEL)
        one = ctx.r1cs_proof_prove(inst, vt, input_b, pc, g3, g4, rnd, t1)
        assert ctx.table_download(vt) == vars_b
        many = loop.prove_loop(sbn, ctx, inst, vt, vars_b, input_b, pc, lg, g3, g4, rnd, t2)
        assert one[1] == many[1] and one[2] == many[2]
        assert one[0] == many[0]
        assert t1.state() == t2.state()
    finally:
        lg.free(); vt.free(); inst.free()


def test_an_unsatisfied_instance_gives_the_models_bytes_and_is_rejected(ctx, sbn):
    shape = (8, 4, 3)
    nc, nv, n_in = shape
    pc, g3, g4, gens = _gens(ctx, _R(nv))
    (A, B, (cr, cc, cv)), vars_, inputs = rpm.satisfying_instance(nc, nv, n_in, 77)
    bad = (A, B, (cr, cc, [(cv[0] + 1) % R_MOD] + cv[1:]))
    mats, vars_, inputs, rnd, want, want_rx, want_ry, want_state = _model(shape, gens, seed=1, mats_vars_inputs=(bad, vars_, inputs))
    (proof, rx, ry), state = _device(ctx, sbn, nc, nv, mats, vars_, inputs, (pc, g3, g4), rnd)
    assert (proof, rx, ry, state) == (want, want_rx, want_ry, want_state)
    assert rpm.verify_instance(Transcript(TR_LABEL), rpm.proof_from_bytes(proof, nc, nv), nc, nv, mats, inputs, gens) is None


def test_all_zero(ctx, sbn):
    """empty matrices, a zero witness, zero randomness, no inputs: every claim, blind and polynomial is zero — the constant one of z meets only
    zeros of evals_ABC — so every commitment of the proof is the identity"""
    shape = (4, 4, 0)
    nc, nv, _ = shape
    pc, g3, g4, gens = _gens(ctx, _R(nv))
    empty = (([], [], []),) * 3
    mats, vars_, inputs, rnd, want, want_rx, want_ry, want_state = _model(shape, gens, seed=2, mats_vars_inputs=(empty, [0] * nv, []), rnd=[0] * rpm.sizes(nc, nv)[0])
    (proof, rx, ry), state = _device(ctx, sbn, nc, nv, mats, vars_, inputs, (pc, g3, g4), rnd)
    assert (proof, rx, ry, state) == (want, want_rx, want_ry, want_state)
    ident = sbn.g1_compress(bytes(64))
    p = rpm.proof_from_bytes(proof, nc, nv)
    points = p["comm_vars"] + list(p["claims_phase2"]) + [p["pok_claims_phase2"][0]["alpha"], p["comm_vars_at_ry"], p["proof_eq_sc_phase1"]["alpha"], p["proof_eq_sc_phase2"]["alpha"]]
    points += [p["pok_claims_phase2"][1][k] for k in ("alpha", "beta", "delta")] + p["proof_eval_vars_at_ry"]["L"] + p["proof_eval_vars_at_ry"]["R"]
    points += [p["proof_eval_vars_at_ry"][k] for k in ("delta", "beta")]
    for sc in (p["sc_proof_phase1"], p["sc_proof_phase2"]):
        points += sc["comm_polys"] + sc["comm_evals"] + [d[k] for d in sc["proofs"] for k in ("delta", "beta")]
    assert all(sbn.g1_compress(q) == ident for q in points)
    spans = rpm.field_spans(nc, nv)
    lo, hi = spans["comm_vars"]
    assert proof[lo:hi] == ident * ((hi - lo) // 32)


def test_results_do_not_depend_on_what_the_handles_ran_before(ctx, sbn):
    """two proves with different generator labels on one context, then the standalone opening and phase-2 sumcheck on the same gens_pc / gens_3
    handles, then the first prove again: the derived handles and sets are shared, not rebuilt or confused"""
    sa, sb_ = (4, 8, 0), (8, 4, 3)
    ha = _gens(ctx, _R(8), LABEL + b"_state_a")
    hb = _gens(ctx, _R(4), LABEL + b"_state_b")
    ma = rpm.satisfying_instance(*sa, 31); mb = rpm.satisfying_instance(*sb_, 32)
    ra, rb = rpm.random_rnd(sa[0], sa[1], 33), rpm.random_rnd(sb_[0], sb_[1], 34)
    first = _device(ctx, sbn, sa[0], sa[1], *ma, ha[:3], ra)
    second = _device(ctx, sbn, sb_[0], sb_[1], *mb, hb[:3], rb)
    tm = Transcript(TR_LABEL)
    pb, rxb, ryb = rpm.prove(tm, sb_[0], sb_[1], *mb, hb[3], rb)
    assert second == ((rpm.proof_bytes(pb), _sbs(rxb), _sbs(ryb)), tm.state())

    def standalone(c, pc, g3):
        """sbn_polyeval_prove and sbn_zk_sumcheck_prove_quad at the shape of the first prove"""
        rng = random.Random(35)
        ell, R = 3, _R(8)
        Z = [rng.randrange(R_MOD) for _ in range(8)]
        r = [rng.randrange(R_MOD) for _ in range(ell)]
        rnd = [rng.randrange(R_MOD) for _ in range(3 + 2 * 2)]
        zt = c.table_upload(_sbs(Z)); tr = sbn.Transcript(b"standalone")
        _, g1 = c.bases_split_at(pc, R)
        tabs = [[rng.randrange(R_MOD) for _ in range(16)] for _ in range(2)]
        ts = [c.table_upload(_sbs(t)) for t in tabs]
        try:
            o1 = c.polyeval_prove(pc, zt, _sbs(r), zm.sb(5), _sbs(rnd), tr)
            o2 = c.zk_sumcheck_prove_quad(ts[0], ts[1], g1, g3, zm.sb(zm.dot(*tabs)), zm.sb(9), _sbs([rng.randrange(R_MOD) for _ in range(4 * 7)]), tr)
            return o1, o2, tr.state()
        finally:
            zt.free(); g1.free()
            for t in ts:
                t.free()
    used = standalone(ctx, ha[0], ha[1])
    fresh_ctx = sbn.Context(0)
    try:
        pc, _ = fresh_ctx.gens_new(_R(8) + 1, LABEL + b"_state_a_pc", want_points=False)
        g3, _ = fresh_ctx.gens_new(3, LABEL + b"_state_a_sc", want_points=False)
        try:
            assert standalone(fresh_ctx, pc, g3) == used
        finally:
            pc.free(); g3.free()
    finally:
        fresh_ctx.close()
    assert _device(ctx, sbn, sa[0], sa[1], *ma, ha[:3], ra) == first


def test_refusals_leave_everything_as_it_was(ctx, sbn):
    shape = (8, 4, 3)
    nc, nv, n_in = shape
    R = _R(nv)
    pc, g3, g4, gens = _gens(ctx, R)
    mats, vars_, inputs, rnd, want, want_rx, want_ry, want_state = _model(shape, gens)
    n_rnd, n_proof = rpm.sizes(nc, nv)
    inst = _upload(ctx, nc, nv, mats)
    inst_nv1 = ctx.r1cs_upload(8, 1, [([], [], b"")] * 3)
    inst_nc1 = ctx.r1cs_upload(1, 4, [([], [], b"")] * 3)
    vt = ctx.table_upload(_sbs(vars_)); vt_long = ctx.table_upload(_sbs(vars_ + vars_)); vt_one = ctx.table_upload(zm.sb(3))
    pc_xy = ctx.bases_download(pc, 0, R + 2)
    pc_no_h = ctx.bases_upload(pc_xy[:64 * (R + 1)])
    pc_long, _ = ctx.gens_new(R + 2, LABEL + b"_pc", want_points=False)
    g3_no_h = ctx.bases_upload(ctx.bases_download(g3, 0, 3))
    g4_no_h = ctx.bases_upload(ctx.bases_download(g4, 0, 4))
    tr = sbn.Transcript(TR_LABEL)
    state0 = tr.state()
    big = R_MOD.to_bytes(32, "little")
    rnd_b, in_b = _sbs(rnd), _sbs(inputs)
    proof = (C.c_uint8 * n_proof)(); rx = (C.c_uint8 * 96)(); ry = (C.c_uint8 * 96)()

    def raw(**kw):
        a = dict(ctx=ctx.h, inst=inst.h, vars=vt.h, input=in_b, n_in=n_in, pc=pc.h, g3=g3.h, g4=g4.h, rnd=rnd_b, tr=tr.h, proof=proof, rx=rx, ry=ry)
        a.update(kw)
        return sbn.lib().sbn_r1cs_proof_prove(a["ctx"], a["inst"], a["vars"], a["input"], C.c_size_t(a["n_in"]), a["pc"], a["g3"], a["g4"], a["rnd"], a["tr"],
                                              a["proof"], a["rx"], a["ry"])
    cases = {k: {k: None} for k in ("inst", "vars", "input", "pc", "g3", "g4", "rnd", "tr", "proof", "rx", "ry")}      # a null pointer
    cases.update({
        "vars of the wrong length": dict(vars=vt_long.h),
        "num_vars = 1": dict(inst=inst_nv1.h, vars=vt_one.h, input=None, n_in=0),
        "num_cons = 1": dict(inst=inst_nc1.h),
        "num_inputs = num_vars": dict(input=in_b + zm.sb(1), n_in=nv),
        "gens_pc without h": dict(pc=pc_no_h.h),
        "gens_pc of the wrong length": dict(pc=pc_long.h),
        "gens_3 of the wrong size": dict(g3=g4.h),
        "gens_4 of the wrong size": dict(g4=g3.h),
        "gens_3 without h": dict(g3=g3_no_h.h),
        "gens_4 without h": dict(g4=g4_no_h.h),
        "rnd[0] >= r": dict(rnd=big + rnd_b[32:]),
        "rnd[last] >= r": dict(rnd=rnd_b[:-32] + big),
        "input[0] >= r": dict(input=big + in_b[32:]),
        "input[last] >= r": dict(input=in_b[:-32] + big),
    })
    try:
        assert raw(ctx=None) == -1
        for name, kw in cases.items():
            assert raw(**kw) == -1, name                    # SBN_EINVAL
            assert tr.state() == state0, name
            assert ctx.table_download(vt) == _sbs(vars_), name
        assert raw(input=in_b + zm.sb(1), n_in=nv) == -1 and b"r1csproof.rs:253" in sbn.lib().sbn_last_error(ctx.h)      # the text cites the reference's assert
        got = ctx.r1cs_proof_prove(inst, vt, in_b, pc, g3, g4, rnd_b, tr)
        assert got == (want, want_rx, want_ry) and tr.state() == want_state
    finally:
        for h in (inst, inst_nv1, inst_nc1, vt, vt_long, vt_one, pc_no_h, pc_long, g3_no_h, g4_no_h):
            h.free()


def test_sizes(sbn):
    for nc, nv, _ in SHAPES + [(1 << 11, 1 << 10, 0), (1 << 16, 1 << 15, 0), (1 << 20, 1 << 20, 0)]:
        assert sbn.r1cs_proof_sizes(nc, nv) == rpm.sizes(nc, nv)
    assert sbn.r1cs_proof_sizes(1 << 20, 1 << 20) == (1368, 46624)
    for nc, nv in ((4, 1), (1, 4), (6, 4), (4, 12), (0, 4), (4, 0)):
        with pytest.raises(sbn.SbnError):
            sbn.r1cs_proof_sizes(nc, nv)
