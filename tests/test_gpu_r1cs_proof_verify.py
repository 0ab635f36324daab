"""GPU: sbn_r1cs_proof_verify — R1CSProof::verify (r1csproof.rs:463-619) in one call — and sbn_zk_sumcheck_verify (sumcheck.rs:366-457) against the
literal models of the reference (tests/r1cs_proof_model.py, tests/zk_sumcheck_model.py): verdict, challenges and the 203-byte transcript state,
what they refuse, what is misuse, their launches and their independence of what the context ran before."""
import ctypes as C
import random

import numpy as np
import pytest

import polyeval_model as pm
import r1cs_model as rm
import r1cs_proof_model as rpm
import r1cs_proof_verify_model as vm
import zk_sumcheck_model as zm
from r1cs_proof_model import R_MOD, Transcript

pytestmark = pytest.mark.gpu
SHAPES = [(2, 2, 0), (2, 2, 1), (4, 4, 1), (8, 4, 3), (4, 8, 0), (64, 4, 2), (2, 64, 5), (16, 16, 15)]
TAMPER_SHAPE = (8, 4, 3)
LABEL = b"gens_r1cs_verify_gpu"
TR_LABEL = b"r1cs proof verify gpu"
_GENS, _MODEL = {}, {}


def _sbs(xs):
    return b"".join(zm.sb(x) for x in xs)


def _R(nv):
    return 1 << pm.factored_lens(rpm.log2(nv))[1]


def _gens(ctx, R, label=LABEL):
    """(gens_pc, gens_3, gens_4 handles, the model's gens dict) per size and label for the whole module"""
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


def _model(shape, gens, seed=0, mats_vars_inputs=None, rnd=None):
    """one model proof per (shape, seed) for the whole module, with the literal verifier's answer ->
    dict(mats, vars, inputs, rnd, proof, rx, ry, evals, state)"""
    key = (shape, seed)
    if key not in _MODEL:
        nc, nv, n_in = shape
        mats, vars_, inputs = mats_vars_inputs or rpm.satisfying_instance(nc, nv, n_in, 4000 + 64 * nc + nv + seed)
        rnd = rnd if rnd is not None else rpm.random_rnd(nc, nv, 13 * nc + nv + seed)
        tm = Transcript(TR_LABEL)
        proof, rx, ry = rpm.prove(tm, nc, nv, mats, vars_, inputs, gens, rnd)
        evals = rm.evaluate(nc, nv, mats, rx, ry)
        tv = Transcript(TR_LABEL)
        assert rpm.verify(tv, proof, nv, nc, inputs, evals, gens) == (rx, ry) and tv.state() == tm.state()
        _MODEL[key] = dict(mats=mats, vars=vars_, inputs=inputs, rnd=rnd, proof=rpm.proof_bytes(proof), rx=_sbs(rx), ry=_sbs(ry), evals=_sbs(evals), state=tm.state())
    return _MODEL[key]


def _prove(ctx, sbn, shape, m, handles):
    """sbn_r1cs_proof_prove on the model's instance -> ((proof, rx, ry), the prover's end state)"""
    nc, nv, _ = shape
    pc, g3, g4 = handles
    inst = ctx.r1cs_upload(nc, nv, [(r, c, rm.to_bytes(v)) for r, c, v in m["mats"]])
    vt = ctx.table_upload(_sbs(m["vars"]))
    tr = sbn.Transcript(TR_LABEL)
    try:
        return ctx.r1cs_proof_prove(inst, vt, _sbs(m["inputs"]), pc, g3, g4, _sbs(m["rnd"]), tr), tr.state()
    finally:
        vt.free(); inst.free()


def _verify(ctx, sbn, shape, m, handles, proof=None, evals=None, inputs=None):
    """-> ((rx, ry) or None, the transcript's state behind the call)"""
    nc, nv, _ = shape
    pc, g3, g4 = handles
    tr = sbn.Transcript(TR_LABEL)
    got = ctx.r1cs_proof_verify(nc, nv, _sbs(m["inputs"]) if inputs is None else inputs, m["evals"] if evals is None else evals, pc, g3, g4,
                                m["proof"] if proof is None else proof, tr)
    return got, tr.state()


@pytest.mark.parametrize("shape", SHAPES)
def test_accepts_the_provers_and_the_models_proofs(ctx, sbn, shape):
    """(2,2,*): one round of phase 1, L = 1; ell even and odd; num_cons far above and far below 2 num_vars; zero, one and num_vars - 1 inputs"""
    nc, nv, _ = shape
    pc, g3, g4, gens = _gens(ctx, _R(nv))
    m = _model(shape, gens)
    (proof, rx, ry), state = _prove(ctx, sbn, shape, m, (pc, g3, g4))
    assert (rx, ry, state) == (m["rx"], m["ry"], m["state"])
    for b in (proof, m["proof"]):
        got, end = _verify(ctx, sbn, shape, m, (pc, g3, g4), proof=b)
        assert got == (m["rx"], m["ry"])
        assert end == m["state"]


def test_accepts_a_proof_of_the_device_prover_at_2_11_by_2_10(ctx, sbn):
    """a satisfied instance above the 2^9 | 2^10 | 2^11 switches of the prover's fused round; A, B, C(rx, ry) from sbn_r1cs_evaluate"""
    nc, nv, n_in = 1 << 11, 1 << 10, 3
    pc, g3, g4, _ = _gens(ctx, _R(nv))
    mats, vars_, inputs = rpm.satisfying_instance(nc, nv, n_in, nc + nv)
    rng = np.random.default_rng(nc + nv)
    vars_b, input_b = _sbs(vars_), _sbs(inputs)
    rnd = rm.random_vals(rng, rpm.sizes(nc, nv)[0]).tobytes()
    inst = ctx.r1cs_upload(nc, nv, [(r, c, rm.to_bytes(v)) for r, c, v in mats])
    vt = ctx.table_upload(vars_b)
    try:
        tp, tv = sbn.Transcript(TR_LABEL), sbn.Transcript(TR_LABEL)
        proof, rx, ry = ctx.r1cs_proof_prove(inst, vt, input_b, pc, g3, g4, rnd, tp)
        evals = b"".join(ctx.r1cs_evaluate(inst, rx, ry))
        assert ctx.r1cs_proof_verify(nc, nv, input_b, evals, pc, g3, g4, proof, tv) == (rx, ry)
        assert tv.state() == tp.state()
        wrong = zm.sb((zm.ib(evals[:32]) + 1) % R_MOD) + evals[32:]
        state0 = tv.state()
        assert ctx.r1cs_proof_verify(nc, nv, input_b, wrong, pc, g3, g4, proof, tv) is None and tv.state() == state0
    finally:
        vt.free(); inst.free()


@pytest.mark.parametrize("degree", [2, 3])
@pytest.mark.parametrize("rounds", [1, 2, 3, 10])
def test_the_sumcheck_check_alone(ctx, sbn, rounds, degree):
    """sbn_zk_sumcheck_verify on a proof of sbn_zk_sumcheck_prove_* against zk_sumcheck_model.verify: verdict, r, the returned point, the state"""
    R = _R(4)
    pc, g3, g4, gens = _gens(ctx, R)
    gn_h, gn = (g3, gens["g3"]) if degree == 2 else (g4, gens["g4"])
    rng = random.Random(1000 * degree + rounds)
    n = degree + 1
    tabs = [[rng.randrange(R_MOD) for _ in range(1 << rounds)] for _ in range(2 if degree == 2 else 4)]
    claim = zm.dot(*tabs) if degree == 2 else sum(t * (a * b - c) for t, a, b, c in zip(*tabs)) % R_MOD
    blind = rng.randrange(R_MOD)
    rnd = _sbs([rng.randrange(R_MOD) for _ in range(rounds * (n + 4))])
    _, g1_h = ctx.bases_split_at(pc, R)
    ts = [ctx.table_upload(_sbs(t)) for t in tabs]
    try:
        tp = sbn.Transcript(TR_LABEL)
        prove = ctx.zk_sumcheck_prove_quad if degree == 2 else ctx.zk_sumcheck_prove_r1cs
        proof, r, _, _ = prove(*ts, g1_h, gn_h, zm.sb(claim), zm.sb(blind), rnd, tp)
        comm_claim = zm.commit_one(claim, blind, gens["g1"])
        tl = Transcript(TR_LABEL)
        want = zm.verify(tl, zm.proof_from_bytes(proof, n), comm_claim, rounds, degree, gens["g1"], gn)
        assert want is not None and _sbs(want[1]) == r and tl.state() == tp.state()
        tv = sbn.Transcript(TR_LABEL)
        state0 = tv.state()
        assert ctx.zk_sumcheck_verify(g1_h, gn_h, comm_claim, rounds, degree, proof, tv) == (want[0], r)
        assert tv.state() == tp.state()
        # another claim, a changed response, a point that does not decompress: refused, the transcript stays
        tv = sbn.Transcript(TR_LABEL)
        wrong = zm.commit_one((claim + 1) % R_MOD, blind, gens["g1"])
        assert zm.verify(Transcript(TR_LABEL), zm.proof_from_bytes(proof, n), wrong, rounds, degree, gens["g1"], gn) is None
        assert ctx.zk_sumcheck_verify(g1_h, gn_h, wrong, rounds, degree, proof, tv) is None and tv.state() == state0
        o = (6 + n) * 32 * (rounds - 1) + 128
        bad = proof[:o] + zm.sb(zm.ib(proof[o:o + 32]) + 1) + proof[o + 32:]
        assert ctx.zk_sumcheck_verify(g1_h, gn_h, comm_claim, rounds, degree, bad, tv) is None and tv.state() == state0
        bad = proof[:o] + R_MOD.to_bytes(32, "little") + proof[o + 32:]
        assert ctx.zk_sumcheck_verify(g1_h, gn_h, comm_claim, rounds, degree, bad, tv) is None and tv.state() == state0
        bad = proof[:32] + vm.undecodable_point() + proof[64:]
        assert ctx.zk_sumcheck_verify(g1_h, gn_h, comm_claim, rounds, degree, bad, tv) is None and tv.state() == state0
        assert ctx.zk_sumcheck_verify(g1_h, gn_h, comm_claim, rounds, degree, proof, tv) == (want[0], r) and tv.state() == tp.state()
    finally:
        g1_h.free()
        for t in ts:
            t.free()


def test_all_zero(ctx, sbn):
    """empty matrices, a zero witness, zero randomness, no inputs: every commitment of the proof is the identity, every sum is empty or
    cancels, and the proof is accepted"""
    shape = (4, 4, 0)
    nc, nv, _ = shape
    pc, g3, g4, gens = _gens(ctx, _R(nv))
    empty = (([], [], []),) * 3
    m = _model(shape, gens, seed=2, mats_vars_inputs=(empty, [0] * nv, []), rnd=[0] * rpm.sizes(nc, nv)[0])
    (proof, rx, ry), state = _prove(ctx, sbn, shape, m, (pc, g3, g4))
    assert proof == m["proof"]
    spans = rpm.field_spans(nc, nv)
    ident = sbn.g1_compress(bytes(64))
    for f in ("comm_vars", "claims_phase2", "comm_vars_at_ry"):
        lo, hi = spans[f]
        assert proof[lo:hi] == ident * ((hi - lo) // 32)
    assert m["evals"] == bytes(96)
    got, end = _verify(ctx, sbn, shape, m, (pc, g3, g4), proof=proof)
    assert got == (rx, ry) and end == state == m["state"]
    # the identity written with other bits set beside its flag is the same point (arkworks reads the flag first): same verdict, same state
    lo = spans["claims_phase2"][0]
    other = proof[:lo] + bytes([1] + [0] * 30 + [0x40]) + proof[lo + 32:]
    p = rpm.proof_from_bytes(other, nc, nv)
    tl = Transcript(TR_LABEL)
    assert rpm.verify(tl, p, nv, nc, [], (0, 0, 0), gens) is not None and tl.state() == state
    assert _verify(ctx, sbn, shape, m, (pc, g3, g4), proof=other) == ((rx, ry), state)


def test_refuses_what_the_literal_verifier_refuses_and_then_accepts_again(ctx, sbn):
    shape = TAMPER_SHAPE
    nc, nv, _ = shape
    pc, g3, g4, gens = _gens(ctx, _R(nv))
    m = _model(shape, gens)
    h = (pc, g3, g4)
    state0 = sbn.Transcript(TR_LABEL).state()
    cases = vm.tamperings(m["proof"], nc, nv)
    assert any("does not decompress" in k for k in cases) and any(">= r" in k for k in cases) and len(cases) == len(rpm.FIELDS) + 4
    evals = [zm.ib(m["evals"][32 * k:32 * k + 32]) for k in range(3)]
    for name, bad in cases.items():
        p = rpm.proof_from_bytes(bad, nc, nv)
        assert p is None or rpm.verify(Transcript(TR_LABEL), p, nv, nc, m["inputs"], evals, gens) is None, name
        assert _verify(ctx, sbn, shape, m, h, proof=bad) == (None, state0), name
        assert _verify(ctx, sbn, shape, m, h) == ((m["rx"], m["ry"]), m["state"]), name
    for k in range(3):
        wrong = list(evals); wrong[k] = (wrong[k] + 1) % R_MOD
        assert _verify(ctx, sbn, shape, m, h, evals=_sbs(wrong)) == (None, state0)
    for k in range(len(m["inputs"])):
        wrong = list(m["inputs"]); wrong[k] = (wrong[k] + 1) % R_MOD
        assert _verify(ctx, sbn, shape, m, h, inputs=_sbs(wrong)) == (None, state0)
    A, B, (cr, cc, cv) = m["mats"]
    changed = (A, B, (cr, cc, [(cv[0] + 1) % R_MOD] + cv[1:]))
    rx, ry = ([zm.ib(b[i:i + 32]) for i in range(0, len(b), 32)] for b in (m["rx"], m["ry"]))
    assert _verify(ctx, sbn, shape, m, h, evals=_sbs(rm.evaluate(nc, nv, changed, rx, ry))) == (None, state0)
    # the honest prover's proof for the unsatisfied instance, checked with that instance's own evaluations
    tm = Transcript(TR_LABEL)
    p2, rx2, ry2 = rpm.prove(tm, nc, nv, changed, m["vars"], m["inputs"], gens, m["rnd"])
    e2 = rm.evaluate(nc, nv, changed, rx2, ry2)
    assert rpm.verify(Transcript(TR_LABEL), p2, nv, nc, m["inputs"], e2, gens) is None
    assert _verify(ctx, sbn, shape, m, h, proof=rpm.proof_bytes(p2), evals=_sbs(e2)) == (None, state0)
    assert _verify(ctx, sbn, shape, m, h) == ((m["rx"], m["ry"]), m["state"])


def test_misuse_is_einval_and_leaves_the_transcript(ctx, sbn):
    shape = TAMPER_SHAPE
    nc, nv, n_in = shape
    R = _R(nv)
    pc, g3, g4, gens = _gens(ctx, R)
    m = _model(shape, gens)
    pc_xy = ctx.bases_download(pc, 0, R + 2)
    pc_no_h = ctx.bases_upload(pc_xy[:64 * (R + 1)])
    pc_long, _ = ctx.gens_new(R + 2, LABEL + b"_pc", want_points=False)
    g3_no_h = ctx.bases_upload(ctx.bases_download(g3, 0, 3))
    g4_no_h = ctx.bases_upload(ctx.bases_download(g4, 0, 4))
    _, g1 = ctx.bases_split_at(pc, R)
    g1_no_h = ctx.bases_upload(ctx.bases_download(g1, 0, 1))
    tr = sbn.Transcript(TR_LABEL)
    state0 = tr.state()
    big = R_MOD.to_bytes(32, "little")
    in_b = _sbs(m["inputs"])
    rx = (C.c_uint8 * 96)(); ry = (C.c_uint8 * 96)(); acc = C.c_int(7)
    L = sbn.lib()

    def raw(**kw):
        a = dict(ctx=ctx.h, nc=nc, nv=nv, input=in_b, n_in=n_in, evals=m["evals"], pc=pc.h, g3=g3.h, g4=g4.h, proof=m["proof"], tr=tr.h, rx=rx, ry=ry, acc=C.byref(acc))
        a.update(kw)
        return L.sbn_r1cs_proof_verify(a["ctx"], C.c_size_t(a["nc"]), C.c_size_t(a["nv"]), a["input"], C.c_size_t(a["n_in"]), a["evals"], a["pc"], a["g3"], a["g4"],
                                       a["proof"], a["tr"], a["rx"], a["ry"], a["acc"])
    cases = {k: {k: None} for k in ("input", "evals", "pc", "g3", "g4", "proof", "tr", "rx", "ry", "acc")}      # a null pointer
    cases.update({
        "num_cons = 1": dict(nc=1), "num_vars = 1": dict(nv=1, n_in=0, input=None), "num_cons = 0": dict(nc=0), "num_cons no power of two": dict(nc=6),
        "num_vars no power of two": dict(nv=12),
        "num_inputs = num_vars": dict(input=in_b + zm.sb(1), n_in=nv),
        "gens_pc without h": dict(pc=pc_no_h.h), "gens_pc of the wrong length": dict(pc=pc_long.h),
        "gens_3 of the wrong size": dict(g3=g4.h), "gens_4 of the wrong size": dict(g4=g3.h),
        "gens_3 without h": dict(g3=g3_no_h.h), "gens_4 without h": dict(g4=g4_no_h.h),
        "input[0] >= r": dict(input=big + in_b[32:]), "input[last] >= r": dict(input=in_b[:-32] + big),
        "evals[0] >= r": dict(evals=big + m["evals"][32:]), "evals[2] >= r": dict(evals=m["evals"][:64] + big),
    })
    sc = _model((4, 4, 1), _gens(ctx, _R(4))[3])
    sc_proof = sc["proof"][rpm.field_spans(4, 4)["sc_proof_phase1"][0]:rpm.field_spans(4, 4)["sc_proof_phase1"][1]]
    r2 = (C.c_uint8 * 64)(); exy = (C.c_uint8 * 64)()
    ident = bytes(64)

    def raw_sc(**kw):
        a = dict(ctx=ctx.h, g1=g1.h, gn=g4.h, claim=ident, rounds=2, deg=3, proof=sc_proof, tr=tr.h, r=r2, xy=exy, acc=C.byref(acc))
        a.update(kw)
        return L.sbn_zk_sumcheck_verify(a["ctx"], a["g1"], a["gn"], a["claim"], C.c_size_t(a["rounds"]), C.c_size_t(a["deg"]), a["proof"], a["tr"], a["r"], a["xy"], a["acc"])
    sc_cases = {k: {k: None} for k in ("g1", "gn", "claim", "proof", "tr", "r", "xy", "acc")}
    sc_cases.update({
        "no rounds": dict(rounds=0), "degree 1": dict(deg=1), "degree 4": dict(deg=4), "gens_n of another degree": dict(gn=g3.h), "degree 2 with gens_4": dict(deg=2),
        "gens_1 without h": dict(g1=g1_no_h.h), "gens_1 of the wrong size": dict(g1=g3.h), "gens_n without h": dict(gn=g4_no_h.h),
        "comm_claim off the curve": dict(claim=zm.sb(1) + zm.sb(1)), "comm_claim x >= p": dict(claim=b"\xff" * 32 + zm.sb(2)),
    })
    try:
        assert raw(ctx=None) == -1 and raw_sc(ctx=None) == -1
        for name, kw in cases.items():
            assert raw(**kw) == -1, name                    # SBN_EINVAL
            assert tr.state() == state0, name
        for name, kw in sc_cases.items():
            assert raw_sc(**kw) == -1, name
            assert tr.state() == state0, name
        assert raw() == 0 and acc.value == 1 and tr.state() == m["state"]
        assert bytes(rx) == m["rx"] and bytes(ry)[:len(m["ry"])] == m["ry"]
        t2 = sbn.Transcript(TR_LABEL)
        assert raw_sc(tr=t2.h) == 0                         # (the proof was made behind other transcript lines: refused, not misuse)
        assert acc.value == 0 and t2.state() == state0
    finally:
        for h in (pc_no_h, pc_long, g3_no_h, g4_no_h, g1, g1_no_h):
            h.free()


@pytest.mark.parametrize("shape", [(8, 4, 3), (64, 4, 2), (2, 64, 5)])
def test_launch_counts(ctx, sbn, shape):
    """ONE table launch; nx + ny + 3 sums that the transcript waits for and ONE for all equations; three decompress launches: the proof's
    points, the witness commitment's handle, the opening's own"""
    nc, nv, _ = shape
    pc, g3, g4, gens = _gens(ctx, _R(nv))
    m = _model(shape, gens)
    nx, ny = rpm.log2(nc), rpm.log2(nv) + 1
    _verify(ctx, sbn, shape, m, (pc, g3, g4))               # (derived sets and lookup tables are built on first use)
    ctx.sync()
    try:
        ctx.prof_enable(True); ctx.prof_reset()
        assert _verify(ctx, sbn, shape, m, (pc, g3, g4)) == ((m["rx"], m["ry"]), m["state"])
        prof = ctx.prof_get()
    finally:
        ctx.prof_enable(False); ctx.prof_reset()
    assert prof["k_pow2_table"][1] == 1
    assert prof["k_select_sum"][1] == nx + ny + 3 + 1
    assert prof["k_g1_decompress"][1] == 3


def test_results_do_not_depend_on_what_the_context_and_handles_ran_before(ctx, sbn):
    """prove, verify and the standalone opening check interleaved on one context and one set of handles, against a fresh context"""
    sa, sb_ = (4, 8, 0), (8, 4, 3)
    ha = _gens(ctx, _R(8), LABEL + b"_state_a")
    hb = _gens(ctx, _R(4), LABEL + b"_state_b")
    ma, mb = _model(sa, ha[3], seed=5), _model(sb_, hb[3], seed=6)

    def opening(c, pc, m, shape):
        """sbn_polyeval_verify of the proof's own opening, on the transcript state the R1CS verifier has there: refused or accepted, the same everywhere"""
        nc, nv, _ = shape
        sp = rpm.field_spans(nc, nv)
        comm = c.bases_from_compressed(m["proof"][sp["comm_vars"][0]:sp["comm_vars"][1]])
        tr = sbn.Transcript(b"standalone opening")
        try:
            xy, ok = c.g1_decompress(m["proof"][sp["comm_vars_at_ry"][0]:sp["comm_vars_at_ry"][1]])
            assert ok == b"\x01"
            return c.polyeval_verify(pc, comm, m["ry"][32:], m["proof"][sp["proof_eval_vars_at_ry"][0]:sp["proof_eval_vars_at_ry"][1]], tr, C_Zr_xy=xy), tr.state()
        finally:
            comm.free()
    first = _verify(ctx, sbn, sa, ma, ha[:3])
    assert first == ((ma["rx"], ma["ry"]), ma["state"])
    pa = _prove(ctx, sbn, sa, ma, ha[:3])
    second = _verify(ctx, sbn, sb_, mb, hb[:3])
    assert second == ((mb["rx"], mb["ry"]), mb["state"])
    oa = opening(ctx, ha[0], ma, sa)
    bad = vm.tamperings(mb["proof"], sb_[0], sb_[1])["flipped byte in sc_proof_phase2"]
    assert _verify(ctx, sbn, sb_, mb, hb[:3], proof=bad)[0] is None
    pb = _prove(ctx, sbn, sb_, mb, hb[:3])
    assert _verify(ctx, sbn, sa, ma, ha[:3]) == first and _verify(ctx, sbn, sb_, mb, hb[:3]) == second
    assert _verify(ctx, sbn, sa, ma, ha[:3], proof=pa[0][0]) == first
    fresh = sbn.Context(0)
    try:
        pc, _ = fresh.gens_new(_R(8) + 1, LABEL + b"_state_a_pc", want_points=False)
        g3, _ = fresh.gens_new(3, LABEL + b"_state_a_sc", want_points=False)
        g4, _ = fresh.gens_new(4, LABEL + b"_state_a_sc", want_points=False)
        try:
            assert _verify(fresh, sbn, sa, ma, (pc, g3, g4)) == first
            assert opening(fresh, pc, ma, sa) == oa
            assert _prove(fresh, sbn, sa, ma, (pc, g3, g4)) == pa
        finally:
            pc.free(); g3.free(); g4.free()
    finally:
        fresh.close()
    assert pb[1] == mb["state"]
