"""GPU: sbn_sparse_eval_verify — SparseMatPolyEvalProof::verify (sparse_mlpoly_full.rs:1815-1845) in one call — against the literal verdict on bytes
(tests/sparse_eval_verify_model.py: verify_bytes): what it accepts, with the transcript state of the model's verifier and of the prover; what it
refuses, with the transcript untouched and an honest call accepted behind it; what is misuse; its launches; and its independence of what the
context ran before."""
import ctypes as C

import numpy as np
import pytest

import dense_model as dm
import oracle_lib as ol
import polyeval_model as pm
import r1cs_model as rm
import r1cs_proof_model as rpm
import sparse_eval_loop as loop
import sparse_eval_model as sem
import sparse_eval_verify_model as sevm
import zk_sumcheck_model as zm
from sparse_eval_model import R, Transcript

pytestmark = pytest.mark.gpu
LABEL = b"gens_sparse_verify_gpu"
TR_LABEL = b"sparse verify gpu"
KINDS = ("ops", "mem", "derefs")
TAMPER_SHAPES = [(2, 3, (3, 4, 1)), (2, 2, (4, 4, 4, 4))]
Q_MOD = 0x30644e72e131a029b85045b68181585d97816a916871ca8d3c208c16d87cfd47
_GENS, _CASES = {}, {}


def _sbs(xs):
    return b"".join(pm.sb(x) for x in xs)


def _gens(ctx, shape, label=LABEL, points=True):
    """({kind: handle}, the model's gens or None) per size triple and label for the whole module"""
    key = (tuple(shape.lg[k] for k in KINDS), label)
    if key not in _GENS:
        made = {k: ctx.gens_new(shape.R(k) + 1, label + b"_" + k.encode(), want_points=points) for k in KINDS}
        _GENS[key] = ({k: made[k][0] for k in KINDS}, sem.make_gens({k: made[k][1] for k in KINDS}, shape) if points else None)
    return _GENS[key]


@pytest.fixture(scope="module", autouse=True)
def _free_handles():
    yield
    for handles, _ in _GENS.values():
        for h in handles.values():
            h.free()
    for c in _CASES.values():
        for h in c["comm_h"]:
            h.free()
    _GENS.clear(); _CASES.clear()


def case(ctx, shape_key, seed=0):
    """one honest model proof per (shape, seed) for the whole module: the instance, the model's and the device's generators, the computation
    commitment as points and as resident handles, the proof bytes and the prover's end state"""
    key = (shape_key, seed)
    if key not in _CASES:
        nx, ny, _ = shape_key
        mats, rx, ry, evals, rnd = sem.instance(shape_key, seed)
        dense = dm.Dense(nx, ny, mats)
        shape = sem.Shape(nx, ny, dense.N, dense.batch)
        handles, gens = _gens(ctx, shape)
        tp = Transcript(TR_LABEL)
        data = sem.proof_bytes(sem.prove(tp, nx, ny, mats, rx, ry, evals, gens, rnd))
        comm = sem.commit_dense(dense, gens, shape)
        _CASES[key] = dict(nx=nx, ny=ny, mats=mats, rx=rx, ry=ry, evals=evals, rnd=rnd, shape=shape, handles=handles, gens=gens, data=data, state=tp.state(),
                           comm=comm, comm_h=[ctx.bases_upload(b"".join(comm[0])), ctx.bases_upload(b"".join(comm[1]))])
    return _CASES[key]


def device_verify(ctx, sbn, c, data=None, rx=None, evals=None, comm_h=None, handles=None):
    """-> (accepted, the transcript's state behind the call, its state before)"""
    s, h, ch = c["shape"], handles or c["handles"], comm_h or c["comm_h"]
    tr = sbn.Transcript(TR_LABEL)
    before = tr.state()
    ok = ctx.sparse_eval_verify(c["nx"], c["ny"], s.N, s.cells, s.b, ch[0], ch[1], _sbs(c["rx"] if rx is None else rx), _sbs(c["ry"]), _sbs(c["evals"] if evals is None else evals),
                                h["ops"], h["mem"], h["derefs"], c["data"] if data is None else data, tr)
    return ok, tr.state(), before


def model_verify(c, data=None, rx=None, evals=None, comm=None, gens=None):
    tv = Transcript(TR_LABEL)
    ok = sevm.verify_bytes(tv, c["data"] if data is None else data, c["shape"], comm or c["comm"], c["rx"] if rx is None else rx, c["ry"], c["evals"] if evals is None else evals, gens or c["gens"])
    return ok, tv.state()


@pytest.mark.parametrize("shape_key", sem.SHAPES)
def test_accepts_the_provers_and_the_models_bytes(ctx, sbn, shape_key):
    c = case(ctx, shape_key)
    s = c["shape"]
    want = model_verify(c)
    assert want == (True, c["state"])
    assert device_verify(ctx, sbn, c)[:2] == want
    # the device prover's bytes
    dense = ctx.dense_build(c["nx"], c["ny"], [(r, cc, _sbs(v)) for r, cc, v in c["mats"]])
    tp = sbn.Transcript(TR_LABEL)
    try:
        proof = ctx.sparse_eval_prove(dense, _sbs(c["rx"]), _sbs(c["ry"]), _sbs(c["evals"]), c["handles"]["ops"], c["handles"]["mem"], c["handles"]["derefs"], _sbs(c["rnd"]), tp)
    finally:
        dense.free()
    assert device_verify(ctx, sbn, c, data=proof)[:2] == (True, tp.state()) and tp.state() == c["state"]
    # the commitments from compressed bytes
    comp = [ctx.bases_from_compressed(b"".join(ol.g1_compress(p) for p in c["comm"][k])) for k in (0, 1)]
    try:
        assert device_verify(ctx, sbn, c, comm_h=comp)[:2] == want
    finally:
        for h in comp:
            h.free()
    if shape_key == (2, 3, (3, 4, 1)):                              # an identity row in comm_derefs
        lo, hi = sem.field_spans(s)["comm_derefs"]
        assert c["data"][hi - 32:hi] == sbn.g1_compress(bytes(64))


@pytest.mark.parametrize("lg_n", [10, 13])
def test_accepts_a_proof_of_the_device_prover_at_larger_sizes(ctx, sbn, lg_n):
    nx = ny = lg_n
    N, b = 1 << lg_n, 3
    shape = sem.Shape(nx, ny, N, b)
    handles, gens = _gens(ctx, shape, LABEL + b"_big", points=lg_n == 10)
    rng = np.random.default_rng(lg_n)
    dense = ctx.dense_build(nx, ny, loop.random_mats(nx, ny, N, b, 70 + lg_n))
    rx, ry = rm.random_vals(rng, nx).tobytes(), rm.random_vals(rng, ny).tobytes()
    rnd = rm.random_vals(rng, sem.sizes(nx, ny, N, b)[0]).tobytes()
    comm_h, splits = [], []
    try:
        evals = loop.evals_of(sbn, ctx, dense, rx, ry)
        tp = sbn.Transcript(TR_LABEL)
        proof = ctx.sparse_eval_prove(dense, rx, ry, evals, handles["ops"], handles["mem"], handles["derefs"], rnd, tp)
        comm_xy = []
        for kind, tab in (("ops", dense.comb_ops), ("mem", dense.comb_mem)):
            Gn, G1 = ctx.bases_split_at(handles[kind], shape.R(kind))
            splits += [Gn, G1]
            xy, _ = ctx.commit_table(Gn, tab, None, 1 << pm.factored_lens(shape.ell[kind])[0], shape.R(kind))
            comm_xy.append(xy); comm_h.append(ctx.bases_upload(xy))
        tv = sbn.Transcript(TR_LABEL)
        assert ctx.sparse_eval_verify(nx, ny, N, 1 << nx, b, comm_h[0], comm_h[1], rx, ry, evals, handles["ops"], handles["mem"], handles["derefs"], proof, tv)
        assert tv.state() == tp.state()
        bad = bytearray(proof); bad[-32] ^= 1                       # z2 of the derefs opening
        tb = sbn.Transcript(TR_LABEL)
        assert not ctx.sparse_eval_verify(nx, ny, N, 1 << nx, b, comm_h[0], comm_h[1], rx, ry, evals, handles["ops"], handles["mem"], handles["derefs"], bytes(bad), tb)
        assert tb.state() == sbn.Transcript(TR_LABEL).state()
        if gens is not None:                                        # 2^10: the literal verdict as well
            ints = lambda x: [int.from_bytes(x[i:i + 32], "little") for i in range(0, len(x), 32)]      # noqa: E731
            comm = tuple([xy[64 * i:64 * i + 64] for i in range(len(xy) // 64)] for xy in comm_xy)
            tm = Transcript(TR_LABEL)
            assert sevm.verify_bytes(tm, proof, shape, comm, ints(rx), ints(ry), ints(evals), gens) and tm.state() == tp.state()
    finally:
        for h in comm_h + splits:
            h.free()
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


def tamperings(c):
    """{name: data} — every change of the proof's bytes the check must refuse"""
    data, sp = c["data"], sem.field_spans(c["shape"])
    out = {}
    for f in sem.FIELDS:                                            # the lowest byte of the field's last element; comm_derefs: of its first (its last may be the identity)
        lo, hi = sp[f]
        b = bytearray(data); b[lo if f == "comm_derefs" else hi - 32] ^= 1
        out["flipped byte in " + f] = bytes(b)
    for f in ("prod.proof_ops", "prod.proof_mem", "hash.eval_row", "hash.proof_ops", "hash.proof_mem", "hash.proof_derefs"):
        lo, hi = sp[f]
        b = bytearray(data); b[hi - 32:hi] = R.to_bytes(32, "little")
        out["scalar = r in " + f] = bytes(b)
    lo, hi = sp["comm_derefs"]
    spots = {"first row of comm_derefs": lo, "last row of comm_derefs": hi - 32}
    for f in ("hash.proof_ops", "hash.proof_mem", "hash.proof_derefs"):
        spots["L[0] of " + f] = sp[f][0]
        spots["beta of " + f] = sp[f][1] - 96
    start = data[lo:lo + 32]
    for name, at in spots.items():
        b = bytearray(data); b[at:at + 32] = _bad_point(data[at:at + 32] if not data[at + 31] & 0x40 else start)
        out["no point at " + name] = bytes(b)
    return out


@pytest.mark.parametrize("shape_key", TAMPER_SHAPES)
def test_refuses_what_the_literal_verdict_refuses_and_then_accepts_again(ctx, sbn, shape_key):
    c = case(ctx, shape_key)
    honest = (True, c["state"])
    for name, data in tamperings(c).items():
        assert model_verify(c, data=data)[0] is False, name
        ok, state, before = device_verify(ctx, sbn, c, data=data)
        assert ok is False and state == before, name
        assert device_verify(ctx, sbn, c)[:2] == honest, name
    assert len(tamperings(c)) == 13 + 6 + 8


@pytest.mark.parametrize("shape_key", TAMPER_SHAPES)
def test_refuses_wrong_inputs_of_the_verifier(ctx, sbn, shape_key):
    c = case(ctx, shape_key)
    other = case(ctx, shape_key, seed=1)                            # another instance of the same shape
    honest = (True, c["state"])
    trials = []
    for i in range(c["shape"].b):
        wrong = list(c["evals"]); wrong[i] = (wrong[i] + 1) % R
        trials.append(("evals[%d]" % i, dict(evals=wrong), dict(evals=wrong)))
    wrx = list(c["rx"]); wrx[0] = (wrx[0] + 1) % R
    trials.append(("rx[0]", dict(rx=wrx), dict(rx=wrx)))
    trials.append(("comm_ops of another instance", dict(comm_h=[other["comm_h"][0], c["comm_h"][1]]), dict(comm=(other["comm"][0], c["comm"][1]))))
    trials.append(("comm_mem of another instance", dict(comm_h=[c["comm_h"][0], other["comm_h"][1]]), dict(comm=(c["comm"][0], other["comm"][1]))))
    if c["shape"].lg["ops"] == c["shape"].lg["derefs"]:
        h, g = c["handles"], c["gens"]
        trials.append(("gens_ops and gens_derefs swapped", dict(handles=dict(ops=h["derefs"], mem=h["mem"], derefs=h["ops"])), dict(gens=dict(ops=g["derefs"], mem=g["mem"], derefs=g["ops"]))))
    for name, dev, mod in trials:
        assert model_verify(c, **mod)[0] is False, name
        ok, state, before = device_verify(ctx, sbn, c, **dev)
        assert ok is False and state == before, name
        assert device_verify(ctx, sbn, c)[:2] == honest, name


def test_misuse_is_einval_and_launches_nothing(ctx, sbn):
    c = case(ctx, (2, 3, (3, 4, 1)))
    s, h, ch = c["shape"], c["handles"], c["comm_h"]
    L = sbn.lib()
    tr = sbn.Transcript(TR_LABEL)
    before = tr.state()
    rx, ry, ev = _sbs(c["rx"]), _sbs(c["ry"]), _sbs(c["evals"])
    no_h = ctx.bases_upload(ol.gens_new(s.R("ops") + 1, b"no h")[0][:64 * (s.R("ops") + 1)])
    big = R.to_bytes(32, "little")

    def call(nx=c["nx"], ny=c["ny"], N=s.N, cells=s.cells, b=s.b, co=ch[0].h, cm=ch[1].h, rx=rx, ry=ry, ev=ev, go=h["ops"].h, gm=h["mem"].h, gd=h["derefs"].h, proof=c["data"], t=tr.h, acc=True):
        a = C.c_int(7)
        p = lambda x: None if x is None else (C.c_uint8 * len(x)).from_buffer_copy(x)      # noqa: E731
        rc = L.sbn_sparse_eval_verify(ctx.h, C.c_size_t(nx), C.c_size_t(ny), C.c_size_t(N), C.c_size_t(cells), C.c_size_t(b), co, cm, p(rx), p(ry), p(ev), go, gm, gd, p(proof), t,
                                      C.byref(a) if acc else None)
        return rc
    ctx.prof_enable(True)
    try:
        ctx.prof_reset()
        bad = [dict(co=None), dict(cm=None), dict(rx=None), dict(ry=None), dict(ev=None), dict(go=None), dict(gm=None), dict(gd=None), dict(proof=None), dict(t=None), dict(acc=False),
               dict(b=0), dict(b=5), dict(N=1), dict(N=3), dict(N=0), dict(cells=2 * s.cells), dict(cells=s.cells // 2),
               dict(co=ch[1].h), dict(cm=ch[0].h), dict(go=h["mem"].h), dict(gm=h["ops"].h), dict(gd=h["mem"].h), dict(go=no_h.h),
               dict(rx=big + rx[32:]), dict(ry=ry[:-32] + big), dict(ev=big + ev[32:])]
        assert len(ch[0]) != len(ch[1]) and len(h["mem"]) != len(h["ops"])
        for kw in bad:
            assert call(**kw) == -1, kw
        assert ctx.prof_get() == {}, "a refused call launched something"
        assert tr.state() == before
    finally:
        ctx.prof_enable(False)
        no_h.free()
    assert device_verify(ctx, sbn, c)[:2] == (True, c["state"])


@pytest.mark.parametrize("shape_key", [(1, 1, (2, 2, 2)), (2, 3, (3, 4, 1)), (2, 2, (4, 4, 4, 4))])
def test_launch_counts(ctx, sbn, shape_key):
    c = case(ctx, shape_key)
    device_verify(ctx, sbn, c)                                      # (the derived sets are built by now)
    ctx.prof_enable(True)
    try:
        ctx.prof_reset()
        assert device_verify(ctx, sbn, c)[0]
        prof = {k: v[1] for k, v in ctx.prof_get().items()}
    finally:
        ctx.prof_enable(False)
    assert prof["k_g1_decompress"] == 1 and prof["k_window_sums"] == 4 and prof["k_sums_to_host"] == 4
    assert prof["k_polyeval_eq"] == 3 and prof["k_polyeval_verify_row"] == 3 and "k_points_to_host" not in prof and "k_pow2_table" not in prof


def test_results_do_not_depend_on_what_the_context_ran_before(ctx, sbn):
    """prove, verify, the standalone opening check and the R1CS proof's check interleaved on one context, against a fresh context"""
    ka, kb = (2, 3, (3, 4, 1)), (3, 3, (8, 8, 8))
    a, b = case(ctx, ka), case(ctx, kb)
    r1 = (4, 4, 1)
    Rpc = 1 << pm.factored_lens(rpm.log2(r1[1]))[1]

    def r1cs(cx):
        pc, pc_xy = cx.gens_new(Rpc + 1, LABEL + b"_r1_pc"); g3, g3_xy = cx.gens_new(3, LABEL + b"_r1_sc"); g4, g4_xy = cx.gens_new(4, LABEL + b"_r1_sc")
        try:
            gens = rpm.make_gens(pc_xy, Rpc, g3_xy, g4_xy)
            mats, vars_, inputs = rpm.satisfying_instance(r1[0], r1[1], r1[2], 4242)
            proof, rx, ry = rpm.prove(Transcript(b"r1"), r1[0], r1[1], mats, vars_, inputs, gens, rpm.random_rnd(r1[0], r1[1], 77))
            evals = rm.evaluate(r1[0], r1[1], mats, rx, ry)
            tr = sbn.Transcript(b"r1")
            got = cx.r1cs_proof_verify(r1[0], r1[1], b"".join(zm.sb(x) for x in inputs), b"".join(zm.sb(x) for x in evals), pc, g3, g4, rpm.proof_bytes(proof), tr)
            assert got is not None
            return got, tr.state()
        finally:
            pc.free(); g3.free(); g4.free()

    def opening(cx, c, handles, comm_h):
        """sbn_joint_opening_verify of the proof's mem opening on a transcript of its own: refused or accepted, the same everywhere"""
        lo, hi = sem.field_spans(c["shape"])["hash.proof_mem"]
        tr = sbn.Transcript(b"standalone opening")
        return cx.joint_opening_verify(handles["mem"], comm_h[1], _sbs([3, 5]), sem.MEM_LABELS, _sbs(c["rx"] + c["ry"])[:32 * c["shape"].m], c["data"][lo:hi], tr), tr.state()

    def prove(cx, c, handles):
        dense = cx.dense_build(c["nx"], c["ny"], [(r, cc, _sbs(v)) for r, cc, v in c["mats"]])
        tr = sbn.Transcript(TR_LABEL)
        try:
            return cx.sparse_eval_prove(dense, _sbs(c["rx"]), _sbs(c["ry"]), _sbs(c["evals"]), handles["ops"], handles["mem"], handles["derefs"], _sbs(c["rnd"]), tr), tr.state()
        finally:
            dense.free()
    first = device_verify(ctx, sbn, a)
    assert first[:2] == (True, a["state"])
    pa = prove(ctx, a, a["handles"])
    second = device_verify(ctx, sbn, b)
    oa = opening(ctx, a, a["handles"], a["comm_h"])
    ra = r1cs(ctx)
    assert device_verify(ctx, sbn, b, data=tamperings(b)["flipped byte in prod.proof_ops"])[0] is False
    small = ctx.g1_small_sums(b["comm"][0][0] + b["comm"][0][1], pm.sb(7) + pm.sb(R - 1), [2])
    assert device_verify(ctx, sbn, a) == first and device_verify(ctx, sbn, b) == second and second[:2] == (True, b["state"])
    assert device_verify(ctx, sbn, a, data=pa[0]) == first
    fresh = sbn.Context(0)
    try:
        fh = {k: fresh.gens_new(a["shape"].R(k) + 1, LABEL + b"_" + k.encode(), want_points=False)[0] for k in KINDS}
        fc = [fresh.bases_upload(b"".join(a["comm"][0])), fresh.bases_upload(b"".join(a["comm"][1]))]
        try:
            assert device_verify(fresh, sbn, a, comm_h=fc, handles=fh) == first
            assert opening(fresh, a, fh, fc) == oa
            assert prove(fresh, a, fh) == pa
            assert r1cs(fresh) == ra
            assert fresh.g1_small_sums(b["comm"][0][0] + b["comm"][0][1], pm.sb(7) + pm.sb(R - 1), [2]) == small
        finally:
            for h in list(fh.values()) + fc:
                h.free()
    finally:
        fresh.close()
