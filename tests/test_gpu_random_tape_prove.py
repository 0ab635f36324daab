"""GPU: a proof whose rnd comes from the library's RandomTape and draw plan (sbn_snark_draw_rnd, sbn_nizk_draw_rnd) is, byte for byte, the proof of the
literal models (tests/snark_model.py, tests/nizk_model.py) with rnd from the Python tape of tests/random_tape_model.py started from the same init —
Hyrax on three raw shapes, the KZG build once, NIZK mode on the three — and verifies."""
import pytest

import nizk_model as nm
import polyeval_model as pm
import random_tape_model as rtm
import snark_model as sm
import sparse_eval_kzg_model as skm
import sparse_eval_model as sem
from conftest import golden
from snark_model import R_MOD, Transcript

pytestmark = pytest.mark.gpu
TR = b"keyless_snark"
INIT = 0x0badc0ffee0ddf00d1234567 * 0x100000001 % R_MOD
SHAPES = [(4, 4, 1, None), (5, 3, 2, None), (2, 1, 3, None)]          # raw shapes of test_gpu_snark / test_gpu_nizk: padded already; both padded; num_inputs + 1 decides
KAT = golden("pairing_kat.json")
TAU = int(KAT["tau"], 16)


def _sbs(xs):
    return b"".join(pm.sb(x) for x in xs)


def _mats_bytes(mats):
    return [(r, c, _sbs(v)) for r, c, v in mats]


def _device_rnd(sbn, name, draw):
    t = sbn.RandomTape(name, pm.sb(INIT))
    try:
        return draw(t)
    finally:
        t.free()


@pytest.mark.parametrize("key", SHAPES)
def test_snark_proof_from_the_librarys_tape_is_the_models(ctx, sbn, key):
    nc, nv, ni, empty = key
    mats, vars_, inputs = sm.satisfying_instance(nc, nv, ni, seed=11, empty=empty)
    inst = sm.Instance(nc, nv, ni, mats)
    dg = ctx.snark_gens_new(nc, nv, ni, max(len(m[0]) for m in mats))
    dkey = ctx.snark_encode(nc, nv, ni, _mats_bytes(mats), dg)
    vt = ctx.table_upload(_sbs(sm.pad_vars(vars_, sm.npo2(max(len(vars_), 1)))))
    try:
        gens = sm.make_gens([ctx.bases_download(getattr(dg, k), 0, len(getattr(dg, k)) + 1) for k in dg.KINDS], inst)
        comm = sm.encode(inst, gens)
        want_rnd = rtm.draw_snark(rtm.RandomTape(rtm.SNARK_NAME, INIT), comm)
        rnd = _device_rnd(sbn, rtm.SNARK_NAME, lambda t: t.draw_snark(dkey))
        assert len(rnd) == 32 * dkey.sizes()[0] and rnd == rtm.to_bytes(want_rnd)
        tp = Transcript(TR)
        want = sm.proof_bytes(sm.prove(tp, inst, comm, vars_, inputs, gens, want_rnd))
        tr = sbn.Transcript(TR)
        got = ctx.snark_prove(dkey, vt, _sbs(inputs), dg, rnd, tr)
        assert got == want and tr.state() == tp.state()
        tv = sbn.Transcript(TR)
        assert ctx.snark_verify(dkey, _sbs(inputs), dg, got, tv) is True and tv.state() == tp.state()
        # another init, another proof, which verifies as well
        t2 = sbn.RandomTape(rtm.SNARK_NAME, pm.sb(INIT + 1))
        try:
            other = ctx.snark_prove(dkey, vt, _sbs(inputs), dg, t2.draw_snark(dkey), sbn.Transcript(TR))
        finally:
            t2.free()
        assert other != got and ctx.snark_verify(dkey, _sbs(inputs), dg, other, sbn.Transcript(TR)) is True
    finally:
        vt.free(); dkey.free(); dg.free()


def test_kzg_proof_from_the_librarys_tape_is_the_models(ctx, sbn):
    nc, nv, ni, empty = (5, 3, 2, None)
    mats, vars_, inputs = sm.satisfying_instance(nc, nv, ni, seed=11, empty=empty)
    inst = sm.Instance(nc, nv, ni, mats)
    dg = ctx.snark_gens_new(nc, nv, ni, max(len(m[0]) for m in mats))
    dkey = ctx.snark_encode(nc, nv, ni, _mats_bytes(mats), dg)
    vt = ctx.table_upload(_sbs(sm.pad_vars(vars_, sm.npo2(max(len(vars_), 1)))))
    srs = g2 = tg2 = None
    try:
        gens = sm.make_gens([ctx.bases_download(getattr(dg, k), 0, len(getattr(dg, k)) + 1) for k in dg.KINDS], inst)
        comm = sm.encode(inst, gens)
        srs_n = (1 << sem.Shape(inst.nx, inst.ny, comm["N"], 3).ell["derefs"]) + 1
        want_rnd = rtm.draw_snark(rtm.RandomTape(rtm.SNARK_NAME, INIT), comm, kzg=True)
        rnd = _device_rnd(sbn, rtm.SNARK_NAME, lambda t: t.draw_snark(dkey, kzg=True))
        assert len(rnd) == 32 * dkey.sizes(True)[0] and rnd == rtm.to_bytes(want_rnd)
        tp = Transcript(TR)
        want = sm.proof_bytes(sm.prove(tp, inst, comm, vars_, inputs, gens, want_rnd, skm.Srs(TAU, srs_n)), True)
        srs = ctx.kzg_srs_from_tau(pm.sb(TAU), srs_n)
        tr = sbn.Transcript(TR)
        got = ctx.snark_prove(dkey, vt, _sbs(inputs), dg, rnd, tr, srs=srs)
        assert got == want and tr.state() == tp.state()
        g2, tg2 = (ctx.g2_prepare(bytes.fromhex(KAT["g2"][k])) for k in ("gen", "tau"))
        assert ctx.snark_verify(dkey, _sbs(inputs), dg, got, sbn.Transcript(TR), g2=g2, tau_g2=tg2) is True
    finally:
        for h in (g2, tg2, srs, vt, dkey, dg):
            if h is not None:
                h.free()


@pytest.mark.parametrize("key", SHAPES)
def test_nizk_proof_from_the_librarys_tape_is_the_models(ctx, sbn, key):
    nc, nv, ni, _ = key
    digest = bytes(range(7, 39))
    mats, vars_, inputs = nm.instance(key, 11)
    inst = nm.Instance(nc, nv, ni, mats)
    dg = ctx.nizk_gens_new(nc, nv, ni)
    dinst = ctx.nizk_instance_new(nc, nv, ni, _mats_bytes(mats), digest)
    vt = ctx.table_upload(_sbs(nm.pad_vars(vars_, nm.sm.npo2(max(len(vars_), 1)))))
    try:
        gens = nm.make_gens([ctx.bases_download(b, 0, len(b) + 1) for b in (dg.pc, dg.g3, dg.g4)], inst)
        want_rnd = rtm.draw_nizk(rtm.RandomTape(rtm.NIZK_NAME, INIT), inst)
        rnd = _device_rnd(sbn, rtm.NIZK_NAME, lambda t: t.draw_nizk(dinst))
        assert len(rnd) == 32 * dinst.sizes()[0] and rnd == rtm.to_bytes(want_rnd)
        tp = Transcript(TR)
        want = nm.proof_bytes(nm.prove(tp, inst, digest, vars_, inputs, gens, want_rnd))
        tr = sbn.Transcript(TR)
        got = ctx.nizk_prove(dinst, vt, _sbs(inputs), dg, rnd, tr)
        assert got == want and tr.state() == tp.state()
        assert ctx.nizk_verify(dinst, _sbs(inputs), dg, got, sbn.Transcript(TR)) is True
    finally:
        vt.free(); dinst.free(); dg.free()
