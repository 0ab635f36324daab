"""GPU: sbn_sumcheck_prove — the whole batched cubic sumcheck, transcript included, in one call — against a replay in Python.

The replay: the model transcript (tests/transcript_model.py), the CPU oracle's prove_cubic_batched loop for the sums and the final
claims, the reference's round logic (sumcheck.rs:269-301) in Python integers.  The oracle's loop takes its challenges up front, so
it is run on the challenges the device returned; the model then re-derives every round from the oracle's sums: round 0's sums
depend on no challenge, and round j + 1's are checked only after r_j was found equal, so the comparison is the sequential one."""
import numpy as np
import pytest

import transcript_model as tm
from conftest import rand_scalars

pytestmark = pytest.mark.gpu
R = tm.R_MOD


def _int(b):
    return int.from_bytes(b, "little")


def _tables(ctx, count, n, seed, zero=False):
    import torch
    dev, host = [], []
    for k in range(count):
        x = torch.zeros((n, 8), dtype=torch.int32, device="cuda")
        if not zero:
            ctx.scalars_synthetic(0x7A4E5C21F + seed + k, 0, n, x.data_ptr())
        torch.cuda.synchronize()
        host.append(x.cpu().numpy().view("uint8").reshape(-1))
        dev.append(ctx.table_from_dev(x.data_ptr(), n))
        del x
    return dev, host


def _split(lst, n_par, n_seq, with_c=True):
    o = 2 * n_par + (1 if (n_par and with_c) else 0)
    return lst[:n_par], lst[n_par:2 * n_par], (lst[2 * n_par] if (n_par and with_c) else None), lst[o:o + n_seq], lst[o + n_seq:o + 2 * n_seq], lst[o + 2 * n_seq:]


def _check_against_replay(ol, host_parts, co, claim, model, polys, rs, finals):
    Ap, Bp, Cp, As, Bs, Cs = host_parts
    rounds = len(rs)
    _, want_comb, want_fin = ol.sc_prove_cubic_batched(Ap, Bp, Cp, As, Bs, Cs, co, b"".join(rs), 16)
    e = claim
    for j in range(rounds):
        e0, e2, e3 = (_int(want_comb[j][32 * k:32 * k + 32]) for k in range(3))
        cj, rj, e = tm.sumcheck_round_step(model, e, e0, e2, e3)
        assert [_int(x) for x in polys[j]] == cj, f"round {j}: polynomial"
        assert _int(rs[j]) == rj, f"round {j}: challenge"
    assert finals == want_fin
    return e


def _begin(ctx, dev_parts, co, rand):
    Ap, Bp, Cp, As, Bs, Cs = dev_parts
    if rand is not None:
        return ctx.sumcheck_begin_eq(Ap, Bp, rand, As, Bs, Cs, co)
    return ctx.sumcheck_begin(Ap, Bp, Cp, As, Bs, Cs, co)


def _start(sbn, label, pos):
    """library transcript + model at STROBE position pos"""
    a, m = sbn.Transcript(label), tm.Transcript(label)
    k = (pos - m.s.pos - 9) % tm.RATE
    a.append_message(b"f", bytes(k)); m.append_message(b"f", bytes(k))
    assert m.s.pos == pos and a.state() == m.state()
    return a, m


def _run(ctx, sbn, ol, n_par, n_seq, logn, seed, eq=False, zero=False, claim=None, pos=29, via_rounds=False):
    n = 1 << logn
    with_c = not eq
    dev, host = _tables(ctx, 2 * n_par + (1 if (n_par and with_c) else 0) + 3 * n_seq, n, seed, zero)
    dparts, hparts = _split(dev, n_par, n_seq, with_c), _split(host, n_par, n_seq, with_c)
    rand = rand_scalars(logn, seed + 5) if eq else None
    if eq:
        hparts = hparts[:2] + (np.frombuffer(ol.eq_evals(rand), dtype=np.uint8),) + hparts[3:]
    co = rand_scalars(n_par + n_seq, seed + 2)
    claim = _int(rand_scalars(1, seed + 3)) if claim is None else claim
    tr, model = _start(sbn, b"sumcheck prove test", pos)
    st, ev0 = _begin(ctx, dparts, co, rand)
    ref = None
    if via_rounds:
        # the same state driven by sbn_sumcheck_round with the host transcript: drawn here before the one-call run
        st2, ev = _begin(ctx, dparts, co, rand)
        assert ev == ev0
        t2 = tr.clone()
        e, p2, r2 = claim, [], []
        for j in range(logn):
            evs = [ev[0:32], ((e - _int(ev[0:32])) % R).to_bytes(32, "little"), ev[32:64], ev[64:96]]
            cj = sbn.unipoly_from_evals(b"".join(evs))
            cj = [cj[32 * k:32 * k + 32] for k in range(4)]
            t2.append_message(b"poly", b"UniPoly_begin")
            for x in cj:
                t2.append_scalar(b"coeff", x)
            t2.append_message(b"poly", b"UniPoly_end")
            rj = t2.challenge_scalar(b"challenge_nextround")
            e = _int(sbn.unipoly_eval(b"".join(cj), rj))
            p2.append(cj); r2.append(rj)
            ev = st2.round(rj)
        ref = (p2, r2, st2.finish(), t2.state())
        st2.free()
    polys, rs, finals = ctx.sumcheck_prove(st, tr, claim.to_bytes(32, "little"))
    assert len(st) == 1 and len(rs) == logn
    st.free()
    _check_against_replay(ol, hparts, co, claim, model, polys, rs, finals)
    after = tr.state()
    assert after == model.state()
    assert _int(tr.challenge_scalar(b"next")) == model.challenge_scalar(b"next")          # the host goes on where the device stopped
    if ref is not None:
        assert (polys, rs, finals, after) == ref
    for t in dev:
        t.free()
    return tr, model


@pytest.mark.parametrize("pos", [0, 1, 77, 78, 82, 164, 165])
def test_device_transcript_start_phases(ctx, sbn, ol, pos):
    """2-entry tables: one round, so the call is the device transcript step alone, started at every kind of phase (a round that is two
    blocks, three blocks, one that ends exactly on a block, headers that straddle a block)"""
    _run(ctx, sbn, ol, 1, 0, 1, 100 + pos, pos=pos)
    _run(ctx, sbn, ol, 2, 1, 2, 300 + pos, pos=pos)


SHAPES = [(1, 0, 1), (1, 0, 2), (0, 1, 3), (3, 2, 8), (12, 6, 10), (12, 6, 15), (12, 6, 17), (16, 0, 17), (12, 6, 21)]


@pytest.mark.parametrize("n_par,n_seq,logn", SHAPES)
def test_prove_vs_replay(ctx, sbn, ol, n_par, n_seq, logn):
    _run(ctx, sbn, ol, n_par, n_seq, logn, 1000 + 37 * logn + n_par)


@pytest.mark.parametrize("n_par,n_seq,logn", [s for s in SHAPES if s[0] > 0])
def test_prove_begin_eq_vs_replay(ctx, sbn, ol, n_par, n_seq, logn):
    _run(ctx, sbn, ol, n_par, n_seq, logn, 2000 + 37 * logn + n_par, eq=True)


def test_prove_all_zero_tables(ctx, sbn, ol):
    _run(ctx, sbn, ol, 3, 2, 8, 3000, zero=True)
    _run(ctx, sbn, ol, 12, 6, 17, 3001, zero=True, claim=0)


def test_prove_claim_below_e0_wraps(ctx, sbn, ol):
    """claim = 0 with uniform tables: e1 = claim - e0 is negative before the reduction in every round's first step"""
    _run(ctx, sbn, ol, 3, 2, 8, 3100, claim=0)
    _run(ctx, sbn, ol, 12, 6, 10, 3101, claim=R - 1)


@pytest.mark.parametrize("n_par,n_seq,logn", [(1, 0, 1), (3, 2, 8), (12, 6, 10), (12, 6, 17), (0, 2, 12)])
def test_prove_equals_round_loop_with_host_transcript(ctx, sbn, ol, n_par, n_seq, logn):
    _run(ctx, sbn, ol, n_par, n_seq, logn, 4000 + logn, via_rounds=True)
    if n_par:
        _run(ctx, sbn, ol, n_par, n_seq, logn, 4100 + logn, via_rounds=True, eq=True)


def test_two_sumchecks_on_one_transcript(ctx, sbn, ol):
    n_par, n_seq = 4, 2
    tr, model = _start(sbn, b"two in a row", 40)
    for k, logn in enumerate((9, 16)):
        dev, host = _tables(ctx, 2 * n_par + 1 + 3 * n_seq, 1 << logn, 5000 + 50 * k)
        co = rand_scalars(n_par + n_seq, 5001 + k); claim = _int(rand_scalars(1, 5002 + k))
        st, _ = _begin(ctx, _split(dev, n_par, n_seq), co, None)
        polys, rs, finals = ctx.sumcheck_prove(st, tr, claim.to_bytes(32, "little"))
        st.free()
        _check_against_replay(ol, _split(host, n_par, n_seq), co, claim, model, polys, rs, finals)
        assert tr.state() == model.state()
        tr.append_message(b"between", b"sumchecks"); model.append_message(b"between", b"sumchecks")
        for t in dev:
            t.free()


def test_two_contexts_two_transcripts(ctx, sbn, ol):
    import threading
    other = sbn.Context(0)
    errs = []

    def work(cx, seed):
        try:
            for rep in range(2):
                _run(cx, sbn, ol, 5, 2, 13, seed + 10 * rep, pos=3 + seed % 100)
        except BaseException as e:      # noqa: BLE001 - reported by the main thread
            errs.append(e)
    try:
        ths = [threading.Thread(target=work, args=(cx, s)) for cx, s in ((ctx, 6000), (other, 6100))]
        for t in ths:
            t.start()
        for t in ths:
            t.join()
    finally:
        other.close()
    assert not errs, errs


def test_prove_errors(ctx, sbn):
    a, b, c2 = (ctx.table_upload(rand_scalars(8, s)) for s in (1, 2, 3))
    co = rand_scalars(1, 4)
    tr = sbn.Transcript(b"errors")
    before = tr.state()
    st, _ = ctx.sumcheck_begin([a], [b], c2, [], [], [], co)
    with pytest.raises(sbn.SbnError):
        ctx.sumcheck_prove(st, tr, R.to_bytes(32, "little"))             # claim not canonical
    assert tr.state() == before and len(st) == 8
    st.round(rand_scalars(1, 5))
    with pytest.raises(sbn.SbnError):
        ctx.sumcheck_prove(st, tr, bytes(32))                             # not a fresh state
    assert tr.state() == before
    st.free()
    for t in (a, b, c2):
        t.free()
