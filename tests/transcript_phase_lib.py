"""Shared by the GPU tests of the device transcript (test_gpu_sumcheck_prove.py, test_gpu_product_proof.py, test_gpu_transcript_phases.py):
a library transcript and the model brought to a chosen STROBE phase, sbn_sumcheck_prove against the replay (the model transcript, the CPU
oracle's prove_cubic_batched loop, the reference's round logic in Python integers) and sbn_product_proof_prove against
tests/product_proof_model.py.  Exact comparisons only.  Not a test module."""
import numpy as np

import product_proof_model as pm
import pyref
import transcript_model as tm
from conftest import fr_bytes, rand_scalars

R = tm.R_MOD


def _int(b):
    return int.from_bytes(b, "little")


def _ints(b):
    return [int.from_bytes(b[32 * i:32 * i + 32], "little") for i in range(len(b) // 32)]


def _start(sbn, label, pos, long_filler=False):
    """library transcript + model at STROBE position pos.  The filler message is as short as the phase allows: pos_begin is then the filler's
    own operation header, or 0 where the filler crosses a block; long_filler: 166 bytes more, the same pos with pos_begin = 0 everywhere"""
    a, m = sbn.Transcript(label), tm.Transcript(label)
    p0 = m.s.pos
    k = (pos - p0 - 9) % tm.RATE
    short = k
    if long_filler:
        k += tm.RATE
    a.append_message(b"f", bytes(k)); m.append_message(b"f", bytes(k))
    assert m.s.pos == pos and a.state() == m.state()
    assert m.s.pos_begin == (0 if (long_filler or p0 + 9 + short >= tm.RATE) else p0 + 8)
    return a, m


# ---- sbn_sumcheck_prove against the replay ----------------------------------------------------------------------------------------

def _tables(ctx, count, n, seed, zero=False, value=None):
    """`count` device tables of n scalars and their canonical bytes on the host: synthetic, all zero, or `value` throughout"""
    import torch
    dev, host = [], []
    for k in range(count):
        if value is not None:
            x = torch.from_numpy(np.frombuffer(int(value).to_bytes(32, "little") * n, dtype=np.int32).reshape(n, 8).copy()).cuda()
        else:
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


def _run(ctx, sbn, ol, n_par, n_seq, logn, seed, eq=False, zero=False, claim=None, pos=29, via_rounds=False, long_filler=False, value=None, tables=None):
    """tables: (dev, host) of an earlier _tables call for this shape, used instead of fresh ones and left alive (the call only reads them)"""
    n = 1 << logn
    with_c = not eq
    dev, host = tables if tables is not None else _tables(ctx, 2 * n_par + (1 if (n_par and with_c) else 0) + 3 * n_seq, n, seed, zero, value)
    dparts, hparts = _split(dev, n_par, n_seq, with_c), _split(host, n_par, n_seq, with_c)
    rand = rand_scalars(logn, seed + 5) if eq else None
    if eq:
        hparts = hparts[:2] + (np.frombuffer(ol.eq_evals(rand), dtype=np.uint8),) + hparts[3:]
    co = rand_scalars(n_par + n_seq, seed + 2)
    claim = _int(rand_scalars(1, seed + 3)) if claim is None else claim
    tr, model = _start(sbn, b"sumcheck prove test", pos, long_filler)
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
    if tables is None:
        for t in dev:
            t.free()
    return tr, model


# ---- sbn_product_proof_prove against the model ----------------------------------------------------------------------------------------

def _upload_circuits(ctx, inputs):
    """inputs: per circuit a list of ints (2^L) -> layers[i][j] (Tables: the input, then sbn_product_circuit_many's layers down to two entries), all tables made"""
    ins = [ctx.table_upload(fr_bytes(v)) for v in inputs]
    pcs = ctx.product_circuit_many(ins)
    return [[ins[i]] + pcs[i][:-1] for i in range(len(ins))], [t for pc in pcs for t in pc] + ins


def _case_inputs(n_circ, n_dotp, L, seed, kind="uniform"):
    N, h = 1 << L, 1 << (L - 1)
    vals = pyref.prng_scalars(n_circ * N + 3 * n_dotp * h, seed)
    if kind == "zero_entries":
        vals = [0 if i % 5 == 0 else v for i, v in enumerate(vals)]
    elif kind == "zero_product":
        vals[3] = 0
    elif kind == "ones":
        vals = [1] * len(vals)
    ins = [vals[i * N:(i + 1) * N] for i in range(n_circ)]
    o = n_circ * N
    dots = [tuple(vals[o + (3 * k + t) * h:o + (3 * k + t + 1) * h] for t in range(3)) for k in range(n_dotp)]
    return ins, dots


def _proof_against_model(ctx, sbn, ins, dots, layers, dtabs, L, tr, m, what, verify=True):
    """one sbn_product_proof_prove on uploaded circuits against the model's prover from the same transcript; both transcripts move on"""
    n_circ, n_dotp = len(ins), len(dots)
    label_state = m.state()
    got = ctx.product_proof_prove(layers, dtabs, tr)
    circuits = [pm.product_circuit(v) for v in ins]
    want = pm.prove(m, circuits, dots)
    flat = pm.proof_to_flat(want)
    for name, g, w in zip(("out_polys", "out_claims", "out_rand", "out_claims_final"), got, flat):
        assert g == w, (name,) + what
    assert tr.state() == m.state(), what
    if verify:
        ok, _, _ = pm.verify(tm.Transcript.from_state(label_state), pm.proof_from_flat(*got, n_circ, n_dotp, L),
                             [pm.circuit_evaluate(c) for c in circuits], [pm.dotp_evaluate(d) for d in dots], L)
        assert ok


def _against_model(ctx, sbn, n_circ, n_dotp, L, seed, kind="uniform"):
    ins, dots = _case_inputs(n_circ, n_dotp, L, seed, kind)
    layers, owned = _upload_circuits(ctx, ins)
    dtabs = [tuple(ctx.table_upload(fr_bytes(t)) for t in d) for d in dots]
    try:
        tr = sbn.Transcript(b"product proof test"); m = tm.Transcript(b"product proof test")
        _proof_against_model(ctx, sbn, ins, dots, layers, dtabs, L, tr, m, (n_circ, n_dotp, L, kind))
        tr.free()
    finally:
        for t in owned + [t for d in dtabs for t in d]:
            t.free()
