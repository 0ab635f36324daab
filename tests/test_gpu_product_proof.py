"""GPU: sbn_product_proof_prove — the whole layered product-circuit argument in one call — against tests/product_proof_model.py
(prover and verifier in plain Python) and against the layer loop written with the entry points the call replaces.  Exact comparisons only."""
import ctypes as C

import pytest

import product_proof_model as pm
import pyref
import transcript_model as tm
from conftest import fr_bytes
from transcript_phase_lib import _against_model, _ints

pytestmark = pytest.mark.gpu
R = pyref.R
SBN_EINVAL = -1          # include/sbn254.h


def _dotp_claims(ctx, dtabs):
    out = []
    for l, r, w in dtabs:
        lv, rv, wv = (_ints(ctx.table_download(t)) for t in (l, r, w))
        out.append(sum(a * b * c for a, b, c in zip(lv, rv, wv)) % R)
    return out


def _loop(ctx, sbn, layers, dotps, tr, dotp_claims):
    """ProductCircuitEvalProofBatched::prove written with the existing entry points — the definition of the one call's values"""
    n, L, nd = len(layers), len(layers[0]), len(dotps)
    tops = [ctx.table_halves(layers[i][L - 1]) for i in range(n)]
    claims_to_verify = [a * b % R for a, b in zip(_ints(b"".join(ctx.table_read0_many([t[0] for t in tops]))), _ints(b"".join(ctx.table_read0_many([t[1] for t in tops]))))]
    rand, polys, claims, dclaims = [], b"", b"", b""
    for layer in range(L - 1, -1, -1):
        halves = [ctx.table_halves(layers[i][layer]) for i in range(n)]
        A, B = [h[0] for h in halves], [h[1] for h in halves]
        seq = dotps if layer == 0 else []
        if layer == 0 and nd:
            claims_to_verify = claims_to_verify + list(dotp_claims)       # DotProductCircuit::evaluate of every circuit (no entry point computes it: the caller's sums)
        coeffs = [tr.challenge_scalar(b"rand_coeffs_next_layer") for _ in claims_to_verify]
        claim = sum(a * int.from_bytes(c, "little") for a, c in zip(claims_to_verify, coeffs)) % R
        if len(A[0]) == 1:
            fin = ctx.table_read0_many(A) + ctx.table_read0_many(B) + [fr_bytes([1])]
            for d in range(3):
                fin += ctx.table_read0_many([s[d] for s in seq]) if seq else []
            rs = []
        else:
            st, _ = ctx.sumcheck_begin_eq(A, B, fr_bytes(rand), [s[0] for s in seq], [s[1] for s in seq], [s[2] for s in seq], b"".join(coeffs))
            lp, rs, fin = ctx.sumcheck_prove(st, tr, fr_bytes([claim]))
            st.free()
            polys += b"".join(b"".join(co) for co in lp)
            rs = _ints(b"".join(rs))
        lefts, rights = fin[:n], fin[n:2 * n]
        for a, b in zip(lefts, rights):
            tr.append_message(b"claim_prod_left", a); tr.append_message(b"claim_prod_right", b)
        claims += b"".join(lefts) + b"".join(rights)
        if seq:
            d = fin[2 * n + 1:]
            for k in range(nd):
                tr.append_message(b"claim_dotp_left", d[k]); tr.append_message(b"claim_dotp_right", d[nd + k]); tr.append_message(b"claim_dotp_weight", d[2 * nd + k])
            dclaims = b"".join(d)
        r_layer = int.from_bytes(tr.challenge_scalar(b"challenge_r_layer"), "little")
        claims_to_verify = [(a + r_layer * (b - a)) % R for a, b in zip(_ints(b"".join(lefts)), _ints(b"".join(rights)))]
        rand = [r_layer] + rs
        for h in halves:
            h[0].free(); h[1].free()
    for t in tops:
        t[0].free(); t[1].free()
    return polys, claims + dclaims, fr_bytes(rand), fr_bytes(claims_to_verify)


@pytest.mark.parametrize("n_circ", [1, 2, 4, 12, 16])
def test_against_the_model_small(ctx, sbn, n_circ):
    for n_dotp in (0, 3, 6):
        for L in range(1, 9):
            _against_model(ctx, sbn, n_circ, n_dotp, L, 1000 * n_circ + 10 * n_dotp + L)


@pytest.mark.parametrize("kind", ["zero_entries", "zero_product", "ones"])
def test_against_the_model_special_values(ctx, sbn, kind):
    _against_model(ctx, sbn, 4, 3, 5, 4242, kind)


def _synthetic(ctx, count, n, seed):
    import torch
    out = []
    for k in range(count):
        x = torch.empty((n, 8), dtype=torch.int32, device="cuda")
        ctx.scalars_synthetic(0x5BA27A2B4E254 + seed + k, 0, n, x.data_ptr())
        torch.cuda.synchronize()
        out.append(ctx.table_from_dev(x.data_ptr(), n))
        del x
    return out


def _synthetic_case(ctx, n_circ, n_dotp, L, seed):
    ins = _synthetic(ctx, n_circ, 1 << L, seed)
    pcs = ctx.product_circuit_many(ins)
    layers = [[ins[i]] + pcs[i][:-1] for i in range(n_circ)]
    flat = _synthetic(ctx, 3 * n_dotp, 1 << (L - 1), seed + 100)
    dtabs = [tuple(flat[3 * k:3 * k + 3]) for k in range(n_dotp)]
    return layers, dtabs, ins + [t for pc in pcs for t in pc] + flat


def _phase_transcripts(sbn, pos):
    """a library transcript whose STROBE position is `pos` when the proof's first challenge label arrives"""
    a = sbn.Transcript(b"phase")
    p0 = a.state()[200]
    k = (pos - p0 - 9) % tm.RATE
    a.append_message(b"f", bytes(range(k)))
    assert a.state()[200] == pos
    return a


@pytest.mark.parametrize("pos", [0, 64, 77, 78, 165])
def test_against_the_loop_every_mode_boundary(ctx, sbn, pos):
    """18 layers: the loop's sumchecks go through PLAIN-sized, SCALED and combined-kernel layers and the streaming rounds (tables >= 2^16)"""
    L = 18 if pos == 64 else 17
    layers, dtabs, owned = _synthetic_case(ctx, 8, 2, L, 300 + pos)         # (8 circuits: from there on the one call takes the combined kernels too)
    try:
        every = [t for row in layers for t in row] + [t for d in dtabs for t in d]      # every table the caller hands over
        before = [ctx.table_download(t) for t in every]
        t1 = _phase_transcripts(sbn, pos); t2 = t1.clone()
        got = ctx.product_proof_prove(layers, dtabs, t1)
        want = _loop(ctx, sbn, layers, dtabs, t2, _dotp_claims(ctx, dtabs))
        for name, g, w in zip(("out_polys", "out_claims", "out_rand", "out_claims_final"), got, want):
            assert g == w, (name, pos)
        assert t1.state() == t2.state()
        assert [ctx.table_download(t) for t in every] == before                        # the caller's tables are only read
        t1.free(); t2.free()
    finally:
        for t in owned:
            t.free()


@pytest.mark.parametrize("shape", [(12, 6, 22), (4, 0, 21)])
def test_keyless_shape(ctx, sbn, shape):
    n_circ, n_dotp, L = shape
    layers, dtabs, owned = _synthetic_case(ctx, n_circ, n_dotp, L, 900 + L)
    try:
        probe = layers[0] + layers[n_circ - 1] + [t for d in dtabs for t in d]      # every layer of the first and the last circuit, every dot-product table
        before = [ctx.table_download(t) for t in probe]
        t1 = sbn.Transcript(b"keyless shape"); t2 = t1.clone()
        got = ctx.product_proof_prove(layers, dtabs, t1)
        claims_dotp = _dotp_claims(ctx, dtabs)
        want = _loop(ctx, sbn, layers, dtabs, t2, claims_dotp)
        for name, g, w in zip(("out_polys", "out_claims", "out_rand", "out_claims_final"), got, want):
            assert g == w, name
        assert t1.state() == t2.state()
        assert [ctx.table_download(t) for t in probe] == before            # the caller's tables are only read
        # the model verifier: the circuits' products and the dot products as the claims
        tops = [ctx.table_download(layers[i][L - 1]) for i in range(n_circ)]
        claims_prod = [int.from_bytes(t[:32], "little") * int.from_bytes(t[32:], "little") % R for t in tops]
        ok, claims, rand = pm.verify(tm.Transcript(b"keyless shape"), pm.proof_from_flat(*got, n_circ, n_dotp, L), claims_prod, claims_dotp, L)
        assert ok
        # the statement the argument reduces to
        for i in range(n_circ):
            assert ctx.table_evaluate(layers[i][0], got[2]) == got[3][32 * i:32 * i + 32], i
        t1.free(); t2.free()
    finally:
        for t in owned:
            t.free()


def test_errors_leave_the_transcript_alone(ctx, sbn):
    layers, dtabs, owned = _synthetic_case(ctx, 2, 1, 4, 77)
    lib = sbn.lib()
    try:
        tr = sbn.Transcript(b"errors"); before = tr.state()
        n, L = 2, 4
        bufs = [(C.c_uint8 * 8192)() for _ in range(4)]
        arr = lambda ts: (C.c_void_p * len(ts))(*[t.h for t in ts])
        good = [layers[i][j] for i in range(n) for j in range(L)]
        d = [arr([x[k] for x in dtabs]) for k in range(3)]
        call = lambda la, nc, nl, nd, trh: lib.sbn_product_proof_prove(ctx.h, la, C.c_size_t(nc), C.c_size_t(nl), d[0], d[1], d[2], C.c_size_t(nd), trh, *bufs)
        assert call(arr(good), n, L, 1, tr.h) == 0                           # the arguments are fine as they are ...
        tr.free(); tr = sbn.Transcript(b"errors")
        bad = list(good); bad[1], bad[2] = bad[2], bad[1]                    # ... unequal lengths: two layers swapped
        assert call(arr(bad), n, L, 1, tr.h) == SBN_EINVAL and tr.state() == before
        assert call(arr(good), n, L - 1, 1, tr.h) == SBN_EINVAL and tr.state() == before      # the dot-product circuits no longer fit the depth
        many = arr([layers[0][j] for _ in range(24) for j in range(L)])
        assert call(many, 24, L, 1, tr.h) == SBN_EINVAL and tr.state() == before              # 24 + 1 instances
        assert call(arr(good), n, L, 1, None) == SBN_EINVAL                                   # a null transcript
        holes = arr(good); holes[5] = None
        assert call(holes, n, L, 1, tr.h) == SBN_EINVAL and tr.state() == before              # a null entry among the layers
        short = ctx.table_halves(dtabs[0][2])
        d_good = d[2]; d[2] = arr([short[0]])
        assert call(arr(good), n, L, 1, tr.h) == SBN_EINVAL and tr.state() == before          # one dot-product table shorter than the other two
        d[2] = d_good; short[0].free(); short[1].free()
        # "A dead state" cannot be handed to this call: it takes no sumcheck state, and a transcript only comes from sbn_transcript_new / _clone /
        # _from_state, the last of which refuses records no STROBE-128 transcript can be in (tests/test_transcript_cpu.py) — so the call has no such check.
        assert call(arr(good), 0, L, 1, tr.h) == SBN_EINVAL and tr.state() == before
        tr.free()
    finally:
        for t in owned:
            t.free()
