"""CPU: the model of the layered product-circuit argument (tests/product_proof_model.py) against itself — prover against verifier — and
the host transcript (sbn_transcript_*) over a layer boundary's operation sequence at every start phase; the export of sbn_product_proof_prove.

No GPU.  All comparisons are exact."""
import os
import re

import pytest

import product_proof_model as pm
import pyref
import transcript_model as tm

R = pyref.R
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _inputs(n_circ, n_dotp, n_layers, seed):
    vals = pyref.prng_scalars(n_circ * (1 << n_layers) + 3 * n_dotp * (1 << (n_layers - 1)), seed)
    N, h = 1 << n_layers, 1 << (n_layers - 1)
    circuits = [pm.product_circuit(vals[i * N:(i + 1) * N]) for i in range(n_circ)]
    o = n_circ * N
    dotps = [tuple(vals[o + (3 * k + t) * h:o + (3 * k + t + 1) * h] for t in range(3)) for k in range(n_dotp)]
    return circuits, dotps


def _prove_verify(n_circ, n_dotp, n_layers, seed=7, **kw):
    circuits, dotps = _inputs(n_circ, n_dotp, n_layers, seed)
    tp, tv = tm.Transcript(b"product proof"), tm.Transcript(b"product proof")
    proof = pm.prove(tp, circuits, dotps, **kw)
    return circuits, dotps, proof, tp, tv


def _verify(tv, proof, circuits, dotps):
    return pm.verify(tv, proof, [pm.circuit_evaluate(c) for c in circuits], [pm.dotp_evaluate(d) for d in dotps], len(circuits[0]))


def test_model_known_answers_of_the_reference():
    # product_tree.rs:544-590: 2 * 3 * 5 * 7 = 210; 1*5 + 2*6 + 3*7 + 4*8 = 70
    assert pm.circuit_evaluate(pm.product_circuit([2, 3, 5, 7])) == 210
    assert pm.dotp_evaluate(([1, 2, 3, 4], [5, 6, 7, 8], [1, 1, 1, 1])) == 70


@pytest.mark.parametrize("n_layers", [1, 2, 5])
@pytest.mark.parametrize("n_dotp", [0, 3])
@pytest.mark.parametrize("n_circ", [1, 3, 12])
def test_verifier_accepts_the_prover(n_circ, n_dotp, n_layers):
    circuits, dotps, proof, tp, tv = _prove_verify(n_circ, n_dotp, n_layers)
    ok, claims, rand = _verify(tv, proof, circuits, dotps)
    assert ok
    assert tp.state() == tv.state()                       # prover and verifier leave the same transcript
    assert len(rand) == n_layers
    # the statement the argument reduces to: layer 0 (left || right) of every circuit at rand
    for c, claim in zip(circuits, claims):
        assert pm.evaluate_mle(c[0][0] + c[0][1], rand) == claim
    # ... and the dot-product claims are the three tables at rand[1:]
    for k, d in enumerate(dotps):
        for t in range(3):
            assert pm.evaluate_mle(d[t], rand[1:]) == proof["claims_dotp"][t][k]
    # the flat layout round-trips
    flat = pm.proof_to_flat(proof)
    assert pm.proof_from_flat(*flat, n_circ, n_dotp, n_layers) == proof
    assert len(flat[0]) == 128 * (n_layers * (n_layers - 1) // 2) and len(flat[1]) == 32 * (2 * n_circ * n_layers + 3 * n_dotp)


@pytest.mark.parametrize("which", ["polys", "claims_left", "claims_right", "claims_dotp", "rand", "claims_final"])
def test_verifier_rejects_one_changed_scalar(which):
    circuits, dotps, proof, _, _ = _prove_verify(3, 3, 5)
    assert _verify(tm.Transcript(b"product proof"), proof, circuits, dotps)[0]
    bump = lambda x: (x + 1) % R
    if which == "polys":
        spots = [(lambda p, i=i, j=j, k=k: p["polys"][i][j].__setitem__(k, bump(p["polys"][i][j][k]))) for i in range(5) for j in range(i) for k in range(4)]
    elif which in ("claims_left", "claims_right"):
        s = 0 if which == "claims_left" else 1
        spots = [(lambda p, i=i, k=k: p["claims"][i][s].__setitem__(k, bump(p["claims"][i][s][k]))) for i in range(5) for k in range(3)]
    elif which == "claims_dotp":
        spots = [(lambda p, t=t, k=k: p["claims_dotp"][t].__setitem__(k, bump(p["claims_dotp"][t][k]))) for t in range(3) for k in range(3)]
    else:
        spots = [(lambda p, k=k: p[which].__setitem__(k, bump(p[which][k]))) for k in range(len(proof[which]))]
    for change in spots:                                   # every single position of that output array
        bad = pm.proof_from_flat(*pm.proof_to_flat(proof), 3, 3, 5)
        change(bad)
        assert bad != proof
        assert not _verify(tm.Transcript(b"product proof"), bad, circuits, dotps)[0]


@pytest.mark.parametrize("n_layers", [1, 2, 5])
def test_verifier_rejects_a_proof_without_the_zero_round_layer(n_layers):
    circuits, dotps, proof, _, tv = _prove_verify(3, 3 if n_layers > 1 else 0, n_layers, skip_zero_round_layer=True)
    assert not _verify(tv, proof, circuits, dotps)[0]


# ---- the library ---------------------------------------------------------------------------------------------------------------

def test_library_exports_and_declares_the_call(sbn):
    assert "sbn_product_proof_prove" in sbn.EXPORTED_SYMBOLS
    assert hasattr(sbn.lib(), "sbn_product_proof_prove")
    with open(os.path.join(ROOT, "include", "sbn254.h")) as f:
        assert re.search(r"\bint\s+sbn_product_proof_prove\s*\(\s*sbn_ctx\s*\*", f.read())
    assert callable(getattr(sbn.Context, "product_proof_prove"))


def _at_phase(sbn, pos):
    a, m = sbn.Transcript(b"phase"), tm.Transcript(b"phase")
    k = (pos - m.s.pos - 9) % tm.RATE                      # append_message moves pos by 2 + len(label) + 4 + 2 + len(msg) modulo the rate
    fill = bytes(range(k))
    a.append_message(b"f", fill); m.append_message(b"f", fill)
    assert m.s.pos == pos
    return a, m


@pytest.mark.parametrize("n", [1, 18, 24])
def test_every_start_phase_of_a_layer_boundary(sbn, n):
    """n coefficients, the claim appends (n_circ = n - n_dotp circuits, n_dotp = min(6, n - 1) dot-product circuits), challenge_r_layer"""
    n_dotp = min(6, n - 1); n_circ = n - n_dotp
    vals = [v.to_bytes(32, "little") for v in pyref.prng_scalars(2 * n_circ + 3 * n_dotp, 99 + n)]
    for pos in range(tm.RATE):
        a, m = _at_phase(sbn, pos)
        assert a.state() == m.state()
        for _ in range(n):
            assert int.from_bytes(a.challenge_scalar(b"rand_coeffs_next_layer"), "little") == m.challenge_scalar(b"rand_coeffs_next_layer"), pos
        assert a.state() == m.state()
        it = iter(vals)
        for _ in range(n_circ):
            for label in (b"claim_prod_left", b"claim_prod_right"):
                v = next(it); a.append_message(label, v); m.append_message(label, v)
        for _ in range(n_dotp):
            for label in (b"claim_dotp_left", b"claim_dotp_right", b"claim_dotp_weight"):
                v = next(it); a.append_message(label, v); m.append_message(label, v)
        assert a.state() == m.state()
        assert int.from_bytes(a.challenge_scalar(b"challenge_r_layer"), "little") == m.challenge_scalar(b"challenge_r_layer"), pos
        assert a.state() == m.state()
        a.free()
