"""CPU: tests/r1cs_proof_model.py — the literal restatement of R1CSProof::prove / ::verify (r1csproof.rs:241-619) and of the three Σ-protocols of
nizk/mod.rs that sbn_r1cs_proof_prove is checked against.  The model's prover and verifier must agree with each other (completeness and the
same transcript), the verifier must reject what it should, and the row form the device uses for ProductProof's delta must be the same
group element."""
import random

import pytest

import polyeval_model as pm
import r1cs_proof_model as rpm
import zk_sumcheck_model as zm
from r1cs_proof_model import R_MOD, Transcript

SHAPES = [(2, 2, 0), (2, 2, 1), (4, 4, 1), (8, 4, 3), (4, 8, 0), (16, 16, 15)]
LABEL = b"gens_r1cs_proof_cpu"
_CACHE = {}


def _gens(ol, nv):
    R = 1 << pm.factored_lens(rpm.log2(nv))[1]
    if R not in _CACHE:
        _CACHE[R] = rpm.make_gens(ol.gens_new(R + 1, LABEL + b"_pc")[0], R, ol.gens_new(3, LABEL + b"_sc")[0], ol.gens_new(4, LABEL + b"_sc")[0])
    return _CACHE[R]


def _proved(ol, shape):
    """one honest proof per shape for the whole module"""
    if shape not in _CACHE:
        nc, nv, n_in = shape
        mats, vars_, inputs = rpm.satisfying_instance(nc, nv, n_in, 1000 + nc * 64 + nv)
        gens = _gens(ol, nv)
        tr = Transcript(b"r1cs proof cpu")
        proof, rx, ry = rpm.prove(tr, nc, nv, mats, vars_, inputs, gens, rpm.random_rnd(nc, nv, nc + nv))
        _CACHE[shape] = (mats, vars_, inputs, gens, proof, rx, ry, tr.state())
    return _CACHE[shape]


@pytest.mark.parametrize("shape", SHAPES)
def test_prove_then_verify_accepts_and_ends_in_the_same_state(ol, shape):
    nc, nv, n_in = shape
    mats, vars_, inputs, gens, proof, rx, ry, state = _proved(ol, shape)
    assert len(rx) == rpm.log2(nc) and len(ry) == rpm.log2(nv) + 1
    tv = Transcript(b"r1cs proof cpu")
    got = rpm.verify_instance(tv, proof, nc, nv, mats, inputs, gens)
    assert got == (rx, ry)
    assert tv.state() == state
    b = rpm.proof_bytes(proof)
    assert len(b) == rpm.sizes(nc, nv)[1]
    assert rpm.proof_bytes(rpm.proof_from_bytes(b, nc, nv)) == b


@pytest.mark.parametrize("field", rpm.FIELDS)
def test_verifier_rejects_a_flipped_byte_in_each_field(ol, field):
    shape = (8, 4, 3)
    nc, nv, _ = shape
    mats, vars_, inputs, gens, proof, rx, ry, _ = _proved(ol, shape)
    b = bytearray(rpm.proof_bytes(proof))
    lo, hi = rpm.field_spans(nc, nv)[field]
    b[hi - 32] ^= 1                                         # the lowest byte of the field's last element: an x coordinate or a scalar
    bad = rpm.proof_from_bytes(bytes(b), nc, nv)
    assert bad is None or rpm.verify_instance(Transcript(b"r1cs proof cpu"), bad, nc, nv, mats, inputs, gens) is None


def test_verifier_rejects_the_proof_of_a_changed_instance(ol):
    shape = (8, 4, 3)
    nc, nv, _ = shape
    mats, vars_, inputs, gens, proof, _, _, _ = _proved(ol, shape)
    A, B, (cr, cc, cv) = mats
    changed = (A, B, (cr, cc, [cv[0] + 1] + cv[1:]))
    assert rpm.verify_instance(Transcript(b"r1cs proof cpu"), proof, nc, nv, changed, inputs, gens) is None
    # and an honest run of the prover on the unsatisfied instance is rejected too
    tr = Transcript(b"r1cs proof cpu")
    p2, _, _ = rpm.prove(tr, nc, nv, changed, vars_, inputs, gens, rpm.random_rnd(nc, nv, 5))
    assert rpm.verify_instance(Transcript(b"r1cs proof cpu"), p2, nc, nv, changed, inputs, gens) is None


def test_each_sigma_protocol_accepts_its_proof_and_rejects_a_changed_response(ol):
    rng = random.Random(7)
    g1 = _gens(ol, 4)["g1"]
    rs = lambda k: [rng.randrange(R_MOD) for _ in range(k)]          # noqa: E731
    x, r, t1, t2 = rs(4)
    tp, tv = Transcript(b"sigma"), Transcript(b"sigma")
    p, C = rpm.knowledge_prove(tp, g1, t1, t2, x, r)
    assert C == zm.commit_one(x, r, g1)
    assert rpm.knowledge_verify(tv, g1, p, C) and tv.state() == tp.state()
    for k in ("z1", "z2"):
        assert not rpm.knowledge_verify(Transcript(b"sigma"), g1, dict(p, **{k: (p[k] + 1) % R_MOD}), C)
    v, s1, s2, rr = rs(4)
    tp, tv = Transcript(b"sigma"), Transcript(b"sigma")
    p, C1, C2 = rpm.equality_prove(tp, g1, rr, v, s1, v, s2)
    assert rpm.equality_verify(tv, g1, p, C1, C2) and tv.state() == tp.state()
    assert not rpm.equality_verify(Transcript(b"sigma"), g1, dict(p, z=(p["z"] + 1) % R_MOD), C1, C2)
    p, C1, C2 = rpm.equality_prove(Transcript(b"sigma"), g1, rr, v, s1, (v + 1) % R_MOD, s2)      # unequal values: no valid proof
    assert not rpm.equality_verify(Transcript(b"sigma"), g1, p, C1, C2)
    x, rX, y, rY, rZ = rs(5)
    tp, tv = Transcript(b"sigma"), Transcript(b"sigma")
    p, X, Y, Z = rpm.product_prove(tp, g1, rs(5), x, rX, y, rY, x * y % R_MOD, rZ)
    assert rpm.product_verify(tv, g1, p, X, Y, Z) and tv.state() == tp.state()
    for k in range(5):
        z = list(p["z"]); z[k] = (z[k] + 1) % R_MOD
        assert not rpm.product_verify(Transcript(b"sigma"), g1, dict(p, z=z), X, Y, Z)
    p, X, Y, Z = rpm.product_prove(Transcript(b"sigma"), g1, rs(5), x, rX, y, rY, (x * y + 1) % R_MOD, rZ)
    assert not rpm.product_verify(Transcript(b"sigma"), g1, p, X, Y, Z)


def test_delta_over_the_fresh_point_is_a_row_over_gens_1(ol):
    """ProductProof's delta = b3 * X + b5 * h with X = x * G + rX * h (nizk/mod.rs:202-205) is the commitment of [b3 x, b3 rX + b5] over gens_1"""
    rng = random.Random(11)
    g1 = _gens(ol, 4)["g1"]
    cases = [[rng.randrange(R_MOD) for _ in range(4)] for _ in range(4)]
    cases += [[0, rng.randrange(R_MOD), rng.randrange(R_MOD), rng.randrange(R_MOD)], [0, 0, 5, 0], [3, 4, 0, 0]]
    for x, rX, b3, b5 in cases:
        X = zm.commit_one(x, rX, g1)
        assert zm.commit_one(b3, b5, (X, g1[1])) == zm.commit_one(b3 * x % R_MOD, (b3 * rX + b5) % R_MOD, g1)


@pytest.mark.parametrize("shape", SHAPES)
def test_size_formulas_against_what_the_model_produces(ol, shape):
    nc, nv, _ = shape
    n_rnd, n_bytes = rpm.sizes(nc, nv)
    proof = _proved(ol, shape)[4]                           # (prove asserts that the tape of n_rnd scalars is used up exactly)
    assert len(rpm.proof_bytes(proof)) == n_bytes
    assert rpm.field_spans(nc, nv)[rpm.FIELDS[-1]][1] == n_bytes
    nx, ell = rpm.log2(nc), rpm.log2(nv)
    ml, lg = pm.factored_lens(ell)
    assert n_rnd == (1 << ml) + 8 * nx + 7 * (ell + 1) + 2 * lg + 17
    assert rpm.sizes(1 << 20, 1 << 20) == (1368, 46624)
