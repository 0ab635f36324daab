"""CPU: tests/r1cs_proof_verify_model.py — the single-sum form of R1CSProof::verify that sbn_r1cs_proof_verify runs on the device — against the
literal restatement of the reference (r1cs_proof_model.verify, zk_sumcheck_model.verify): the same verdict and the same transcript on honest
proofs, and a refusal wherever the literal verifier refuses."""
import random

import pytest

import polyeval_model as pm
import r1cs_model as rm
import r1cs_proof_model as rpm
import r1cs_proof_verify_model as vm
import zk_sumcheck_model as zm
from r1cs_proof_model import R_MOD, Transcript

SHAPES = [(2, 2, 0), (2, 2, 1), (4, 4, 1), (8, 4, 3), (4, 8, 0)]
TAMPER_SHAPE = (8, 4, 3)
LABEL = b"gens_r1cs_verify_cpu"
TR_LABEL = b"r1cs proof verify cpu"
_CACHE = {}


def _gens(ol, nv):
    R = 1 << pm.factored_lens(rpm.log2(nv))[1]
    if R not in _CACHE:
        _CACHE[R] = rpm.make_gens(ol.gens_new(R + 1, LABEL + b"_pc")[0], R, ol.gens_new(3, LABEL + b"_sc")[0], ol.gens_new(4, LABEL + b"_sc")[0])
    return _CACHE[R]


def _proved(ol, shape):
    """one honest proof per shape for the whole module -> (mats, inputs, gens, proof bytes, rx, ry, evals, the prover's end state)"""
    if shape not in _CACHE:
        nc, nv, n_in = shape
        mats, vars_, inputs = rpm.satisfying_instance(nc, nv, n_in, 3000 + nc * 64 + nv)
        gens = _gens(ol, nv)
        tr = Transcript(TR_LABEL)
        proof, rx, ry = rpm.prove(tr, nc, nv, mats, vars_, inputs, gens, rpm.random_rnd(nc, nv, 11 * nc + nv))
        _CACHE[shape] = (mats, inputs, gens, rpm.proof_bytes(proof), rx, ry, rm.evaluate(nc, nv, mats, rx, ry), tr.state())
    return _CACHE[shape]


def _literal(proof, nc, nv, inputs, evals, gens):
    """the literal verifier on the same bytes -> ((rx, ry) or None, end state)"""
    tr = Transcript(TR_LABEL)
    p = rpm.proof_from_bytes(proof, nc, nv)
    return (None if p is None else rpm.verify(tr, p, nv, nc, inputs, evals, gens)), tr.state()


@pytest.mark.parametrize("shape", SHAPES)
def test_honest_proofs_same_verdict_and_transcript_as_the_literal_verifier(ol, shape):
    nc, nv, _ = shape
    mats, inputs, gens, proof, rx, ry, evals, state = _proved(ol, shape)
    want, want_state = _literal(proof, nc, nv, inputs, evals, gens)
    assert want == (rx, ry) and want_state == state
    tr = Transcript(TR_LABEL)
    got = vm.verify(tr, proof, nc, nv, inputs, evals, gens)
    assert got is not None and got[:2] == (rx, ry)
    assert tr.state() == state
    run = got[2]
    nr = rpm.log2(nc) + rpm.log2(nv) + 1
    assert len(run.T) == 4 * nr + 22 and len(run.eqs) == 2 * nr + 6 and run.sums == nr + 3
    assert max(len(e) for e in run.eqs) <= vm.TERMS_MAX


def _tamperings(ol):
    nc, nv, _ = TAMPER_SHAPE
    return vm.tamperings(_proved(ol, TAMPER_SHAPE)[3], nc, nv)


TAMPER_NAMES = ["flipped byte in " + f for f in rpm.FIELDS] + ["comm_Az_claim does not decompress", "delta of round 0 does not decompress",
                                                               "z of the first equality proof >= r", "z[0] of phase 2 round 0 is z + r"]


@pytest.mark.parametrize("name", TAMPER_NAMES)
def test_every_tampering_the_literal_verifier_refuses_is_refused(ol, name):
    nc, nv, _ = TAMPER_SHAPE
    mats, inputs, gens, proof, rx, ry, evals, _ = _proved(ol, TAMPER_SHAPE)
    cases = _tamperings(ol)
    assert sorted(cases) == sorted(TAMPER_NAMES)
    bad = cases[name]
    assert bad != proof and len(bad) == len(proof)
    assert _literal(bad, nc, nv, inputs, evals, gens)[0] is None
    tr = Transcript(TR_LABEL)
    state0 = tr.state()
    assert vm.verify(tr, bad, nc, nv, inputs, evals, gens) is None
    assert tr.state() == state0


def test_wrong_evals_a_wrong_input_and_a_changed_instance_are_refused(ol):
    nc, nv, _ = TAMPER_SHAPE
    mats, inputs, gens, proof, rx, ry, evals, _ = _proved(ol, TAMPER_SHAPE)
    for k in range(3):
        wrong = list(evals); wrong[k] = (wrong[k] + 1) % R_MOD
        assert _literal(proof, nc, nv, inputs, wrong, gens)[0] is None
        assert vm.verify(Transcript(TR_LABEL), proof, nc, nv, inputs, wrong, gens) is None
    for k in range(len(inputs)):
        wrong = list(inputs); wrong[k] = (wrong[k] + 1) % R_MOD
        assert _literal(proof, nc, nv, wrong, evals, gens)[0] is None
        assert vm.verify(Transcript(TR_LABEL), proof, nc, nv, wrong, evals, gens) is None
    A, B, (cr, cc, cv) = mats
    changed = (A, B, (cr, cc, [(cv[0] + 1) % R_MOD] + cv[1:]))
    ev2 = rm.evaluate(nc, nv, changed, rx, ry)
    assert ev2 != evals
    assert _literal(proof, nc, nv, inputs, ev2, gens)[0] is None
    assert vm.verify(Transcript(TR_LABEL), proof, nc, nv, inputs, ev2, gens) is None
    # the honest prover on the unsatisfied instance, checked with that instance's own evaluations
    vars_ = rpm.satisfying_instance(nc, nv, TAMPER_SHAPE[2], 3000 + nc * 64 + nv)[1]
    p2, rx2, ry2 = rpm.prove(Transcript(TR_LABEL), nc, nv, changed, vars_, inputs, gens, rpm.random_rnd(nc, nv, 5))
    b2, e2 = rpm.proof_bytes(p2), rm.evaluate(nc, nv, changed, rx2, ry2)
    assert _literal(b2, nc, nv, inputs, e2, gens)[0] is None
    assert vm.verify(Transcript(TR_LABEL), b2, nc, nv, inputs, e2, gens) is None


@pytest.mark.parametrize("degree", [2, 3])
@pytest.mark.parametrize("rounds", [1, 2, 3])
def test_the_sumcheck_check_alone_against_the_literal_verifier(ol, rounds, degree):
    rng = random.Random(100 * degree + rounds)
    gens = _gens(ol, 4)
    g1, gn = gens["g1"], gens["g3" if degree == 2 else "g4"]
    n = degree + 1
    tabs = [[rng.randrange(R_MOD) for _ in range(1 << rounds)] for _ in range(2 if degree == 2 else 4)]
    claim = zm.dot(*tabs) if degree == 2 else sum(t * (a * b - c) for t, a, b, c in zip(*tabs)) % R_MOD
    blind = rng.randrange(R_MOD)
    rnd = [rng.randrange(R_MOD) for _ in range(rounds * (n + 4))]
    tp = Transcript(TR_LABEL)
    proof, r, _, _ = (zm.prove_quad if degree == 2 else zm.prove_r1cs)(tp, rnd, claim, blind, *tabs, g1, gn)
    comm_claim = zm.commit_one(claim, blind, g1)
    tl = Transcript(TR_LABEL)
    want = zm.verify(tl, proof, comm_claim, rounds, degree, g1, gn)
    assert want is not None and want[1] == r and tl.state() == tp.state()
    tv = Transcript(TR_LABEL)
    got = vm.zk_verify(tv, zm.proof_bytes(proof), comm_claim, rounds, degree, g1, gn)
    assert got is not None and got[:2] == want and tv.state() == tp.state()
    assert len(got[2].eqs) == 2 * rounds and got[2].sums == rounds
    wrong = zm.commit_one((claim + 1) % R_MOD, blind, g1)
    tv = Transcript(TR_LABEL)
    assert zm.verify(Transcript(TR_LABEL), proof, wrong, rounds, degree, g1, gn) is None
    assert vm.zk_verify(tv, zm.proof_bytes(proof), wrong, rounds, degree, g1, gn) is None and tv.state() == Transcript(TR_LABEL).state()
