"""CPU: the literal model of PolyEvalProof (tests/polyeval_model.py) proves and verifies, rejects tampered proofs, and the library exports the
one-call opening with its argument checks.  The model is what tests/test_gpu_polyeval.py holds the device's bytes against."""
import ctypes as C
import random

import pytest

import polyeval_model as pm
from polyeval_model import R_MOD, Transcript

LABEL = b"gens_polyeval_test"


def _case(ol, ell, with_blinds, seed):
    rng = random.Random(seed)
    ml, mr = pm.factored_lens(ell)
    n = 1 << mr
    gens = pm.split_gens(ol.gens_new(n + 1, LABEL)[0], n)
    Z = [rng.randrange(R_MOD) for _ in range(1 << ell)]
    r = [rng.randrange(R_MOD) for _ in range(ell)]
    blinds = [rng.randrange(R_MOD) for _ in range(1 << ml)] if with_blinds else None
    blind_Zr = rng.randrange(R_MOD) if with_blinds else None
    rnd = [rng.randrange(R_MOD) for _ in range(3 + 2 * mr)]
    Zr = pm.dot(Z, pm.eq_evals(r))                          # DensePolynomial::evaluate (hyrax.rs:217-222)
    return gens, Z, r, blinds, blind_Zr, rnd, Zr


@pytest.mark.parametrize("with_blinds", [False, True])
@pytest.mark.parametrize("ell", range(1, 9))
def test_model_prove_then_verify(ol, ell, with_blinds):
    gens, Z, r, blinds, blind_Zr, rnd, Zr = _case(ol, ell, with_blinds, 100 + ell)
    tp = Transcript(b"polyeval")
    proof, C_Zr, Cx = pm.prove(tp, gens, Z, blinds, r, Zr, blind_Zr, rnd)
    comm = pm.commit_poly(gens, Z, blinds, ell)
    assert pm.msm(pm.eq_evals(r[:ell // 2]), comm) == Cx      # C_LZ of the verifier is the prover's Cx
    tv = Transcript(b"polyeval")
    assert pm.verify(tv, proof, gens, r, C_Zr, comm)
    assert tv.state() == tp.state()                          # both sides end on the same transcript
    back = pm.proof_from_bytes(pm.proof_bytes(proof))
    assert back == proof
    if not with_blinds:
        assert pm.verify_plain(Transcript(b"polyeval"), proof, gens, r, Zr, comm)


@pytest.mark.parametrize("what", ["L_0", "R_last", "delta", "beta", "z1", "z2", "Zr"])
def test_model_verify_rejects_a_flipped_value(ol, what):
    ell = 5
    gens, Z, r, blinds, blind_Zr, rnd, Zr = _case(ol, ell, True, 7)
    proof, C_Zr, _ = pm.prove(Transcript(b"polyeval"), gens, Z, blinds, r, Zr, blind_Zr, rnd)
    comm = pm.commit_poly(gens, Z, blinds, ell)
    assert pm.verify(Transcript(b"polyeval"), proof, gens, r, C_Zr, comm)
    bad = {k: (list(v) if isinstance(v, list) else v) for k, v in proof.items()}
    gen = ol.g1_mul_gen_batch(pm.sb(1), 1)
    if what == "L_0":
        bad["L"][0] = ol.g1_add(bad["L"][0], gen)
    elif what == "R_last":
        bad["R"][-1] = ol.g1_add(bad["R"][-1], gen)
    elif what in ("delta", "beta"):
        bad[what] = ol.g1_add(bad[what], gen)
    elif what in ("z1", "z2"):
        bad[what] = (bad[what] + 1) % R_MOD
    else:
        C_Zr = ol.g1_add(pm.mul(gens[1], (Zr + 1) % R_MOD), pm.mul(gens[2], blind_Zr))      # a commitment to another Zr
    assert not pm.verify(Transcript(b"polyeval"), bad, gens, r, C_Zr, comm)


def test_model_joint_opening_verifies(ol):
    """prove_single: the opening of the merged polynomial at challenges || r is an opening of the joint claim"""
    rng = random.Random(11)
    count, ell_r = 4, 3
    ell = 2 + ell_r
    n = 1 << pm.factored_lens(ell)[1]
    gens = pm.split_gens(ol.gens_new(n + 1, LABEL)[0], n)
    polys = [[rng.randrange(R_MOD) for _ in range(1 << ell_r)] for _ in range(count)]
    r = [rng.randrange(R_MOD) for _ in range(ell_r)]
    evals = [pm.dot(p, pm.eq_evals(r)) for p in polys]
    Z = [x for p in polys for x in p]                       # DensePolynomial::merge (hyrax.rs:237-247)
    rnd = [rng.randrange(R_MOD) for _ in range(3 + 2 * (n.bit_length() - 1))]
    tp = Transcript(b"joint")
    ch, claim, proof, C_Zr, _ = pm.prove_single(tp, gens, Z, r, evals, rnd)
    assert claim == pm.dot(Z, pm.eq_evals(ch + r))
    tv = Transcript(b"joint")
    for e in evals:
        tv.append_scalar(b"evals_ops_val", e)
    assert [tv.challenge_scalar(b"challenge_combine_n_to_one") for _ in range(2)] == ch
    tv.append_scalar(b"joint_claim_eval", claim)
    assert pm.verify_plain(tv, proof, gens, ch + r, claim, pm.commit_poly(gens, Z, None, ell))
    assert tv.state() == tp.state()


def test_library_exports_the_one_call_opening_and_checks_its_arguments(sbn):
    """no device here: the symbols exist, and a call without a context (whatever else is wrong with it) is SBN_EINVAL, never a crash"""
    L = sbn.lib()
    for name in ("sbn_polyeval_prove", "sbn_joint_opening_prove", "sbn_prof_last_polyeval", "sbn_prof_last_acc"):
        assert hasattr(L, name)
    tr = sbn.Transcript(b"polyeval")
    before = tr.state()
    buf = lambda k: (C.c_uint8 * k)()                      # noqa: E731
    xi, yi = C.c_int(0), C.c_int(0)
    good_rnd = bytes(32 * 5)
    bad_rnd = bytes(32 * 4) + b"\xff" * 32                  # >= r: not canonical
    fake = C.c_void_p(0)
    for ell, rnd in ((2, good_rnd), (0, good_rnd), (2, bad_rnd)):
        rc = L.sbn_polyeval_prove(None, fake, fake, None, buf(64), C.c_size_t(ell), buf(32), None, rnd, tr.h, buf(256), buf(64), C.byref(xi), buf(64), C.byref(yi))
        assert rc == -1                                     # SBN_EINVAL
    rc = L.sbn_joint_opening_prove(None, fake, fake, buf(64), C.c_size_t(2), b"e", C.c_size_t(1), b"c", C.c_size_t(1), b"j", C.c_size_t(1), buf(32), C.c_size_t(1),
                                   good_rnd, tr.h, buf(32), buf(32), buf(256), buf(64), C.byref(xi), buf(64), C.byref(yi))
    assert rc == -1
    assert L.sbn_prof_last_polyeval(None, (C.c_double * 3)()) == -1
    assert L.sbn_prof_last_acc(None, (C.c_uint64 * 8)()) == -1
    assert tr.state() == before                             # a failed call leaves the transcript as it was
