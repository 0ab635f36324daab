"""CPU: the single-sum form of the opening check (tests/polyeval_verify_model.py) says what the literal verifier (tests/polyeval_model.py) says,
on honest proofs and on every tampered one of the reject list; the closed form of b_hat is the dot product; the library exports the one-call
verifier and refuses a call without a context."""
import ctypes as C
import random

import pytest

import polyeval_model as pm
import polyeval_verify_model as pvm
from polyeval_model import R_MOD, Transcript

LABEL, OTHER_LABEL = b"gens_polyeval_test", b"gens_polyeval_other"


def _case(ol, ell, with_blinds, seed):
    rng = random.Random(seed)
    ml, mr = pm.factored_lens(ell)
    n = 1 << mr
    gens = pm.split_gens(ol.gens_new(n + 1, LABEL)[0], n)
    other = pm.split_gens(ol.gens_new(n + 1, OTHER_LABEL)[0], n)
    Z = [rng.randrange(R_MOD) for _ in range(1 << ell)]
    r = [rng.randrange(R_MOD) for _ in range(ell)]
    blinds = [rng.randrange(R_MOD) for _ in range(1 << ml)] if with_blinds else None
    blind_Zr = rng.randrange(R_MOD) if with_blinds else None
    rnd = [rng.randrange(R_MOD) for _ in range(3 + 2 * mr)]
    Zr = pm.dot(Z, pm.eq_evals(r))
    proof, C_Zr, _ = pm.prove(Transcript(b"polyeval"), gens, Z, blinds, r, Zr, blind_Zr, rnd)
    return gens, other, r, proof, C_Zr, pm.commit_poly(gens, Z, blinds, ell)


@pytest.mark.parametrize("with_blinds", [False, True])
@pytest.mark.parametrize("ell", range(1, 8))
def test_folded_check_accepts_what_the_literal_verifier_accepts(ol, ell, with_blinds):
    gens, _, r, proof, C_Zr, comm = _case(ol, ell, with_blinds, 500 + ell)
    tl, tf = Transcript(b"polyeval"), Transcript(b"polyeval")
    assert pm.verify(tl, proof, gens, r, C_Zr, comm)
    assert pvm.verify_folded(tf, proof, gens, r, C_Zr, comm)
    assert tf.state() == tl.state()


@pytest.mark.parametrize("ell", [1, 2, 5])
def test_folded_check_rejects_every_tampering_the_literal_verifier_rejects(ol, ell):
    gens, other, r, proof, C_Zr, comm = _case(ol, ell, True, 520 + ell)
    names = pvm.tamperings(ell)
    assert len(names) == 2 * pm.factored_lens(ell)[1] + 7 + (ell >= 2)
    for what in names:
        a = pvm.tamper(what, proof, r, C_Zr, comm, gens, other)
        literal = pm.verify(Transcript(b"polyeval"), a[0], a[4], a[1], a[2], a[3])
        folded = pvm.verify_folded(Transcript(b"polyeval"), a[0], a[4], a[1], a[2], a[3])
        assert not literal and not folded, what


@pytest.mark.parametrize("lg", range(1, 8))
def test_b_hat_in_closed_form_is_the_dot_product(lg):
    rng = random.Random(lg)
    us = [rng.randrange(1, R_MOD) for _ in range(lg)]
    for r_right in ([rng.randrange(R_MOD) for _ in range(lg)], [0] * lg, [1] * lg, [i & 1 for i in range(lg)], [rng.randrange(R_MOD), 0, 1][:lg] + [rng.randrange(R_MOD)] * max(lg - 3, 0)):
        assert pvm.b_hat_closed(us, r_right) == pm.dot(pm.compute_s(us), pm.eq_evals(r_right))


def test_library_exports_the_one_call_verifier_and_checks_its_arguments(sbn):
    """no device here: the symbols exist, and a call without a context is SBN_EINVAL with the transcript as it was, never a crash"""
    L = sbn.lib()
    for name in ("sbn_g1_decompress", "sbn_bases_from_compressed", "sbn_polyeval_verify", "sbn_joint_opening_verify"):
        assert hasattr(L, name)
    tr = sbn.Transcript(b"polyeval")
    before = tr.state()
    buf = lambda k: (C.c_uint8 * k)()                      # noqa: E731
    acc = C.c_int(7)
    fake = C.c_void_p(0)
    assert L.sbn_polyeval_verify(None, fake, fake, buf(64), C.c_size_t(2), None, buf(32), buf(192), tr.h, C.byref(acc)) == -1      # SBN_EINVAL
    assert L.sbn_joint_opening_verify(None, fake, fake, buf(64), C.c_size_t(2), b"e", C.c_size_t(1), b"c", C.c_size_t(1), b"j", C.c_size_t(1), buf(32), C.c_size_t(1),
                                      buf(192), tr.h, buf(32), C.byref(acc)) == -1
    assert L.sbn_g1_decompress(None, buf(32), C.c_size_t(1), buf(64), buf(1)) == -1
    out = C.c_void_p(0)
    assert L.sbn_bases_from_compressed(None, buf(32), C.c_size_t(1), C.byref(out), None) == -1 and not out.value
    assert tr.state() == before
