"""CPU: the literal model of the two ZK sumchecks (tests/zk_sumcheck_model.py) proves and verifies, rejects a flipped byte in every proof
field, consumes the draws in the order sbn_zk_sumcheck_prove_* states, and the library exports both entry points with the header's arity.
The model is what tests/test_gpu_zk_sumcheck.py holds the device's bytes against."""
import ctypes as C
import os
import random
import re

import pytest

import zk_sumcheck_model as zm
from zk_sumcheck_model import R_MOD, Transcript

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KINDS = {"r1cs": (4, 4), "quad": (2, 3)}                    # tables, coefficients


def _gens(ol, n):
    g1 = zm.gens_1_of(ol.gens_new(1, b"gens_zk_test_pc")[0])
    gn = zm.split_gens(ol.gens_new(n, b"gens_zk_test_sc%d" % n)[0], n)
    assert g1[1] != gn[1]                                   # two different h, as in R1CSSumcheckGens::new
    return g1, gn


def _case(ol, kind, rounds, seed):
    nt, n = KINDS[kind]
    rng = random.Random(seed)
    g1, gn = _gens(ol, n)
    tabs = [[rng.randrange(R_MOD) for _ in range(1 << rounds)] for _ in range(nt)]
    if kind == "r1cs":
        claim = sum(t * (a * b - c) for t, a, b, c in zip(*tabs)) % R_MOD
    else:
        claim = zm.dot(*tabs)
    blind_claim = rng.randrange(R_MOD)
    rnd = [rng.randrange(R_MOD) for _ in range(rounds * (n + 4))]
    return g1, gn, tabs, claim, blind_claim, rnd


def _prove(kind, tr, rnd, claim, blind_claim, tabs, g1, gn):
    return (zm.prove_r1cs if kind == "r1cs" else zm.prove_quad)(tr, rnd, claim, blind_claim, *tabs, g1, gn)


@pytest.mark.parametrize("kind", ["r1cs", "quad"])
@pytest.mark.parametrize("rounds", [1, 2, 3, 4])
def test_model_prove_then_verify(ol, pr, kind, rounds):
    nt, n = KINDS[kind]
    g1, gn, tabs, claim, blind_claim, rnd = _case(ol, kind, rounds, 40 + rounds)
    tp = Transcript(b"zk sumcheck")
    proof, r, finals, blind_last = _prove(kind, tp, rnd, claim, blind_claim, tabs, g1, gn)
    assert blind_last == rnd[2 * rounds - 1]
    bound = [list(t) for t in tabs]
    for rj in r:
        bound = [pr.bind_top(t, rj) for t in bound]
    assert finals == [t[0] for t in bound]
    tv = Transcript(b"zk sumcheck")
    got = zm.verify(tv, proof, zm.commit_one(claim, blind_claim, g1), rounds, n - 1, g1, gn)
    assert got is not None
    comm_last, rv = got
    assert rv == r and tv.state() == tp.state()
    # what the caller checks next (r1csproof.rs): the last comm_eval commits to comb_func(finals) under blinds_evals[-1]
    ev = finals[0] * (finals[1] * finals[2] - finals[3]) % R_MOD if kind == "r1cs" else finals[0] * finals[1] % R_MOD
    assert comm_last == zm.commit_one(ev, blind_last, g1)
    back = zm.proof_from_bytes(zm.proof_bytes(proof), n)
    assert back == proof and len(zm.proof_bytes(proof)) == rounds * (6 + n) * 32


@pytest.mark.parametrize("kind", ["r1cs", "quad"])
def test_model_verify_rejects_a_flipped_byte_in_every_field(ol, kind):
    nt, n = KINDS[kind]
    rounds = 2
    g1, gn, tabs, claim, blind_claim, rnd = _case(ol, kind, rounds, 9)
    proof, _, _, _ = _prove(kind, Transcript(b"zk sumcheck"), rnd, claim, blind_claim, tabs, g1, gn)
    comm_claim = zm.commit_one(claim, blind_claim, g1)
    good = zm.proof_bytes(proof)
    assert zm.verify(Transcript(b"zk sumcheck"), zm.proof_from_bytes(good, n), comm_claim, rounds, n - 1, g1, gn) is not None
    stride = (6 + n) * 32
    for rnd_i in range(rounds):
        for field in range(6 + n):                          # comm_poly, comm_eval, delta, beta, z[n], z_delta, z_beta
            bad = bytearray(good)
            bad[rnd_i * stride + 32 * field] ^= 1
            p = zm.proof_from_bytes(bytes(bad), n)
            assert p is None or zm.verify(Transcript(b"zk sumcheck"), p, comm_claim, rounds, n - 1, g1, gn) is None, (rnd_i, field)
    gen = ol.g1_mul_gen_batch(zm.sb(1), 1)
    assert zm.verify(Transcript(b"zk sumcheck"), proof, ol.g1_add(comm_claim, gen), rounds, n - 1, g1, gn) is None


@pytest.mark.parametrize("kind", ["r1cs", "quad"])
def test_the_draws_are_consumed_in_the_stated_order(ol, kind):
    """blinds_poly[rounds], blinds_evals[rounds], then per round d_vec[n], r_delta, r_beta: every value of the proof that is linear in one
    draw moves when exactly that draw moves"""
    nt, n = KINDS[kind]
    rounds = 2
    g1, gn, tabs, claim, blind_claim, rnd = _case(ol, kind, rounds, 21)
    base, r0, _, bl0 = _prove(kind, Transcript(b"zk sumcheck"), rnd, claim, blind_claim, tabs, g1, gn)
    assert bl0 == rnd[2 * rounds - 1]
    # the algebra of round 0 from the stated positions
    d0 = rnd[2 * rounds:2 * rounds + n]; r_delta0, r_beta0 = rnd[2 * rounds + n], rnd[2 * rounds + n + 1]
    assert base["proofs"][0]["delta"] == zm.commit_vec(d0, r_delta0, gn)
    d1 = rnd[2 * rounds + n + 2:2 * rounds + 2 * n + 2]; r_delta1 = rnd[2 * rounds + 2 * n + 2]
    assert base["proofs"][1]["delta"] == zm.commit_vec(d1, r_delta1, gn)
    # a changed blinds_poly[0] moves comm_poly_0 and nothing before it in the transcript; the tape must be used up exactly
    alt = list(rnd); alt[0] = (alt[0] + 1) % R_MOD
    other, _, _, _ = _prove(kind, Transcript(b"zk sumcheck"), alt, claim, blind_claim, tabs, g1, gn)
    assert other["comm_polys"][0] == ol.g1_add(base["comm_polys"][0], gn[1])
    alt = list(rnd); alt[rounds] = (alt[rounds] + 1) % R_MOD                      # blinds_evals[0]
    other, r1, _, _ = _prove(kind, Transcript(b"zk sumcheck"), alt, claim, blind_claim, tabs, g1, gn)
    assert r1[0] == r0[0] and other["comm_polys"][0] == base["comm_polys"][0]
    assert other["comm_evals"][0] == ol.g1_add(base["comm_evals"][0], g1[1])
    with pytest.raises(AssertionError):
        _prove(kind, Transcript(b"zk sumcheck"), rnd + [1], claim, blind_claim, tabs, g1, gn)
    with pytest.raises(AssertionError):
        _prove(kind, Transcript(b"zk sumcheck"), rnd[:-1], claim, blind_claim, tabs, g1, gn)
    # r_beta of round 0 sits behind r_delta: moving it moves beta_0 by h1 and nothing absorbed before beta_0
    alt = list(rnd); alt[2 * rounds + n + 1] = (r_beta0 + 1) % R_MOD
    other, r1, _, _ = _prove(kind, Transcript(b"zk sumcheck"), alt, claim, blind_claim, tabs, g1, gn)
    assert other["proofs"][0]["beta"] == ol.g1_add(base["proofs"][0]["beta"], g1[1])
    assert other["proofs"][0]["delta"] == base["proofs"][0]["delta"] and r1[0] == r0[0]
    # ... and r_delta of round 1 moves delta_1 by gens_n's h and leaves beta_0 alone
    alt = list(rnd); alt[2 * rounds + 2 * n + 2] = (r_delta1 + 1) % R_MOD
    other, _, _, _ = _prove(kind, Transcript(b"zk sumcheck"), alt, claim, blind_claim, tabs, g1, gn)
    assert other["proofs"][1]["delta"] == ol.g1_add(base["proofs"][1]["delta"], gn[1])
    assert other["proofs"][0]["beta"] == base["proofs"][0]["beta"]


def _header_arity(name):
    with open(os.path.join(ROOT, "include", "sbn254.h")) as f:
        src = f.read()
    m = re.search(r"\bint\s+%s\s*\(([^;]*?)\)\s*;" % name, src, re.S)
    assert m, name + " is not declared in include/sbn254.h"
    return len([a for a in m.group(1).split(",") if a.strip()])


def test_library_exports_both_entry_points_with_the_headers_arity(sbn):
    """no device here: the symbols exist, binding.py declares them as the header does, and a call without a context is SBN_EINVAL"""
    L = sbn.lib()
    for name, arity in (("sbn_zk_sumcheck_prove_r1cs", 15), ("sbn_zk_sumcheck_prove_quad", 13)):
        assert hasattr(L, name) and name in sbn.EXPORTED_SYMBOLS
        assert _header_arity(name) == arity
        assert len(getattr(L, name).argtypes) == arity
    tr = sbn.Transcript(b"zk sumcheck")
    before = tr.state()
    buf = lambda k: (C.c_uint8 * k)()                      # noqa: E731
    fake = C.c_void_p(0)
    assert L.sbn_zk_sumcheck_prove_r1cs(None, fake, fake, fake, fake, fake, fake, buf(32), buf(32), buf(256), tr.h, buf(320), buf(32), buf(128), buf(32)) == -1
    assert L.sbn_zk_sumcheck_prove_quad(None, fake, fake, fake, fake, buf(32), buf(32), buf(224), tr.h, buf(288), buf(32), buf(64), buf(32)) == -1
    assert tr.state() == before
