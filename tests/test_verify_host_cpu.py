"""CPU: the verifiers' host arithmetic (csrc/verify_host.hpp: the point and scalar helpers, OpeningShape, polyeval_host_eq, joint_reduce,
polyeval_verify_script, polyeval_verify_scalars) against tests/polyeval_verify_model.py, tests/polyeval_model.py, tests/transcript_model.py and plain
integers.  tests/verify_host_check.cpp includes the header alone and is built with g++ under ASan + UBSan as a stand-alone program, fed one case per
line and compared line by line; where a transcript is involved its whole 203-byte state is compared."""
import os
import random
import subprocess

import pytest

import polyeval_model as pm
import polyeval_verify_model as pvm
import transcript_model as tm
from conftest import ROOT

R = tm.R_MOD
Q = 21888242871839275222246405745257275088696311157297823662689037894645226208583      # BN254's base field


@pytest.fixture(scope="module")
def check(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("verify_host") / "verify_host_check")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        os.path.join(ROOT, "tests", "verify_host_check.cpp"), "-o", exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr

    def run(cases):
        """cases: [[word, ...]] (bytes go as hex, integers as decimal counts) -> the words of each case's result line"""
        def word(w):
            return str(w) if isinstance(w, (int, str)) else (bytes(w).hex() or "-")
        text = "".join(" ".join(word(w) for w in case) + "\n" for case in cases)
        r = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
        lines = r.stdout.splitlines()
        assert lines[-1] == "VERIFY HOST CHECK DONE" and len(lines) == len(cases) + 1
        return [ln.split() for ln in lines[:-1]]
    return run


def le32(x):
    return int(x).to_bytes(32, "little")


def xy(x, y):
    return le32(x) + le32(y)


def hx(b):
    return bytes(b).hex() or "-"


def sqrt_q(a):
    """a square root mod q (q = 3 mod 4), or None"""
    y = pow(a, (Q + 1) // 4, Q)
    return y if y * y % Q == a % Q else None


def test_g1_xy_valid(check):
    rng = random.Random(11)
    assert sqrt_q(2) not in (None, 1, Q - 1)            # x = q - 1 has points (y^2 = 2); (q - 1, 1) is not one of them
    x5 = next(x for x in range(5, 50) if sqrt_q(x ** 3 + 3) is not None)
    cases = [
        ((0, 0), 1),                                    # the identity
        ((1, 2), 1),                                    # the generator
        ((x5, sqrt_q(x5 ** 3 + 3)), 1),
        ((Q, 2), 0), ((1, Q), 0),                       # x = q, y = q: not canonical (q = 0 would otherwise read as (0, 2) / (1, 0))
        ((1, Q + 2), 0),                                # y = 2 + q: the same residue, not canonical
        ((Q - 1, 1), 0),                                # canonical, off the curve
        ((Q - 1, sqrt_q(2)), 1),                        # canonical at the largest x, on the curve
        ((1, Q - 2), 1),                                # the generator with y negated
        ((1 | 1 << 255, 2), 0), ((1, 2 | 1 << 255), 0),      # bit 255 set in a coordinate
        ((1, 3), 0), ((0, 1), 0), ((1, 0), 0),
    ]
    for _ in range(20):                                 # random pairs: on the curve only by the equation
        x, y = rng.randrange(Q), rng.randrange(Q)
        cases.append(((x, y), int(y * y % Q == (x ** 3 + 3) % Q)))
    got = check([["valid", xy(*p)] for p, _ in cases])
    for (p, want), (g,) in zip(cases, got):
        assert g == str(want), p


def test_compressed_normalise(check):
    rng = random.Random(12)
    flag, low = 1 << 254, (1 << 254) - 1
    garbage = rng.randrange(1, low + 1)
    ordinary = [1, Q - 1, 1 | 1 << 255, rng.randrange(Q), rng.randrange(Q) | 1 << 255, 0]
    cases = [(flag, flag), (flag | garbage, flag), (flag | low, flag), (flag | 1 << 255, flag), (flag | 1 << 255 | garbage, flag)] + [(v, v) for v in ordinary]
    got = check([["norm", le32(a)] for a, _ in cases])
    for (a, want), (g,) in zip(cases, got):
        assert g == le32(want).hex(), hex(a)


def test_fr_neg_bytes(check):
    rng = random.Random(13)
    vals = [0, 1, R - 1, 2, (R - 1) // 2, (R + 1) // 2] + [rng.randrange(R) for _ in range(50)]
    got = check([["frneg", le32(v)] for v in vals])
    for v, (g,) in zip(vals, got):
        assert g == le32(-v % R).hex(), v


def test_g1_neg_bytes_and_identity(check):
    rng = random.Random(14)
    pts = [(0, 0), (5, 1), (5, Q - 1), (1, 2), (1, Q - 2), (7, 0), (0, 3), (Q - 1, (Q - 1) // 2), (Q - 1, (Q + 1) // 2)] + [(rng.randrange(Q), rng.randrange(1, Q)) for _ in range(30)]
    got = check([["g1neg", xy(*p)] for p in pts])
    for (x, y), (g, ident) in zip(pts, got):
        assert g == xy(x, -y % Q).hex(), (x, y)          # y = 0 (the identity's too) stays 0
        assert ident == str(int(x == 0 and y == 0))


def test_fq_to_dev_mont(check):
    rng = random.Random(15)
    vals = [0, 1, Q - 1, 2, 32, (Q - 1) // 2] + [rng.randrange(Q) for _ in range(50)]
    got = check([["devmont", le32(v)] for v in vals])
    for v, (g,) in zip(vals, got):
        assert g == le32(v * pow(2, 261, Q) % Q).hex(), v


@pytest.mark.parametrize("ell", [1, 2, 3, 40])
def test_opening_shape(check, ell):
    ml, mr = pm.factored_lens(ell)
    (got,) = check([["shape", ell]])
    assert [int(w) for w in got] == [ell, ml, mr, 1 << ml, 1 << mr, mr, 2 * mr + 2]
    assert ml + mr == ell and mr - ml in (0, 1)


@pytest.mark.parametrize("m", range(5))
def test_polyeval_host_eq(check, m):
    rng = random.Random(16 + m)
    pool = [0, 1, R - 1]
    points = [[v] * m for v in pool] + [[rng.choice(pool + [rng.randrange(R)]) for _ in range(m)] for _ in range(12)] + [[rng.randrange(R) for _ in range(m)]]
    got = check([["eq", m, b"".join(le32(v) for v in r)] for r in points])
    for r, (g,) in zip(points, got):
        want = pm.eq_evals(r)
        assert len(want) == 1 << m
        assert g == b"".join(le32(v) for v in want).hex(), r


@pytest.mark.parametrize("ell_r", [0, 3])
@pytest.mark.parametrize("count", [1, 2, 8])
def test_joint_reduce(check, count, ell_r):
    rng = random.Random(100 * count + ell_r)
    labels = (b"evals_ops_val", b"challenge_combine_n_to_one", b"joint_claim_eval")
    lc = count.bit_length() - 1
    for evals in ([rng.randrange(R) for _ in range(count)], [R - 1] * count, [0] * count):
        r = [rng.randrange(R) for _ in range(ell_r)]
        t = tm.Transcript(b"joint")
        for e in evals:                                  # sparse_mlpoly_full.rs:384-397, as polyeval_model.prove_single has it
            t.append_scalar(labels[0], e)
        before = t.state()
        ch = [t.challenge_scalar(labels[1]) for _ in range(lc)]
        if lc == 0:
            assert t.state() == before                   # no challenge is drawn for a single eval
        pe = list(evals)
        for i in range(lc - 1, -1, -1):
            pe = [(pe[2 * k] + ch[i] * (pe[2 * k + 1] - pe[2 * k])) % R for k in range(len(pe) // 2)]
        t.append_scalar(labels[2], pe[0])
        (got,) = check([["joint", b"joint", b"".join(le32(e) for e in evals), lc, *labels, b"".join(le32(v) for v in r), ell_r]])
        assert got == [hx(b"".join(le32(v) for v in ch + r)), le32(pe[0]).hex(), t.state().hex()]
        if lc == 0:
            assert pe[0] == evals[0]


@pytest.fixture(scope="module")
def openings(ol):
    """honest model proofs with lg = 1 .. 5 bullet rounds (ell = 2 lg - 1: ml = lg - 1, mr = lg), blinds on the even ones"""
    out = {}
    for lg in range(1, 6):
        ell = 2 * lg - 1
        rng = random.Random(600 + lg)
        ml, mr = pm.factored_lens(ell)
        assert mr == lg
        n = 1 << mr
        gens = pm.split_gens(ol.gens_new(n + 1, b"gens_verify_host_test")[0], n)
        Z = [rng.randrange(R) for _ in range(1 << ell)]
        r = [rng.randrange(R) for _ in range(ell)]
        blinds = [rng.randrange(R) for _ in range(1 << ml)] if lg % 2 == 0 else None
        blind_Zr = rng.randrange(R) if lg % 2 == 0 else None
        rnd = [rng.randrange(R) for _ in range(3 + 2 * mr)]
        proof, C_Zr, _ = pm.prove(tm.Transcript(b"polyeval"), gens, Z, blinds, r, pm.dot(Z, pm.eq_evals(r)), blind_Zr, rnd)
        comm = pm.commit_poly(gens, Z, blinds, ell)
        assert pvm.verify_folded(tm.Transcript(b"polyeval"), proof, gens, r, C_Zr, comm)
        out[lg] = (gens, r, proof, C_Zr, pm.msm(pm.eq_evals(r[:ml]), comm))
    return out


@pytest.mark.parametrize("lg", range(1, 6))
def test_opening_script_and_scalars(check, ol, openings, lg):
    gens, r, proof, Cy, Cx = openings[lg]
    r_right = r[len(r) - lg:]
    # the model: the protocol line of PolyEvalProof::verify, then folded_terms; the challenges from a replay of the same lines
    t = tm.Transcript(b"polyeval")
    t.append_message(b"protocol-name", b"polynomial evaluation proof")
    replay = t.clone()
    scalars, points = pvm.folded_terms(t, proof, gens, r_right, Cx, Cy)
    replay.append_message(b"protocol-name", b"dot product proof (log)")
    pm.append_point(replay, b"Cx", Cx); pm.append_point(replay, b"Cy", Cy)
    for s in pm.eq_evals(r_right):
        replay.append_scalar(b"a", s)
    rq = replay.challenge_scalar(b"r")
    us = []
    for i in range(lg):
        pm.append_point(replay, b"L", proof["L"][i]); pm.append_point(replay, b"R", proof["R"][i])
        us.append(replay.challenge_scalar(b"u"))
    pm.append_point(replay, b"delta", proof["delta"]); pm.append_point(replay, b"beta", proof["beta"])
    cc = replay.challenge_scalar(b"c")
    assert replay.state() == t.state()
    a_hat = pvm.b_hat_closed(us, r_right)
    z1, z2 = proof["z1"], proof["z2"]
    s_vec = pm.compute_s(us)
    assert len(scalars) == 2 * lg + 4 + (1 << lg) + 2 and scalars[2 * lg + 1] == a_hat
    assert scalars[2 * lg + 4:2 * lg + 4 + (1 << lg)] == [-z1 * s % R for s in s_vec]      # the row the device builds from nz1, u and u^-1

    pb = pm.proof_bytes(proof)
    vec = lambda v: b"".join(le32(x) for x in v)         # noqa: E731
    (got,) = check([["opening", b"polyeval", Cx + Cy, vec(pm.eq_evals(r_right)), 1 << lg, pb[:32 * (2 * lg + 2)], lg, vec(r_right), le32(z1), le32(z2)]])
    want = ["1", le32(rq).hex(), le32(cc).hex(), vec(us).hex(), vec(pow(u, -1, R) for u in us).hex(), le32(a_hat).hex(), le32(-z1 % R).hex(), le32(-z2 % R).hex(),
            le32(scalars[-2]).hex(), vec(scalars[:2 * lg + 4]).hex(), t.state().hex()]
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, i
    assert scalars[-2] == -z1 * a_hat * rq % R and scalars[-1] == -z2 % R
