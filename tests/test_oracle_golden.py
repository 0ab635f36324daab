"""CPU: the C oracle against the committed golden vectors, the reference's own unit-test relations and the
pure-Python model.  This is what "pins" the oracle (there are no reference fixtures for MSM bytes: parity unpinned
at byte level by the reference itself)."""
import hashlib

import pytest
from conftest import golden

H = bytes.fromhex


def test_field_kat(ol):
    g = golden("field_kat.json")
    for which, name in ((0, "fq"), (1, "fr")):
        for row in g[name]:
            a, b = H(row["a"]), H(row["b"])
            assert ol.fe_op("add", which, a, b) == H(row["add"])
            assert ol.fe_op("sub", which, a, b) == H(row["sub"])
            assert ol.fe_op("mul", which, a, b) == H(row["mul"])
            assert ol.fe_op("inv", which, a) == H(row["inv_a"])
    for row in g["fr_from_wide"]:
        assert ol.fr_from_wide(H(row["in"])) == H(row["out"])      # transcript.rs:56-67


def test_scalar_bytes_canonical(ol, pr):
    # scalar.rs:87-95 from_bytes rejects >= r ; scalar.rs:206-215 round trip
    assert ol.fe_is_canonical(1, (pr.R - 1).to_bytes(32, "little"))
    assert not ol.fe_is_canonical(1, pr.R.to_bytes(32, "little"))
    assert not ol.fe_is_canonical(1, b"\xff" * 32)
    assert not ol.fe_is_canonical(0, pr.P.to_bytes(32, "little"))


def test_g1_kat(ol, pr):
    g = golden("g1_kat.json")
    G = pr.point_to_xy(pr.G)
    for row in g["mul"]:
        out = ol.g1_mul(G, H(row["k"]))
        assert out == H(row["kG"])
        assert ol.g1_on_curve(out)
        assert ol.g1_compress(out) == H(row["compressed"])
        assert ol.g1_decompress(H(row["compressed"])) == out        # group.rs:323-329 round trip
    for row in g["add"]:
        assert ol.g1_add(H(row["p"]), H(row["q"])) == H(row["sum"]), row["note"]
    c = g["compressed"]
    assert ol.g1_compress(G) == H(c["generator"]) == bytes([1]) + bytes(31)   # G -> 01 00..00
    assert ol.g1_compress(bytes(64)) == H(c["infinity"]) == bytes(31) + b"\x40"
    assert ol.g1_compress(ol.g1_neg(G)) == H(c["neg_generator"])
    assert len(ol.g1_compress(G)) == 32                                          # kzg.rs:558-581 / group.rs:91-93


def test_msm_kat(ol):
    for case in golden("msm_kat.json")["cases"]:
        s = b"".join(H(x) for x in case["scalars"]); p = b"".join(H(x) for x in case["points"])
        assert ol.msm_naive(s, p) == H(case["expected"]), case["note"]
        assert ol.msm_pippenger(s, p, 1) == H(case["expected"]), case["note"]
        assert ol.msm_pippenger(s, p, 4) == H(case["expected"]), case["note"]


def test_window_heuristic(ol):
    # c = 3 if n < 32 else floor(ceil(log2 n) * 69 / 100) + 2 ; 8193 -> 11, 2^25 -> 19
    assert ol.window_bits(31) == 3
    assert ol.window_bits(8193) == 11
    assert ol.window_bits(1 << 25) == 19


def test_gens_kat(ol, pr):
    g = golden("gens_kat.json")
    for label, row in g.items():
        n = row["n"]
        xy, dl = ol.gens_new(n, label.encode())
        assert len(xy) == 64 * (n + 1)
        for i, (d, p) in enumerate(zip(row["first_dlogs"], row["first_points"])):
            assert dl[32 * i:32 * i + 32] == H(d)
            assert xy[64 * i:64 * i + 64] == H(p)
        assert dl[32 * n:] == H(row["h_dlog"])
        ones = sum(1 for i in range(n + 1) if dl[32 * i:32 * i + 32] == (1).to_bytes(32, "little"))
        assert ones == row["count_equal_to_G_incl_h"]
        assert sum(int.from_bytes(dl[32 * i:32 * i + 32], "little") for i in range(n + 1)) % pr.R == int.from_bytes(H(row["dlog_sum_mod_r"]), "little")
    # SURVEY App. A measured these on the reference's derivation: 5381 of 8194 and 695 of 1026 generators equal G
    assert g["gens_r1cs_eval"]["count_equal_to_G_incl_h"] == 5381
    assert g["gens_r1cs_sat"]["count_equal_to_G_incl_h"] == 695


def test_keccak(ol):
    for m in (b"", b"abc", bytes(range(200)), b"x" * 135, b"y" * 136, b"z" * 137):
        assert ol.sha3_256(m) == hashlib.sha3_256(m).digest()
        assert ol.shake256(m, 777) == hashlib.shake_256(m).digest(777)


def test_commit_kat(ol, pr):
    for case in golden("commit_kat.json")["cases"]:
        R, L = case["R"], case["L"]
        xy, _ = ol.gens_new(R, case["label"].encode())
        Z = pr.prng_scalars(L * R, case["seed"])
        if case["zero_row"] is not None:
            Z[R:2 * R] = [0] * R
            Z[2 * R:3 * R] = [Z[2 * R]] * R
        Zb = b"".join(pr.scalar_to_bytes(v) for v in Z)
        bl = b"".join(pr.scalar_to_bytes(v) for v in pr.prng_scalars(L, case["seed"] + 1)) if case["with_blinds"] else None
        out = ol.commit_rows(Zb, bl, L, R, xy[:64 * R], xy[64 * R:], 8)
        assert out == b"".join(H(x) for x in case["expected_rows"])
        if not case["with_blinds"] and case["zero_row"] is not None:
            assert out[64:128] == bytes(64)      # all-zero row commits to the identity
        # single-row entry point (commitments.rs:144-154)
        assert ol.commit(Zb[:32 * R], bl[:32] if bl else bytes(32), xy[:64 * R], xy[64 * R:]) == H(case["expected_rows"][0])


def test_sumcheck_kat(ol):
    g = golden("sumcheck_kat.json")
    for u in g["unipoly"]:
        ev = b"".join(H(x) for x in u["evals"])
        co = ol.unipoly_from_evals(ev)
        assert co == b"".join(H(x) for x in u["coeffs"]), u["note"]
        assert ol.unipoly_eval(co, H(u["at"])) == H(u["value"])
    for r in g["rounds"]:
        T, A, B, C = (b"".join(H(x) for x in r[k]) for k in "TABC")
        assert ol.sc_eval_cubic(A, B, C) == b"".join(H(x) for x in r["cubic"])
        assert ol.sc_eval_r1cs(T, A, B, C) == b"".join(H(x) for x in r["r1cs"])
        assert ol.sc_eval_quad(A, B) == b"".join(H(x) for x in r["quad"])
    for e in g["eq"]:
        assert ol.eq_evals(b"".join(H(x) for x in e["r"])) == b"".join(H(x) for x in e["evals"])
    for b in g["bind"]:
        assert ol.bind_top(b"".join(H(x) for x in b["Z"]), H(b["r"])) == b"".join(H(x) for x in b["out"])


def test_reference_sumcheck_roundtrip(ol, pr):
    """sumcheck.rs:818-861 restated: prove 2 rounds on A=[1,2,3,4], B=C=1 with an arbitrary challenge stream and check the
    verifier's relations (e0+e1 == claim each round, final claim == A0*B0*C0)."""
    from conftest import fr_bytes
    A, B, C = fr_bytes([1, 2, 3, 4]), fr_bytes([1, 1, 1, 1]), fr_bytes([1, 1, 1, 1])
    claim = 10
    for rnd in range(2):
        ev = ol.sc_eval_cubic(A, B, C)
        e0, e2, e3 = (int.from_bytes(ev[32 * i:32 * i + 32], "little") for i in range(3))
        e1 = (claim - e0) % pr.R
        co = ol.unipoly_from_evals(fr_bytes([e0, e1, e2, e3]))
        cs = [int.from_bytes(co[32 * i:32 * i + 32], "little") for i in range(4)]
        assert (cs[0] + sum(cs)) % pr.R == claim                      # verifier check: p(0)+p(1) == claim
        r = int.from_bytes(hashlib.sha3_256(co).digest(), "little") % pr.R
        rb = pr.scalar_to_bytes(r)
        A, B, C = ol.bind_top(A, rb), ol.bind_top(B, rb), ol.bind_top(C, rb)
        claim = int.from_bytes(ol.unipoly_eval(co, rb), "little")
    a0, b0, c0 = (int.from_bytes(x[:32], "little") for x in (A, B, C))
    assert a0 * b0 * c0 % pr.R == claim


def test_dense_poly_reference_tests(ol, pr):
    """hyrax.rs:435-453: Z=[1,2,3,4] evaluates to 1 at (0,0) and 4 at (1,1) (evaluate = <Z, eq(r)>)."""
    from conftest import fr_bytes
    Z = fr_bytes([1, 2, 3, 4])
    for r, want in (([0, 0], 1), ([1, 1], 4), ([0, 1], 2), ([1, 0], 3)):
        chi = ol.eq_evals(fr_bytes(r))
        assert int.from_bytes(ol.fr_dot(Z, chi), "little") == want


@pytest.mark.parametrize("n", [1, 5, 31, 32, 100, 300])
def test_pippenger_vs_naive_vs_python(ol, pr, n):
    from conftest import rand_scalars
    sc = rand_scalars(n, n)
    dl = rand_scalars(n, 1000 + n)
    pts = ol.g1_mul_gen_batch(dl, 8)
    want = ol.g1_mul(pr.point_to_xy(pr.G), ol.fr_dot(sc, dl))          # discrete-log identity
    assert ol.msm_pippenger(sc, pts, 3) == want
    if n <= 100:
        assert ol.msm_naive(sc, pts) == want
    if n <= 5:
        ks = [int.from_bytes(sc[32 * i:32 * i + 32], "little") for i in range(n)]
        ps = [pr.point_from_xy(pts[64 * i:64 * i + 64]) for i in range(n)]
        assert pr.point_to_xy(pr.msm(ks, ps)) == want


def test_oracle_bullet_reduction_verifier_relations(ol, pr):
    """The reference's own test for this function (nizk/bullet.rs:215-255: n = 8, gens label "test-gens", Q = generator) is a
    prove -> verify round trip; the relations its verifier (bullet.rs:155-170) and DotProductProofLog::verify rely on must hold
    for the oracle's restatement: g_hat = MSM(s, G), b_hat = <s, b>, sum u^2 L + Gamma + sum u^-2 R = a_hat g_hat + a_hat b_hat Q + rhat H.
    The group side is re-derived with the independent pure-Python model."""
    from conftest import rand_scalars
    n, lg = 8, 3
    pts, dl = ol.gens_new(n, b"test-gens")
    G_xy, H_xy = pts[:64 * n], pts[64 * n:]
    Q = (1, 2); Q_xy = pr.point_to_xy(Q)
    a, b = rand_scalars(n, 1), rand_scalars(n, 2)
    blind = rand_scalars(1, 3); blinds_vec = rand_scalars(2 * lg, 4); us = rand_scalars(lg, 5)
    o = ol.bullet_prove(G_xy, Q_xy, H_xy, a, b, blind, blinds_vec, us)
    R = pr.R
    sc = lambda bs, i: pr.scalar_from_bytes(bs[32 * i:32 * i + 32])
    u = [sc(us, i) for i in range(lg)]; ui = [pow(x, R - 2, R) for x in u]
    s = []
    for i in range(n):
        v = 1
        for j in range(lg):
            v = v * (u[lg - 1 - j] if (i >> j) & 1 else ui[lg - 1 - j]) % R
        s.append(v)
    G = [pr.point_from_xy(G_xy[64 * i:64 * i + 64]) for i in range(n)]
    H = pr.point_from_xy(H_xy)
    av = [sc(a, i) for i in range(n)]; bv = [sc(b, i) for i in range(n)]
    assert pr.point_to_xy(pr.msm(s, G)) == o["g_hat"]
    assert sum(x * y for x, y in zip(s, bv)) % R == pr.scalar_from_bytes(o["b_hat"])
    assert sum(pow(x, R - 2, R) * y for x, y in zip(s, av)) % R == pr.scalar_from_bytes(o["a_hat"])   # a folds with u on the left half (bullet.rs:94-98)
    Gamma = pr.add(pr.add(pr.msm(av, G), pr.mul(Q, sum(x * y for x, y in zip(av, bv)) % R)), pr.mul(H, sc(blind, 0)))
    assert pr.point_to_xy(Gamma) == o["Gamma"]
    lhs = Gamma
    for i in range(lg):
        lhs = pr.add(lhs, pr.mul(pr.point_from_xy(o["L"][64 * i:64 * i + 64]), u[i] * u[i] % R))
        lhs = pr.add(lhs, pr.mul(pr.point_from_xy(o["R"][64 * i:64 * i + 64]), ui[i] * ui[i] % R))
    ah, bh, rh = (pr.scalar_from_bytes(o[k]) for k in ("a_hat", "b_hat", "blind_hat"))
    rhs = pr.add(pr.add(pr.mul(pr.point_from_xy(o["g_hat"]), ah), pr.mul(Q, ah * bh % R)), pr.mul(H, rh))
    assert lhs == rhs


def test_oracle_bullet_vs_python_model(ol):
    """tests/golden/bullet_kat.json comes from tests/pyref.py (per-round generator folds written as the reference writes them,
    Python integers): the C oracle must reproduce every output."""
    H = bytes.fromhex
    for case in golden("bullet_kat.json")["cases"]:
        o = ol.bullet_prove(H(case["G"]), H(case["Q"]), H(case["H"]), H(case["a"]), H(case["b"]), H(case["blind"]), H(case["blinds_vec"]), H(case["us"]))
        for k in ("L", "R", "Gamma", "a_hat", "b_hat", "g_hat", "blind_hat"):
            assert o[k] == H(case[k]), (case["n"], k)


def test_prove_cubic_batched_loop_vs_round_functions(ol, pr):
    """orc_sc_prove_cubic_batched (sumcheck.rs:165-330, threaded) against the per-round oracle functions that the golden vectors pin
    (sc_eval_cubic, bind_top) and a big-integer check of the coeffs combination (sumcheck.rs:269-271) and of the verifier's relation
    p(0) + p(1) == claim (sumcheck.rs:35-86) driven with the combined values."""
    from conftest import fr_bytes, rand_scalars
    n, n_par, n_seq = 64, 3, 2
    Ap = [rand_scalars(n, 10 + i) for i in range(n_par)]; Bp = [rand_scalars(n, 20 + i) for i in range(n_par)]; Cp = rand_scalars(n, 30)
    As = [rand_scalars(n, 40 + i) for i in range(n_seq)]; Bs = [rand_scalars(n, 50 + i) for i in range(n_seq)]; Cs = [rand_scalars(n, 60 + i) for i in range(n_seq)]
    co = rand_scalars(n_par + n_seq, 70); ch = rand_scalars(6, 80)
    for threads in (1, 3):
        evals, comb, fin = ol.sc_prove_cubic_batched(Ap, Bp, Cp, As, Bs, Cs, co, ch, threads)
        hA, hB, hC, sA, sB, sC = list(Ap), list(Bp), Cp, list(As), list(Bs), list(Cs)
        ints = lambda b: [int.from_bytes(b[32 * i:32 * i + 32], "little") for i in range(len(b) // 32)]
        cs = ints(co)
        claim = None
        for j in range(6):
            want = [ol.sc_eval_cubic(hA[i], hB[i], hC) for i in range(n_par)] + [ol.sc_eval_cubic(sA[i], sB[i], sC[i]) for i in range(n_seq)]
            assert evals[j] == want, j
            cw = [sum(c * ints(e)[t] for c, e in zip(cs, want)) % pr.R for t in range(3)]
            assert comb[j] == fr_bytes(cw), j
            if claim is not None:                                   # the round polynomial through (e0, claim - e0, e2, e3) evaluates consistently
                poly = ol.unipoly_from_evals(fr_bytes([cw[0], (claim - cw[0]) % pr.R, cw[1], cw[2]]))
                pc = ints(poly)
                assert (pc[0] + sum(pc)) % pr.R == claim
            r = ch[32 * j:32 * j + 32]
            # next claim = p(r_j) where p interpolates the combined values with e1 = sum over the upper half of the cube (computed directly)
            upper = 0
            for i in range(n_par):
                h = len(hA[i]) // 64
                upper += cs[i] * sum(a * b * c for a, b, c in zip(ints(hA[i])[h:], ints(hB[i])[h:], ints(hC)[h:]))
            for i in range(n_seq):
                h = len(sA[i]) // 64
                upper += cs[n_par + i] * sum(a * b * c for a, b, c in zip(ints(sA[i])[h:], ints(sB[i])[h:], ints(sC[i])[h:]))
            poly = ol.unipoly_from_evals(fr_bytes([cw[0], upper % pr.R, cw[1], cw[2]]))
            claim = int.from_bytes(ol.unipoly_eval(poly, r), "little")
            hA = [ol.bind_top(x, r) for x in hA]; hB = [ol.bind_top(x, r) for x in hB]; hC = ol.bind_top(hC, r)
            sA = [ol.bind_top(x, r) for x in sA]; sB = [ol.bind_top(x, r) for x in sB]; sC = [ol.bind_top(x, r) for x in sC]
        assert fin == [x[:32] for x in hA] + [x[:32] for x in hB] + [hC[:32]] + [x[:32] for x in sA] + [x[:32] for x in sB] + [x[:32] for x in sC]
        # after the last round the claim is the combination of the final products (what the verifier checks, product_tree.rs:430-460)
        f = [int.from_bytes(x, "little") for x in fin]
        total = sum(cs[i] * f[i] * f[n_par + i] * f[2 * n_par] for i in range(n_par))
        o = 2 * n_par + 1
        total += sum(cs[n_par + i] * f[o + i] * f[o + n_seq + i] * f[o + 2 * n_seq + i] for i in range(n_seq))
        assert total % pr.R == claim
    # no par instances / no seq instances
    ev2, cb2, fin2 = ol.sc_prove_cubic_batched([], [], None, As, Bs, Cs, co[:64], ch[:64], 2)
    assert ev2[0] == [ol.sc_eval_cubic(As[i], Bs[i], Cs[i]) for i in range(n_seq)] and len(fin2) == 6
    ev3, cb3, fin3 = ol.sc_prove_cubic_batched(Ap, Bp, Cp, [], [], [], co[:96], ch[:32], 2)
    assert ev3[0] == [ol.sc_eval_cubic(Ap[i], Bp[i], Cp) for i in range(n_par)] and len(fin3) == 7


@pytest.mark.parametrize("kind", ["r1cs", "quad"])
def test_prove_r1cs_quad_loops_vs_round_functions(ol, pr, kind):
    """orc_sc_prove_r1cs / orc_sc_prove_quad (sumcheck.rs:502-555, 691-716, threaded) against the per-round oracle functions that the
    golden vectors pin (sc_eval_r1cs / sc_eval_quad, bind_top), and the verifier's relations in big integers: claim_0 = sum of the comb
    function over the cube, p(0) + p(1) == claim with p through (e0, claim - e0, e2[, e3]), next claim = p(r_j), and the final claim
    = the comb function of the finals"""
    from conftest import fr_bytes, rand_scalars
    n, rounds = 64, 6
    ntab = 4 if kind == "r1cs" else 2
    tabs = [rand_scalars(n, 110 + k) for k in range(ntab)]
    ch = rand_scalars(rounds, 120)
    ints = lambda b: [int.from_bytes(b[32 * i:32 * i + 32], "little") for i in range(len(b) // 32)]
    comb = (lambda t, a, b, c: t * (a * b - c)) if kind == "r1cs" else (lambda z, abc: z * abc)
    for threads in (1, 3):
        if kind == "r1cs":
            evals, fin = ol.sc_prove_r1cs(*tabs, ch, threads)
        else:
            evals, fin = ol.sc_prove_quad(*tabs, ch, threads)
        assert len(evals) == rounds and len(fin) == ntab
        host = list(tabs)
        claim = sum(comb(*v) for v in zip(*(ints(t) for t in host))) % pr.R
        for j in range(rounds):
            want = ol.sc_eval_r1cs(*host) if kind == "r1cs" else ol.sc_eval_quad(*host)
            assert evals[j] == want, j
            e = ints(evals[j])
            poly = ol.unipoly_from_evals(fr_bytes([e[0], (claim - e[0]) % pr.R] + e[1:]))
            pc = ints(poly)
            assert (pc[0] + sum(pc)) % pr.R == claim, j
            r = ch[32 * j:32 * j + 32]
            claim = int.from_bytes(ol.unipoly_eval(poly, r), "little")
            host = [ol.bind_top(t, r) for t in host]
        assert fin == [t[:32] for t in host]
        assert comb(*ints(b"".join(fin))) % pr.R == claim
    # fewer rounds than variables: the finals are entry 0 of the partly bound tables
    ev2, fin2 = ol.sc_prove_r1cs(*tabs, ch[:64], 2) if kind == "r1cs" else ol.sc_prove_quad(*tabs, ch[:64], 2)
    assert ev2 == evals[:2] and fin2 == [ol.bind_top(ol.bind_top(t, ch[:32]), ch[32:64])[:32] for t in tabs]
