"""PolyEvalProof in plain Python: a literal restatement of the reference's prover AND verifier, the checker of sbn_polyeval_prove.

    prove:  PolyEvalProof::prove (hyrax.rs:65-116) -> DotProductProofLog::prove (nizk/mod.rs:439-522) -> BulletReductionProof::prove
            (nizk/bullet.rs:24-126), folding the generators every round exactly as bullet.rs:85-89 does
    verify: PolyEvalProof::verify (hyrax.rs:118-137) -> DotProductProofLog::verify (nizk/mod.rs:525-567) -> BulletReductionProof::verify
            (nizk/bullet.rs:130-173) with compute_s (bullet.rs:183-200)
    prove_single: the n-to-1 reduction in front of the opening (sparse_mlpoly_full.rs:374-410), labels as parameters

There is no Rust toolchain where this suite runs, so no vector produced by the reference itself exists.  What pins these functions to the
reference is that they restate it line by line on top of transcript_model.py (Merlin, written from the public specification) and the C
oracle's group operations, and that the verifier's relations hold for what the prover makes — the same footing as orc_bullet_prove.
Scalars are Python integers mod r; points are 64-byte canonical affine x || y (all-zero = infinity), compressed with the oracle.
"""
import oracle_lib as ol
from transcript_model import R_MOD, Transcript  # noqa: F401

INF = bytes(64)


def sb(x):
    return int(x % R_MOD).to_bytes(32, "little")


def ib(b):
    return int.from_bytes(b, "little")


def factored_lens(ell):
    return ell // 2, ell - ell // 2                        # hyrax.rs:371-373


def eq_evals(r):
    """EqPolynomial::evals (hyrax.rs:355-369)"""
    ev = [1] * (1 << len(r))
    size = 1
    for j in range(len(r)):
        size *= 2
        for i in range(size - 1, -1, -2):
            s = ev[i // 2]
            ev[i] = s * r[j] % R_MOD
            ev[i - 1] = (s - ev[i]) % R_MOD
    return ev


def mul(p, k):
    return ol.g1_mul(p, sb(k))


def msm(scalars, points):
    """vartime_multiscalar_mul (group.rs:143-158)"""
    if not scalars:
        return INF
    return ol.msm_pippenger(b"".join(sb(s) for s in scalars), b"".join(points), 4)


def append_point(tr, label, p):
    tr.append_message(label, ol.g1_compress(p))            # transcript.rs:102-108


def dot(a, b):
    return sum(x * y for x, y in zip(a, b)) % R_MOD


def split_gens(gens_xy, n):
    """sbn_gens_new(n + 1) -> (G[0..n), Q_base = gens_1.G[0], h)   (DotProductProofGens::new, nizk/mod.rs:412-415)"""
    pts = [gens_xy[64 * i:64 * i + 64] for i in range(n + 2)]
    return pts[:n], pts[n], pts[n + 1]


def bullet_prove(tr, Q, G, H, a, b, blind, blinds_vec):
    """nizk/bullet.rs:24-126 -> (L_vec, R_vec, a_hat, b_hat, g_hat, rhat_Gamma); Gamma (bullet.rs:57-59) is unused by every caller and left out"""
    n = len(G)
    G, a, b = list(G), list(a), list(b)
    Lv, Rv = [], []
    blind_G = blind
    for i in range(n.bit_length() - 1):
        n //= 2
        aL, aR, bL, bR, GL, GR = a[:n], a[n:], b[:n], b[n:], G[:n], G[n:]
        cL, cR = dot(aL, bR), dot(aR, bL)
        blL, blR = blinds_vec[i]
        L = ol.g1_add(ol.g1_add(msm(aL, GR), mul(Q, cL)), mul(H, blL))
        R = ol.g1_add(ol.g1_add(msm(aR, GL), mul(Q, cR)), mul(H, blR))
        append_point(tr, b"L", L); append_point(tr, b"R", R)
        u = tr.challenge_scalar(b"u")
        ui = pow(u, -1, R_MOD)
        G = [ol.g1_add(mul(gl, ui), mul(gr, u)) for gl, gr in zip(GL, GR)]          # bullet.rs:85-89
        a = [(u * x + ui * y) % R_MOD for x, y in zip(aL, aR)]
        b = [(ui * x + u * y) % R_MOD for x, y in zip(bL, bR)]
        blind_G = (u * u * blL + blind_G + ui * ui * blR) % R_MOD
        Lv.append(L); Rv.append(R)
    return Lv, Rv, a[0], b[0], G[0], blind_G


def dotproduct_prove(tr, gens, rnd, x_vec, blind_x, a_vec, y, blind_y):
    """nizk/mod.rs:439-522; rnd = [d, r_delta, r_beta, v1[0], v2[0], v1[1], ...] -> (proof dict, Cx, Cy)"""
    G, Qb, H = gens
    tr.append_message(b"protocol-name", b"dot product proof (log)")
    n = len(x_vec)
    lg = n.bit_length() - 1
    d, r_delta, r_beta = rnd[0], rnd[1], rnd[2]
    blinds_vec = [(rnd[3 + 2 * i], rnd[4 + 2 * i]) for i in range(lg)]
    Cx = ol.g1_add(msm(x_vec, G), mul(H, blind_x))
    append_point(tr, b"Cx", Cx)
    Cy = ol.g1_add(mul(Qb, y), mul(H, blind_y))
    append_point(tr, b"Cy", Cy)
    for s in a_vec:
        tr.append_scalar(b"a", s)
    r = tr.challenge_scalar(b"r")
    Q = mul(Qb, r)                                         # gens_1.scale(r).G[0]
    blind_Gamma = (blind_x + r * blind_y) % R_MOD
    Lv, Rv, x_hat, a_hat, g_hat, rhat = bullet_prove(tr, Q, G, H, x_vec, a_vec, blind_Gamma, blinds_vec)
    y_hat = x_hat * a_hat % R_MOD
    delta = ol.g1_add(mul(g_hat, d), mul(H, r_delta))
    append_point(tr, b"delta", delta)
    beta = ol.g1_add(mul(Q, d), mul(H, r_beta))
    append_point(tr, b"beta", beta)
    c = tr.challenge_scalar(b"c")
    z1 = (d + c * y_hat) % R_MOD
    z2 = (a_hat * (c * rhat + r_beta) + r_delta) % R_MOD
    return dict(L=Lv, R=Rv, delta=delta, beta=beta, z1=z1, z2=z2), Cx, Cy


def prove(tr, gens, Z, blinds, r, Zr, blind_Zr, rnd):
    """hyrax.rs:65-116; Z: 2^ell integers, blinds: L_size integers or None -> (proof dict, C_Zr_prime = Cy, Cx)"""
    tr.append_message(b"protocol-name", b"polynomial evaluation proof")
    ml, mr = factored_lens(len(r))
    Ls, Rs = 1 << ml, 1 << mr
    assert len(Z) == Ls * Rs
    blinds = [0] * Ls if blinds is None else blinds
    L, R = eq_evals(r[:ml]), eq_evals(r[ml:])
    LZ = [sum(L[i] * Z[i * Rs + j] for i in range(Ls)) % R_MOD for j in range(Rs)]
    LZ_blind = dot(blinds, L)
    proof, Cx, Cy = dotproduct_prove(tr, gens, rnd, LZ, LZ_blind, R, Zr, blind_Zr or 0)
    return proof, Cy, Cx


def proof_bytes(p):
    """the layout of sbn_polyeval_prove's out_proof"""
    return (b"".join(ol.g1_compress(x) for x in p["L"]) + b"".join(ol.g1_compress(x) for x in p["R"]) + ol.g1_compress(p["delta"])
            + ol.g1_compress(p["beta"]) + sb(p["z1"]) + sb(p["z2"]))


def proof_from_bytes(b):
    """-> proof dict, or None when a point does not decompress (the reference's deserialisation fails)"""
    lg = (len(b) - 128) // 64
    pts = [ol.g1_decompress(b[32 * i:32 * i + 32]) for i in range(2 * lg + 2)]
    if any(p is None for p in pts):
        return None
    return dict(L=pts[:lg], R=pts[lg:2 * lg], delta=pts[2 * lg], beta=pts[2 * lg + 1], z1=ib(b[64 * lg + 64:64 * lg + 96]), z2=ib(b[64 * lg + 96:]))


def compute_s(us):
    """bullet.rs:183-200"""
    lg = len(us)
    inv = [pow(u, -1, R_MOD) for u in us]
    s = [1] * (1 << lg)
    for i in range(1 << lg):
        for j in range(lg):
            s[i] = s[i] * (us[lg - 1 - j] if (i >> j) & 1 else inv[lg - 1 - j]) % R_MOD
    return s


def bullet_verify(tr, proof, n, b_vec, Gamma, G):
    """bullet.rs:130-173 -> (g_hat, Gamma_hat, b_hat)"""
    lg = n.bit_length() - 1
    assert len(proof["L"]) == lg and len(proof["R"]) == lg
    us = []
    for i in range(lg):
        append_point(tr, b"L", proof["L"][i]); append_point(tr, b"R", proof["R"][i])
        us.append(tr.challenge_scalar(b"u"))
    s = compute_s(us)
    g_hat = msm(s, G)
    b_hat = dot(s, b_vec)
    u_sq = [u * u % R_MOD for u in us]
    u_sq_inv = [pow(x, -1, R_MOD) for x in u_sq]
    Gamma_hat = ol.g1_add(ol.g1_add(msm(u_sq, proof["L"]), Gamma), msm(u_sq_inv, proof["R"]))
    return g_hat, Gamma_hat, b_hat


def dotproduct_verify(tr, proof, gens, a, Cx, Cy):
    """nizk/mod.rs:525-567 -> bool"""
    G, Qb, H = gens
    n = len(a)
    tr.append_message(b"protocol-name", b"dot product proof (log)")
    append_point(tr, b"Cx", Cx); append_point(tr, b"Cy", Cy)
    for s in a:
        tr.append_scalar(b"a", s)
    r = tr.challenge_scalar(b"r")
    Q = mul(Qb, r)
    Gamma = ol.g1_add(Cx, mul(Cy, r))
    g_hat, Gamma_hat, a_hat = bullet_verify(tr, proof, n, a, Gamma, G)
    append_point(tr, b"delta", proof["delta"]); append_point(tr, b"beta", proof["beta"])
    c = tr.challenge_scalar(b"c")
    lhs = ol.g1_add(mul(ol.g1_add(mul(Gamma_hat, c), proof["beta"]), a_hat), proof["delta"])
    rhs = ol.g1_add(mul(ol.g1_add(g_hat, mul(Q, a_hat)), proof["z1"]), mul(H, proof["z2"]))
    return lhs == rhs


def verify(tr, proof, gens, r, C_Zr, comm_C):
    """hyrax.rs:118-137; comm_C: the L_size row commitments of the polynomial (PolyCommitment.C)"""
    tr.append_message(b"protocol-name", b"polynomial evaluation proof")
    ml, _ = factored_lens(len(r))
    L, R = eq_evals(r[:ml]), eq_evals(r[ml:])
    C_LZ = msm(L, comm_C)
    return dotproduct_verify(tr, proof, gens, R, C_LZ, C_Zr)


def verify_plain(tr, proof, gens, r, Zr, comm_C):
    """hyrax.rs:139-151: C_Zr = Zr.commit(0, gens_1)"""
    return verify(tr, proof, gens, r, mul(gens[1], Zr), comm_C)


def commit_poly(gens, Z, blinds, ell):
    """DensePolynomial::commit (hyrax.rs:283-308): one row commitment per row of the L_size x R_size view"""
    G, _, H = gens
    ml, mr = factored_lens(ell)
    Rs = 1 << mr
    blinds = [0] * (1 << ml) if blinds is None else blinds
    return [ol.g1_add(msm(Z[i * Rs:(i + 1) * Rs], G), mul(H, blinds[i])) for i in range(1 << ml)]


def prove_single(tr, gens, Z, r, evals, rnd, labels=(b"evals_ops_val", b"challenge_combine_n_to_one", b"joint_claim_eval")):
    """DerefsEvalProof::prove_single (sparse_mlpoly_full.rs:374-410) and its two siblings (:986-1009, :1013-1035), which differ in the labels
    -> (challenges, joint_claim, proof dict, Cy, Cx)"""
    le, lch, lcl = labels
    lc = len(evals).bit_length() - 1
    assert len(Z) == 1 << (len(r) + lc)
    for e in evals:
        tr.append_scalar(le, e)
    ch = [tr.challenge_scalar(lch) for _ in range(lc)]
    pe = list(evals)
    for i in range(lc - 1, -1, -1):                        # bound_poly_var_bot (hyrax.rs:206-214)
        pe = [(pe[2 * k] + ch[i] * (pe[2 * k + 1] - pe[2 * k])) % R_MOD for k in range(len(pe) // 2)]
    claim = pe[0]
    tr.append_scalar(lcl, claim)
    proof, Cy, Cx = prove(tr, gens, Z, None, ch + list(r), claim, None, rnd)
    return ch, claim, proof, Cy, Cx
