"""R1CSProof in plain Python: a literal restatement of the reference's prover AND verifier and of the three Σ-protocols between its two
sumchecks — the checker of sbn_r1cs_proof_prove.

    knowledge_prove / _verify   KnowledgeProof::prove / ::verify   (nizk/mod.rs:34-59, :61-81)
    equality_prove / _verify    EqualityProof::prove / ::verify    (nizk/mod.rs:96-124, :126-149)
    product_prove / _verify     ProductProof::prove / ::verify     (nizk/mod.rs:167-227, :243-283)
    prove                       R1CSProof::prove                   (r1csproof.rs:241-459), rnd in the layout of include/sbn254.h
    verify                      R1CSProof::verify                  (r1csproof.rs:463-619), A, B, C(rx, ry) from r1cs_model.evaluate

Built on zk_sumcheck_model.py (the two ZK sumchecks), polyeval_model.py (the Hyrax opening), r1cs_model.py (the three matrix loops) and
transcript_model.py (Merlin), on the same footing as they are: no vector produced by the reference itself exists where this suite runs.
Scalars are Python integers mod r; points are 64-byte canonical affine x || y (all-zero = infinity).
gens = dict(pc=(G[0..R), Q_base, h), g1=(Q_base, h), g3=([3], h3), g4=([4], h4)): gens_sc.gens_1 IS gens_pc.gens.gens_1 (r1csproof.rs:177-182).
"""
import random

import oracle_lib as ol
import polyeval_model as pm
import r1cs_model as rm
import zk_sumcheck_model as zm
from transcript_model import R_MOD, Transcript  # noqa: F401

sb, ib, mul, commit_one, append_point = zm.sb, zm.ib, zm.mul, zm.commit_one, zm.append_point
FIELDS = ("comm_vars", "sc_proof_phase1", "claims_phase2", "pok_claims_phase2", "proof_eq_sc_phase1", "sc_proof_phase2", "comm_vars_at_ry",
          "proof_eval_vars_at_ry", "proof_eq_sc_phase2")


def log2(n):
    assert n >= 1 and n & (n - 1) == 0
    return n.bit_length() - 1


def sizes(num_cons, num_vars):
    """(scalars of rnd, bytes of the proof)"""
    nx, ell = log2(num_cons), log2(num_vars)
    ny, (ml, lg) = ell + 1, pm.factored_lens(ell)
    L = 1 << ml
    return L + 8 * nx + 7 * ny + 2 * lg + 17, 32 * (L + 10 * nx + 9 * ny + 20) + 64 * lg + 128


def field_spans(num_cons, num_vars):
    """name -> (first byte, end) of each of the nine fields of out_proof"""
    nx, ell = log2(num_cons), log2(num_vars)
    ny, (ml, lg) = ell + 1, pm.factored_lens(ell)
    lens = [32 << ml, 320 * nx, 128, 352, 64, 288 * ny, 32, 64 * lg + 128, 64]
    out, o = {}, 0
    for name, n in zip(FIELDS, lens):
        out[name] = (o, o + n)
        o += n
    return out


def make_gens(pc_xy, R, g3_xy, g4_xy):
    """the points of sbn_gens_new(R + 1), sbn_gens_new(3), sbn_gens_new(4) -> the gens dict"""
    G, Qb, h = pm.split_gens(pc_xy, R)
    return dict(pc=(G, Qb, h), g1=(Qb, h), g3=zm.split_gens(g3_xy, 3), g4=zm.split_gens(g4_xy, 4))


# ---- the Σ-protocols ------------------------------------------------------------------------------------------------------------

def knowledge_prove(tr, gens_1, t1, t2, x, r):
    """nizk/mod.rs:34-59 -> (proof dict, C)"""
    tr.append_message(b"protocol-name", b"knowledge proof")
    C = commit_one(x, r, gens_1)
    append_point(tr, b"C", C)
    alpha = commit_one(t1, t2, gens_1)
    append_point(tr, b"alpha", alpha)
    c = tr.challenge_scalar(b"c")
    return dict(alpha=alpha, z1=(x * c + t1) % R_MOD, z2=(r * c + t2) % R_MOD), C


def knowledge_verify(tr, gens_1, proof, C):
    tr.append_message(b"protocol-name", b"knowledge proof")
    append_point(tr, b"C", C)
    append_point(tr, b"alpha", proof["alpha"])
    c = tr.challenge_scalar(b"c")
    return commit_one(proof["z1"], proof["z2"], gens_1) == ol.g1_add(mul(C, c), proof["alpha"])


def equality_prove(tr, gens_1, r, v1, s1, v2, s2):
    """nizk/mod.rs:96-124 -> (proof dict, C1, C2)"""
    tr.append_message(b"protocol-name", b"equality proof")
    C1 = commit_one(v1, s1, gens_1)
    append_point(tr, b"C1", C1)
    C2 = commit_one(v2, s2, gens_1)
    append_point(tr, b"C2", C2)
    alpha = mul(gens_1[1], r)
    append_point(tr, b"alpha", alpha)
    c = tr.challenge_scalar(b"c")
    return dict(alpha=alpha, z=(c * (s1 - s2) + r) % R_MOD), C1, C2


def equality_verify(tr, gens_1, proof, C1, C2):
    tr.append_message(b"protocol-name", b"equality proof")
    append_point(tr, b"C1", C1)
    append_point(tr, b"C2", C2)
    append_point(tr, b"alpha", proof["alpha"])
    c = tr.challenge_scalar(b"c")
    C = ol.g1_add(C1, mul(C2, R_MOD - 1))
    return mul(gens_1[1], proof["z"]) == ol.g1_add(mul(C, c), proof["alpha"])


def product_prove(tr, gens_1, b, x, rX, y, rY, z, rZ):
    """nizk/mod.rs:167-227; b = [b1 .. b5] -> (proof dict, X, Y, Z)"""
    tr.append_message(b"protocol-name", b"product proof")
    b1, b2, b3, b4, b5 = b
    X = commit_one(x, rX, gens_1)
    append_point(tr, b"X", X)
    Y = commit_one(y, rY, gens_1)
    append_point(tr, b"Y", Y)
    Z = commit_one(z, rZ, gens_1)
    append_point(tr, b"Z", Z)
    alpha = commit_one(b1, b2, gens_1)
    append_point(tr, b"alpha", alpha)
    beta = commit_one(b3, b4, gens_1)
    append_point(tr, b"beta", beta)
    delta = commit_one(b3, b5, (X, gens_1[1]))             # MultiCommitGens::from_generators(vec![X], gens_n.h)
    append_point(tr, b"delta", delta)
    c = tr.challenge_scalar(b"c")
    zs = [(b1 + c * x) % R_MOD, (b2 + c * rX) % R_MOD, (b3 + c * y) % R_MOD, (b4 + c * rY) % R_MOD, (b5 + c * (rZ - rX * y)) % R_MOD]
    return dict(alpha=alpha, beta=beta, delta=delta, z=zs), X, Y, Z


def product_verify(tr, gens_1, proof, X, Y, Z):
    tr.append_message(b"protocol-name", b"product proof")
    for label, p in ((b"X", X), (b"Y", Y), (b"Z", Z), (b"alpha", proof["alpha"]), (b"beta", proof["beta"]), (b"delta", proof["delta"])):
        append_point(tr, label, p)
    z1, z2, z3, z4, z5 = proof["z"]
    c = tr.challenge_scalar(b"c")

    def check(P, Xp, gens, za, zb):                        # check_equality, nizk/mod.rs:229-240
        return ol.g1_add(P, mul(Xp, c)) == commit_one(za, zb, gens)
    return check(proof["alpha"], X, gens_1, z1, z2) and check(proof["beta"], Y, gens_1, z3, z4) and check(proof["delta"], Z, (X, gens_1[1]), z3, z5)


# ---- R1CSProof ------------------------------------------------------------------------------------------------------------------

def build_z(vars_, inputs):
    """r1csproof.rs:268-277"""
    z = list(vars_) + [1] + list(inputs)
    return z + [0] * (2 * len(vars_) - len(z))


def commit_witness(gens, vars_, blinds):
    """commit_poly, r1csproof.rs:210-237"""
    return pm.commit_poly(gens["pc"], vars_, blinds, log2(len(vars_)))


def prove(tr, num_cons, num_vars, mats, vars_, inputs, gens, rnd):
    """r1csproof.rs:241-459 -> (proof dict, rx, ry)"""
    assert len(vars_) == num_vars and len(inputs) < len(vars_)        # :253
    assert len(rnd) == sizes(num_cons, num_vars)[0]
    tape = zm.Tape(rnd)
    g1, ell = gens["g1"], log2(num_vars)
    tr.append_message(b"protocol-name", b"R1CS proof")
    for s in inputs:
        tr.append_scalar(b"input", s)
    blinds_vars = tape.take(1 << pm.factored_lens(ell)[0])
    comm_vars = commit_witness(gens, vars_, blinds_vars)
    tr.append_message(b"poly_commitment", b"poly_commitment_begin")
    for c in comm_vars:
        append_point(tr, b"poly_commitment_share", c)
    tr.append_message(b"poly_commitment", b"poly_commitment_end")
    z = build_z(vars_, inputs)
    nx, ny = log2(num_cons), log2(len(z))
    tau = [tr.challenge_scalar(b"challenge_tau") for _ in range(nx)]
    Az, Bz, Cz = rm.multiply_vec(num_cons, num_vars, mats, z)
    sc1, rx, claims1, blind_post1 = zm.prove_r1cs(tr, tape.take(8 * nx), 0, 0, rm.eq_evals(tau), Az, Bz, Cz, g1, gens["g4"])
    tau_c, Az_c, Bz_c, Cz_c = claims1
    Az_b, Bz_b, Cz_b, prod_b = tape.take(4)
    pok_Cz, comm_Cz = knowledge_prove(tr, g1, *tape.take(2), Cz_c, Cz_b)
    prod = Az_c * Bz_c % R_MOD
    proof_prod, comm_Az, comm_Bz, comm_prod = product_prove(tr, g1, tape.take(5), Az_c, Az_b, Bz_c, Bz_b, prod, prod_b)
    append_point(tr, b"comm_Az_claim", comm_Az)
    append_point(tr, b"comm_Bz_claim", comm_Bz)
    append_point(tr, b"comm_Cz_claim", comm_Cz)
    append_point(tr, b"comm_prod_Az_Bz_claims", comm_prod)
    blind_expected1 = tau_c * (prod_b - Cz_b) % R_MOD
    claim_post1 = (Az_c * Bz_c - Cz_c) * tau_c % R_MOD
    eq1, _, _ = equality_prove(tr, g1, tape.take(1)[0], claim_post1, blind_expected1, claim_post1, blind_post1)
    rA, rB, rC = (tr.challenge_scalar(l) for l in (b"challenge_Az", b"challenge_Bz", b"challenge_Cz"))
    claim2 = (rA * Az_c + rB * Bz_c + rC * Cz_c) % R_MOD
    blind2 = (rA * Az_b + rB * Bz_b + rC * Cz_b) % R_MOD
    abc = rm.eval_table(num_cons, num_vars, mats, rx, rA, rB, rC)
    sc2, ry, claims2, blind_post2 = zm.prove_quad(tr, tape.take(7 * ny), claim2, blind2, z, abc, g1, gens["g3"])
    eval_vars = zm.dot(vars_, rm.eq_evals(ry[1:]))
    blind_eval = tape.take(1)[0]
    opening, comm_vars_at_ry, _ = pm.prove(tr, gens["pc"], vars_, blinds_vars, ry[1:], eval_vars, blind_eval, tape.take(3 + 2 * pm.factored_lens(ell)[1]))
    blind_expected2 = claims2[1] * ((1 - ry[0]) * blind_eval % R_MOD) % R_MOD
    claim_post2 = claims2[0] * claims2[1] % R_MOD
    eq2, _, _ = equality_prove(tr, g1, tape.take(1)[0], claim_post2, blind_expected2, claim_post2, blind_post2)
    assert tape.pos == len(rnd)
    proof = dict(comm_vars=comm_vars, sc_proof_phase1=sc1, claims_phase2=(comm_Az, comm_Bz, comm_Cz, comm_prod), pok_claims_phase2=(pok_Cz, proof_prod),
                 proof_eq_sc_phase1=eq1, sc_proof_phase2=sc2, comm_vars_at_ry=comm_vars_at_ry, proof_eval_vars_at_ry=opening, proof_eq_sc_phase2=eq2)
    return proof, rx, ry


def verify(tr, proof, num_vars, num_cons, inputs, evals, gens):
    """r1csproof.rs:463-619; evals = (A, B, C)(rx, ry), or a function of (rx, ry) that gives them -> (rx, ry) or None"""
    g1 = gens["g1"]
    tr.append_message(b"protocol-name", b"R1CS proof")
    for s in inputs:
        tr.append_scalar(b"input", s)
    tr.append_message(b"poly_commitment", b"poly_commitment_begin")
    for c in proof["comm_vars"]:
        append_point(tr, b"poly_commitment_share", c)
    tr.append_message(b"poly_commitment", b"poly_commitment_end")
    nx, ny = log2(num_cons), log2(2 * num_vars)
    tau = [tr.challenge_scalar(b"challenge_tau") for _ in range(nx)]
    got = zm.verify(tr, proof["sc_proof_phase1"], commit_one(0, 0, g1), nx, 3, g1, gens["g4"])
    if got is None:
        return None
    comm_claim_post1, rx = got
    comm_Az, comm_Bz, comm_Cz, comm_prod = proof["claims_phase2"]
    pok_Cz, proof_prod = proof["pok_claims_phase2"]
    if not knowledge_verify(tr, g1, pok_Cz, comm_Cz):
        return None
    if not product_verify(tr, g1, proof_prod, comm_Az, comm_Bz, comm_prod):
        return None
    append_point(tr, b"comm_Az_claim", comm_Az)
    append_point(tr, b"comm_Bz_claim", comm_Bz)
    append_point(tr, b"comm_Cz_claim", comm_Cz)
    append_point(tr, b"comm_prod_Az_Bz_claims", comm_prod)
    taus_bound_rx = 1
    for r_i, t_i in zip(rx, tau):
        taus_bound_rx = taus_bound_rx * (r_i * t_i + (1 - r_i) * (1 - t_i)) % R_MOD
    expected1 = mul(ol.g1_add(comm_prod, mul(comm_Cz, R_MOD - 1)), taus_bound_rx)
    if not equality_verify(tr, g1, proof["proof_eq_sc_phase1"], expected1, comm_claim_post1):
        return None
    rA, rB, rC = (tr.challenge_scalar(l) for l in (b"challenge_Az", b"challenge_Bz", b"challenge_Cz"))
    comm_claim2 = ol.g1_add(ol.g1_add(mul(comm_Az, rA), mul(comm_Bz, rB)), mul(comm_Cz, rC))
    got = zm.verify(tr, proof["sc_proof_phase2"], comm_claim2, ny, 2, g1, gens["g3"])
    if got is None:
        return None
    comm_claim_post2, ry = got
    if not pm.verify(tr, proof["proof_eval_vars_at_ry"], gens["pc"], ry[1:], proof["comm_vars_at_ry"], proof["comm_vars"]):
        return None
    chi = rm.eq_evals(ry[1:])
    poly_input_eval = (chi[0] + sum(v * chi[i + 1] for i, v in enumerate(inputs))) % R_MOD        # :580-594
    comm_eval_Z = ol.g1_add(mul(proof["comm_vars_at_ry"], 1 - ry[0]), mul(commit_one(poly_input_eval, 0, g1), ry[0]))
    eA, eB, eC = evals(rx, ry) if callable(evals) else evals
    expected2 = mul(comm_eval_Z, (rA * eA + rB * eB + rC * eC) % R_MOD)
    if not equality_verify(tr, g1, proof["proof_eq_sc_phase2"], expected2, comm_claim_post2):
        return None
    return rx, ry


def verify_instance(tr, proof, num_cons, num_vars, mats, inputs, gens):
    """verify with A, B, C(rx, ry) = r1cs_model.evaluate at the challenges the verifier derives (what SNARK::verify's second half establishes)"""
    return verify(tr, proof, num_vars, num_cons, inputs, lambda rx, ry: rm.evaluate(num_cons, num_vars, mats, rx, ry), gens)


# ---- bytes ----------------------------------------------------------------------------------------------------------------------

def proof_bytes(p):
    """the layout of sbn_r1cs_proof_prove's out_proof: the fields of R1CSProof in declaration order (r1csproof.rs:187-202)"""
    cp = ol.g1_compress
    pok, prod = p["pok_claims_phase2"]
    out = b"".join(cp(c) for c in p["comm_vars"])
    out += zm.proof_bytes(p["sc_proof_phase1"])
    out += b"".join(cp(c) for c in p["claims_phase2"])
    out += cp(pok["alpha"]) + sb(pok["z1"]) + sb(pok["z2"])
    out += cp(prod["alpha"]) + cp(prod["beta"]) + cp(prod["delta"]) + b"".join(sb(z) for z in prod["z"])
    out += cp(p["proof_eq_sc_phase1"]["alpha"]) + sb(p["proof_eq_sc_phase1"]["z"])
    out += zm.proof_bytes(p["sc_proof_phase2"])
    out += cp(p["comm_vars_at_ry"])
    out += pm.proof_bytes(p["proof_eval_vars_at_ry"])
    out += cp(p["proof_eq_sc_phase2"]["alpha"]) + sb(p["proof_eq_sc_phase2"]["z"])
    return out


def proof_from_bytes(b, num_cons, num_vars):
    """-> proof dict, or None when a point does not decompress or a scalar is not canonical (the reference's deserialisation fails)"""
    assert len(b) == sizes(num_cons, num_vars)[1]
    f = {k: b[lo:hi] for k, (lo, hi) in field_spans(num_cons, num_vars).items()}

    def pts(x):
        return [ol.g1_decompress(x[i:i + 32]) for i in range(0, len(x), 32)]

    def scs(x):
        return [ib(x[i:i + 32]) for i in range(0, len(x), 32)]

    def eqp(x):
        return dict(alpha=pts(x[:32])[0], z=scs(x[32:])[0])
    pk = f["pok_claims_phase2"]
    pok = dict(alpha=pts(pk[:32])[0], z1=scs(pk[32:64])[0], z2=scs(pk[64:96])[0])
    pa, pb, pd = pts(pk[96:192])
    prod = dict(alpha=pa, beta=pb, delta=pd, z=scs(pk[192:]))
    p = dict(comm_vars=pts(f["comm_vars"]), sc_proof_phase1=zm.proof_from_bytes(f["sc_proof_phase1"], 4), claims_phase2=tuple(pts(f["claims_phase2"])),
             pok_claims_phase2=(pok, prod), proof_eq_sc_phase1=eqp(f["proof_eq_sc_phase1"]), sc_proof_phase2=zm.proof_from_bytes(f["sc_proof_phase2"], 3),
             comm_vars_at_ry=pts(f["comm_vars_at_ry"])[0], proof_eval_vars_at_ry=pm.proof_from_bytes(f["proof_eval_vars_at_ry"]),
             proof_eq_sc_phase2=eqp(f["proof_eq_sc_phase2"]))
    points = p["comm_vars"] + list(p["claims_phase2"]) + [pok["alpha"], pa, pb, pd, p["proof_eq_sc_phase1"]["alpha"], p["comm_vars_at_ry"], p["proof_eq_sc_phase2"]["alpha"]]
    scalars = [pok["z1"], pok["z2"]] + prod["z"] + [p["proof_eq_sc_phase1"]["z"], p["proof_eq_sc_phase2"]["z"], p["proof_eval_vars_at_ry"]["z1"] if p["proof_eval_vars_at_ry"] else 0,
                                                   p["proof_eval_vars_at_ry"]["z2"] if p["proof_eval_vars_at_ry"] else 0]
    if any(x is None for x in points) or any(x >= R_MOD for x in scalars) or None in (p["sc_proof_phase1"], p["sc_proof_phase2"], p["proof_eval_vars_at_ry"]):
        return None
    return p


# ---- instances ------------------------------------------------------------------------------------------------------------------

def satisfying_instance(nc, nv, n_in, seed):
    """sparse random A and B rows, a random witness, and C with one entry per row at the constant-one column num_vars whose value is
    (Az)_i (Bz)_i -> (mats as (rows, cols, vals) triplets of ints, vars, inputs)"""
    rng = random.Random(seed)
    vars_ = [rng.randrange(R_MOD) for _ in range(nv)]
    inputs = [rng.randrange(R_MOD) for _ in range(n_in)]
    z = build_z(vars_, inputs)
    live = nv + 1 + n_in                                   # columns that carry a value

    def sparse():
        rows, cols, vals = [], [], []
        for i in range(nc):
            for _ in range(rng.randrange(1, 4)):
                rows.append(i); cols.append(rng.randrange(live)); vals.append(rng.choice([1, R_MOD - 1, rng.randrange(R_MOD)]))
        return rows, cols, vals
    A, B = sparse(), sparse()
    Az, Bz, _ = rm.multiply_vec(nc, nv, (A, B, ([], [], [])), z)
    C = (list(range(nc)), [nv] * nc, [a * b % R_MOD for a, b in zip(Az, Bz)])
    return (A, B, C), vars_, inputs


def random_rnd(num_cons, num_vars, seed):
    rng = random.Random(seed)
    return [rng.randrange(R_MOD) for _ in range(sizes(num_cons, num_vars)[0])]
