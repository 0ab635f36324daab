"""The form in which sbn_polyeval_verify checks an opening, in plain Python on oracle arithmetic: DotProductProofLog::verify's final equation
(nizk/mod.rs:560-565) moved to one side,

    a c (sum u_i^2 L_i + sum u_i^-2 R_i + Cx + r Cy) + a beta + delta - z1 sum_j s_j G_j - z1 a r G1 - z2 h = 0,      a = b_hat = <s, R>

one sum over 2 lg n + 4 proof points and the n + 2 generators, with b_hat in closed form.  tests/test_polyeval_verify_cpu.py holds it against the
literal restatement (polyeval_model.dotproduct_verify); the tampering list of the reject tests lives here, shared by the CPU and GPU tests.
"""
import oracle_lib as ol
import polyeval_model as pm
from polyeval_model import R_MOD


def b_hat_closed(us, r_right):
    """<compute_s(us), eq(r_right)> as a product: both vectors are tensor products, and bit b of an index picks u[lg-1-b] / r[lg-1-b] in both"""
    assert len(us) == len(r_right)
    out = 1
    for u, rk in zip(us, r_right):
        out = out * (pow(u, -1, R_MOD) * (1 - rk) + u * rk) % R_MOD
    return out


def folded_terms(tr, proof, gens, r_right, Cx, Cy):
    """the transcript of DotProductProofLog::verify, then (scalars, points) of the single sum"""
    G, Qb, H = gens
    n = len(G)
    lg = n.bit_length() - 1
    assert len(proof["L"]) == lg and len(proof["R"]) == lg and len(r_right) == lg
    tr.append_message(b"protocol-name", b"dot product proof (log)")
    pm.append_point(tr, b"Cx", Cx); pm.append_point(tr, b"Cy", Cy)
    for s in pm.eq_evals(r_right):
        tr.append_scalar(b"a", s)
    rq = tr.challenge_scalar(b"r")
    us = []
    for i in range(lg):
        pm.append_point(tr, b"L", proof["L"][i]); pm.append_point(tr, b"R", proof["R"][i])
        us.append(tr.challenge_scalar(b"u"))
    pm.append_point(tr, b"delta", proof["delta"]); pm.append_point(tr, b"beta", proof["beta"])
    c = tr.challenge_scalar(b"c")
    a = b_hat_closed(us, r_right)
    ac = a * c % R_MOD
    z1, z2 = proof["z1"], proof["z2"]
    scalars = [ac * u * u % R_MOD for u in us] + [ac * pow(u, -2, R_MOD) % R_MOD for u in us] + [1, a, ac, ac * rq % R_MOD]
    points = list(proof["L"]) + list(proof["R"]) + [proof["delta"], proof["beta"], Cx, Cy]
    scalars += [-z1 * s % R_MOD for s in pm.compute_s(us)] + [-z1 * a * rq % R_MOD, -z2 % R_MOD]
    points += list(G) + [Qb, H]
    return scalars, points


def dotproduct_verify_folded(tr, proof, gens, r_right, Cx, Cy):
    scalars, points = folded_terms(tr, proof, gens, r_right, Cx, Cy)
    return pm.msm(scalars, points) == pm.INF


def verify_folded(tr, proof, gens, r, C_Zr, comm_C):
    """PolyEvalProof::verify (hyrax.rs:118-137) with the folded final check"""
    tr.append_message(b"protocol-name", b"polynomial evaluation proof")
    ml, _ = pm.factored_lens(len(r))
    C_LZ = pm.msm(pm.eq_evals(r[:ml]), comm_C)
    return dotproduct_verify_folded(tr, proof, gens, r[ml:], C_LZ, C_Zr)


# ---- the reject list: every way a test replaces one input of a good verification by another VALID value ---------------------------

def generator():
    return ol.g1_mul_gen_batch(pm.sb(1), 1)


def tamperings(ell):
    """names of the single replacements at this ell"""
    lg = pm.factored_lens(ell)[1]
    names = [f"L_{i}" for i in range(lg)] + [f"R_{i}" for i in range(lg)] + ["delta", "beta", "z1", "z2", "r", "C_Zr", "gens"]
    if ell >= 2:
        names.append("comm_swap")                           # two rows need L_size >= 2
    return names


def tamper(what, proof, r, C_Zr, comm, gens, other_gens):
    """-> (proof, r, C_Zr, comm, gens) with the one replacement `what` names; every value stays a valid one of its kind"""
    proof = {k: (list(v) if isinstance(v, list) else v) for k, v in proof.items()}
    r, comm = list(r), list(comm)
    g = generator()
    if what[:2] in ("L_", "R_"):
        proof[what[0]][int(what[2:])] = ol.g1_add(proof[what[0]][int(what[2:])], g)
    elif what in ("delta", "beta"):
        proof[what] = ol.g1_add(proof[what], g)
    elif what in ("z1", "z2"):
        proof[what] = (proof[what] + 1) % R_MOD
    elif what == "r":
        r[-1] = (r[-1] + 1) % R_MOD
    elif what == "C_Zr":
        C_Zr = ol.g1_add(C_Zr, gens[1])                     # the commitment to Zr + 1 under the same blind
    elif what == "comm_swap":
        comm[0], comm[1] = comm[1], comm[0]
    elif what == "gens":
        gens = other_gens
    else:
        raise ValueError(what)
    return proof, r, C_Zr, comm, gens
