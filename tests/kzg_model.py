"""Pure-int model of the reference's KZG prover arithmetic (kzg.rs): evaluate_poly, compute_quotient and batch_prove's combination."""
R = 0x30644e72e131a029b85045b68181585d2833e84879b9709143e1f593f0000001


def evaluate_poly(coeffs, z):
    """kzg.rs:220-229: sum_i coeffs[i] z^i"""
    acc, pw = 0, 1
    for c in coeffs:
        acc = (acc + c * pw) % R
        pw = pw * z % R
    return acc


def compute_quotient(coeffs, z, y):
    """kzg.rs:232-260: synthetic division of p - y by (X - z); [] for fewer than two coefficients"""
    if len(coeffs) <= 1:
        return []
    p = list(coeffs)
    p[0] = (p[0] - y) % R
    n = len(p)
    q = [0] * (n - 1)
    rem = p[n - 1]
    for i in range(n - 2, -1, -1):
        q[i] = rem
        rem = (p[i] + rem * z) % R
    return q


def combine(polys, gamma):
    """kzg.rs:278-288: sum_k gamma^k p_k over max(len) coefficients"""
    out = [0] * max((len(p) for p in polys), default=0)
    gp = 1
    for p in polys:
        for i, c in enumerate(p):
            out[i] = (out[i] + c * gp) % R
        gp = gp * gamma % R
    return out


def batch_prove(polys, z, gamma):
    """KZGBatchedEvalProof::prove -> KZGBatchProof::batch_prove (kzg.rs:478-500, 268-312): (evals, combined eval, quotient)"""
    evals = [evaluate_poly(p, z) for p in polys]
    y, gp = 0, 1
    for e in evals:
        y = (y + e * gp) % R
        gp = gp * gamma % R
    return evals, y, compute_quotient(combine(polys, gamma), z, y)


def to_bytes(vals):
    return b"".join(int(v).to_bytes(32, "little") for v in vals)


def from_bytes(b):
    return [int.from_bytes(b[i:i + 32], "little") for i in range(0, len(b), 32)]
