"""The single-sum form of R1CSProof::verify (r1csproof.rs:463-619) and ZKSumcheckInstanceProof::verify (sumcheck.rs:366-457) on oracle
arithmetic: what sbn_r1cs_proof_verify / sbn_zk_sumcheck_verify compute, with the same point table, the same scalars and the same term
lists the host code (csrc/abi_r1cs_verify.inc) builds.

No fresh point is multiplied.  The table holds the proof's points (from its bytes) and the generators; a "sum" is a list of at most 8 terms
(table index, scalar).  A point whose bytes the transcript needs (Cy of a round, phase 2's comm_claim, the `expected` point of an equality
proof) is one sum; every equation of the reference is one sum, moved to one side, that must be the identity.  Negated coefficients are r - x.
tests/test_r1cs_proof_verify_cpu.py holds this against the literal r1cs_proof_model.verify / zk_sumcheck_model.verify."""
import oracle_lib as ol
import polyeval_model as pm
import r1cs_proof_model as rpm
import zk_sumcheck_model as zm
from transcript_model import R_MOD

TERMS_MAX = 8
INF = bytes(64)
IDENT = bytes(31) + b"\x40"


def normalise(c):
    """a compressed point as the reference's deserialisation and serialisation leave it"""
    return IDENT if c[31] & 0x40 else bytes(c)


class Run:
    """the table and the equations of one call"""

    def __init__(self, points):
        self.T, self.eqs, self.sums = list(points), [], 0

    def total(self, terms):
        assert len(terms) <= TERMS_MAX and all(0 <= i < len(self.T) and 0 <= s < R_MOD for i, s in terms)
        acc = INF
        for i, s in terms:
            acc = ol.g1_add(acc, zm.mul(self.T[i], s))
        return acc

    def point(self, terms):
        """a sum whose bytes the transcript needs: one launch and one wait on the device"""
        self.sums += 1
        return self.total(terms)

    def equation(self, terms):
        self.eqs.append(list(terms))

    def verdict(self):
        return all(self.total(e) == INF for e in self.eqs)


def rounds(run, tr, comp, proof, nrounds, N, base, g, prev, prev_comp):
    """sumcheck.rs:366-457 with nizk/mod.rs:368-400 inside -> (r, the last comm_eval as terms, its bytes); g = (G1, H1, Gn, Hn) table indices"""
    G1, H1, Gn, Hn = g
    stride = (6 + N) * 32
    r = []
    for i in range(nrounds):
        iP = base + 4 * i
        iE, iD, iB = iP + 1, iP + 2, iP + 3
        z = [zm.ib(proof[stride * i + 128 + 32 * k:stride * i + 160 + 32 * k]) for k in range(N + 2)]
        tr.append_message(b"comm_poly", comp[iP])
        r_i = tr.challenge_scalar(b"challenge_nextround")
        tr.append_message(b"comm_claim_per_round", prev_comp)
        tr.append_message(b"comm_eval", comp[iE])
        w0, w1 = (tr.challenge_scalar(b"combine_two_claims_to_one") for _ in range(2))
        a = zm.a_vector((w0, w1), r_i, N)
        target = [(idx, w0 * s % R_MOD) for idx, s in prev] + [(iE, w1)]
        Cy = run.point(target)
        tr.append_message(b"protocol-name", b"dot product proof")
        tr.append_message(b"Cx", comp[iP])
        tr.append_message(b"Cy", ol.g1_compress(Cy))
        for s in a:
            tr.append_scalar(b"a", s)
        tr.append_message(b"delta", comp[iD])
        tr.append_message(b"beta", comp[iB])
        c = tr.challenge_scalar(b"c")
        run.equation([(iP, c), (iD, 1)] + [(Gn + k, (R_MOD - z[k]) % R_MOD) for k in range(N)] + [(Hn, (R_MOD - z[N]) % R_MOD)])
        run.equation([(idx, c * s % R_MOD) for idx, s in target] + [(iB, 1), (G1, (R_MOD - zm.dot(z[:N], a)) % R_MOD), (H1, (R_MOD - z[N + 1]) % R_MOD)])
        prev, prev_comp = [(iE, 1)], comp[iE]
        r.append(r_i)
    return r, prev, prev_comp


def equality(run, tr, C1, iC2, c2_comp, iAlpha, alpha_comp, z, H1):
    """nizk/mod.rs:126-149: C1 as terms, C2 and alpha points of the proof"""
    tr.append_message(b"protocol-name", b"equality proof")
    tr.append_message(b"C1", ol.g1_compress(run.point(C1)))
    tr.append_message(b"C2", c2_comp)
    tr.append_message(b"alpha", alpha_comp)
    c = tr.challenge_scalar(b"c")
    run.equation([(idx, c * s % R_MOD) for idx, s in C1] + [(iC2, (R_MOD - c) % R_MOD), (iAlpha, 1), (H1, (R_MOD - z) % R_MOD)])


def _decompress_all(comp):
    pts = [ol.g1_decompress(c) for c in comp]
    return None if any(p is None for p in pts) else pts


def _scalars_ok(b, offsets):
    return all(zm.ib(b[o:o + 32]) < R_MOD for o in offsets)


def zk_verify(tr, proof, comm_claim, nrounds, degree_bound, gens_1, gens_n):
    """sbn_zk_sumcheck_verify on a transcript copy -> (comm_evals[-1], r, Run) or None; the caller's transcript moves on only then"""
    N = degree_bound + 1
    stride = (6 + N) * 32
    assert len(proof) == stride * nrounds and nrounds >= 1
    if not _scalars_ok(proof, [stride * i + 128 + 32 * k for i in range(nrounds) for k in range(N + 2)]):
        return None
    comp = [normalise(proof[stride * i + 32 * k:stride * i + 32 * k + 32]) for i in range(nrounds) for k in range(4)]
    pts = _decompress_all(comp)
    if pts is None:
        return None
    np_ = 4 * nrounds
    run = Run(pts + [comm_claim, gens_1[0], gens_1[1]] + list(gens_n[0]) + [gens_n[1]])
    g = (np_ + 1, np_ + 2, np_ + 3, np_ + 3 + N)
    t = tr.clone()
    r, last, _ = rounds(run, t, comp, proof, nrounds, N, 0, g, [(np_, 1)], ol.g1_compress(comm_claim))
    if not run.verdict():
        return None
    tr.s = t.s
    return run.T[last[0][0]], r, run


def _open_check(t, opening_bytes, gens_pc, r, C_Zr, comm_bytes):
    """the opening of comm_vars by the literal model (polyeval_model.verify)"""
    comm = [ol.g1_decompress(comm_bytes[i:i + 32]) for i in range(0, len(comm_bytes), 32)]
    opening = pm.proof_from_bytes(opening_bytes)
    return opening is not None and all(c is not None for c in comm) and pm.verify(t, opening, gens_pc, r, C_Zr, comm)


def verify(tr, proof, num_cons, num_vars, inputs, evals, gens, run_cls=Run, decompress=_decompress_all, open_check=_open_check):
    """sbn_r1cs_proof_verify -> (rx, ry, Run) or None; proof: bytes; evals = (A, B, C)(rx, ry); `tr` moves on only behind an accepted proof.
    run_cls / decompress / open_check: where a caller puts its own arithmetic under the same term lists (tools/bench_r1cs_proof_verify.py)"""
    nx, ell = rpm.log2(num_cons), rpm.log2(num_vars)
    ny = ell + 1
    ml, lg = pm.factored_lens(ell)
    L = 1 << ml
    assert len(proof) == rpm.sizes(num_cons, num_vars)[1] and len(inputs) < num_vars
    sp = rpm.field_spans(num_cons, num_vars)
    o_comm, o_sc1, o_claims, o_pok, o_eq1, o_sc2, o_cy, o_open, o_eq2 = (sp[f][0] for f in rpm.FIELDS)
    sc_off = [o_sc1 + 320 * i + 128 + 32 * k for i in range(nx) for k in range(6)] + [o_sc2 + 288 * i + 128 + 32 * k for i in range(ny) for k in range(5)]
    sc_off += [o_pok + 32, o_pok + 64] + [o_pok + 192 + 32 * k for k in range(5)] + [o_eq1 + 32, o_eq2 + 32]
    if not _scalars_ok(proof, sc_off):
        return None
    cut = lambda o: proof[o:o + 32]                                  # noqa: E731
    nr = nx + ny
    comp = [cut(o_sc1 + 320 * i + 32 * k) for i in range(nx) for k in range(4)] + [cut(o_sc2 + 288 * i + 32 * k) for i in range(ny) for k in range(4)]
    comp += [cut(o_claims + 32 * k) for k in range(4)] + [cut(o_pok), cut(o_pok + 96), cut(o_pok + 128), cut(o_pok + 160), cut(o_eq1), cut(o_eq2), cut(o_cy)]
    comp = [normalise(c) for c in comp]
    pts = decompress(comp)
    if pts is None:
        return None
    b1, b2, iAz = 0, 4 * nx, 4 * nr
    iBz, iCz, iPr, iKa, iPa, iPb, iPd, iE1, iE2, iCv = (iAz + k for k in range(1, 11))
    np_ = 4 * nr + 11
    G1, H1 = np_, np_ + 1
    g4 = (G1, H1, H1 + 1, H1 + 5)
    g3 = (G1, H1, H1 + 6, H1 + 9)
    g1 = gens["g1"]
    run = run_cls(pts + [g1[0], g1[1]] + list(gens["g4"][0]) + [gens["g4"][1]] + list(gens["g3"][0]) + [gens["g3"][1]])
    sc = lambda o: zm.ib(proof[o:o + 32])                            # noqa: E731
    neg = lambda x: (R_MOD - x) % R_MOD                              # noqa: E731
    t = tr.clone()
    t.append_message(b"protocol-name", b"R1CS proof")
    for s in inputs:
        t.append_scalar(b"input", s)
    t.append_message(b"poly_commitment", b"poly_commitment_begin")
    for i in range(L):
        t.append_message(b"poly_commitment_share", normalise(cut(o_comm + 32 * i)))
    t.append_message(b"poly_commitment", b"poly_commitment_end")
    tau = [t.challenge_scalar(b"challenge_tau") for _ in range(nx)]
    rx, _, post1 = rounds(run, t, comp, proof[o_sc1:], nx, 4, b1, g4, [], IDENT)
    iPost1, iPost2 = b1 + 4 * (nx - 1) + 1, b2 + 4 * (ny - 1) + 1
    t.append_message(b"protocol-name", b"knowledge proof")
    t.append_message(b"C", comp[iCz]); t.append_message(b"alpha", comp[iKa])
    c = t.challenge_scalar(b"c")
    run.equation([(iCz, c), (iKa, 1), (G1, neg(sc(o_pok + 32))), (H1, neg(sc(o_pok + 64)))])
    t.append_message(b"protocol-name", b"product proof")
    for label, i in ((b"X", iAz), (b"Y", iBz), (b"Z", iPr), (b"alpha", iPa), (b"beta", iPb), (b"delta", iPd)):
        t.append_message(label, comp[i])
    c = t.challenge_scalar(b"c")
    z = [sc(o_pok + 192 + 32 * k) for k in range(5)]
    run.equation([(iPa, 1), (iAz, c), (G1, neg(z[0])), (H1, neg(z[1]))])
    run.equation([(iPb, 1), (iBz, c), (G1, neg(z[2])), (H1, neg(z[3]))])
    run.equation([(iPd, 1), (iPr, c), (iAz, neg(z[2])), (H1, neg(z[4]))])
    for label, i in ((b"comm_Az_claim", iAz), (b"comm_Bz_claim", iBz), (b"comm_Cz_claim", iCz), (b"comm_prod_Az_Bz_claims", iPr)):
        t.append_message(label, comp[i])
    tb = 1
    for r_i, t_i in zip(rx, tau):
        tb = tb * (r_i * t_i + (1 - r_i) * (1 - t_i)) % R_MOD
    equality(run, t, [(iPr, tb), (iCz, neg(tb))], iPost1, post1, iE1, comp[iE1], sc(o_eq1 + 32), H1)
    rA, rB, rC = (t.challenge_scalar(l) for l in (b"challenge_Az", b"challenge_Bz", b"challenge_Cz"))
    claim2 = [(iAz, rA), (iBz, rB), (iCz, rC)]
    ry, _, post2 = rounds(run, t, comp, proof[o_sc2:], ny, 3, b2, g3, claim2, ol.g1_compress(run.point(claim2)))
    if not open_check(t, proof[o_open:o_eq2], gens["pc"], ry[1:], run.T[iCv], proof[o_comm:o_sc1]):
        return None

    def chi(i):
        e = 1
        for j in range(ell):
            e = e * (ry[1 + j] if (i >> (ell - 1 - j)) & 1 else 1 - ry[1 + j]) % R_MOD
        return e
    pie = (chi(0) + sum(v * chi(i + 1) for i, v in enumerate(inputs))) % R_MOD
    eA, eB, eC = evals
    s = (rA * eA + rB * eB + rC * eC) % R_MOD
    equality(run, t, [(iCv, s * (1 - ry[0]) % R_MOD), (G1, s * ry[0] % R_MOD * pie % R_MOD)], iPost2, post2, iE2, comp[iE2], sc(o_eq2 + 32), H1)
    assert len(run.eqs) == 2 * nr + 6 and run.sums == nr + 3
    if not run.verdict():
        return None
    tr.s = t.s
    return rx, ry, run


# ---- what a verifier must refuse: one proof, changed in one place ------------------------------------------------------------------

def undecodable_point():
    """32 bytes that are no compressed point: the smallest x for which x^3 + 3 is no square"""
    x = 1
    while ol.g1_decompress(x.to_bytes(32, "little")) is not None:
        x += 1
    return x.to_bytes(32, "little")


def tamperings(proof, num_cons, num_vars):
    """name -> proof bytes: the flipped byte of each field that tests/test_r1cs_proof_cpu.py uses (the lowest byte of the field's last
    element, an x coordinate or a scalar), a point that does not decompress, a response scalar >= r"""
    spans = rpm.field_spans(num_cons, num_vars)
    out = {}
    for field in rpm.FIELDS:
        b = bytearray(proof)
        b[spans[field][1] - 32] ^= 1
        out["flipped byte in " + field] = bytes(b)
    lo = spans["claims_phase2"][0]
    out["comm_Az_claim does not decompress"] = proof[:lo] + undecodable_point() + proof[lo + 32:]
    lo = spans["sc_proof_phase1"][0] + 64
    out["delta of round 0 does not decompress"] = proof[:lo] + undecodable_point() + proof[lo + 32:]
    hi = spans["proof_eq_sc_phase1"][1]
    out["z of the first equality proof >= r"] = proof[:hi - 32] + R_MOD.to_bytes(32, "little") + proof[hi:]
    lo = spans["sc_proof_phase2"][0] + 128
    out["z[0] of phase 2 round 0 is z + r"] = proof[:lo] + (zm.ib(proof[lo:lo + 32]) + R_MOD).to_bytes(32, "little") + proof[lo + 32:]
    return out
