"""ZKSumcheckInstanceProof in plain Python: a literal restatement of the reference's two ZK sumcheck provers, of DotProductProof::prove, and of
their verifiers — the checker of sbn_zk_sumcheck_prove_r1cs / sbn_zk_sumcheck_prove_quad.

    prove_r1cs:  ZKSumcheckInstanceProof::prove_cubic_with_additive_term (sumcheck.rs:465-649), comb_func = tau * (Az * Bz - Cz) (r1csproof.rs)
    prove_quad:  ZKSumcheckInstanceProof::prove_quad (sumcheck.rs:657-811), comb_func = z * ABC
    dotproduct_prove / dotproduct_verify:  DotProductProof::prove / ::verify (nizk/mod.rs:306-366, :368-400)
    verify:      ZKSumcheckInstanceProof::verify (sumcheck.rs:366-457)
    round_from_sums: one round of either prover from the round's sums (e0, e2[, e3]) — what replays a proof from sums computed elsewhere

UniPoly::from_evals (unipoly.rs:28-59) of 4 (3) values always yields 4 (3) coefficients — a leading zero is kept — and poly.as_vec()
(unipoly.rs:65-67) is that coefficient vector, lowest degree first; so x_vec, a_vec and gens_n all have n = 4 (3) entries in every round.

Built on pyref.py (the sums, the binds, from_evals), transcript_model.py (Merlin) and the C oracle's group operations, on the same footing as
polyeval_model.py.  Scalars are Python integers mod r; points are 64-byte canonical affine x || y (all-zero = infinity).
gens_1 = (G, h) with one generator; gens_n = ([G_0 .. G_{n-1}], h).  The two h are different points in the reference (R1CSSumcheckGens::new).
"""
import oracle_lib as ol
import pyref
from transcript_model import R_MOD, Transcript  # noqa: F401

INF = bytes(64)


def sb(x):
    return int(x % R_MOD).to_bytes(32, "little")


def ib(b):
    return int.from_bytes(b, "little")


def mul(p, k):
    return ol.g1_mul(p, sb(k))


def commit_vec(xs, blind, gens_n):
    """Commitments::commit for a vector (commitments.rs:144-154): sum x_i G_i + blind h"""
    G, h = gens_n
    assert len(xs) == len(G)
    acc = mul(h, blind)
    for x, g in zip(xs, G):
        acc = ol.g1_add(acc, mul(g, x))
    return acc


def commit_one(x, blind, gens_1):
    G, h = gens_1
    return ol.g1_add(mul(G, x), mul(h, blind))


def append_point(tr, label, p):
    tr.append_message(label, ol.g1_compress(p))            # transcript.rs:102-108


def dot(a, b):
    return sum(x * y for x, y in zip(a, b)) % R_MOD


class Tape:
    """the caller's RandomTape draws as sbn_zk_sumcheck_prove_* takes them: a flat list, consumed front to back"""

    def __init__(self, rnd):
        self.rnd, self.pos = list(rnd), 0

    def take(self, k):
        out = self.rnd[self.pos:self.pos + k]
        assert len(out) == k, "the tape ran out"
        self.pos += k
        return out


def dotproduct_prove(tr, tape, gens_1, gens_n, x_vec, blind_x, a_vec, y, blind_y):
    """nizk/mod.rs:306-366 -> (proof dict, Cx, Cy)"""
    tr.append_message(b"protocol-name", b"dot product proof")
    n = len(x_vec)
    assert len(a_vec) == n and len(gens_n[0]) == n
    d_vec = tape.take(n)
    r_delta, r_beta = tape.take(2)
    Cx = commit_vec(x_vec, blind_x, gens_n)
    append_point(tr, b"Cx", Cx)
    Cy = commit_one(y, blind_y, gens_1)
    append_point(tr, b"Cy", Cy)
    for s in a_vec:
        tr.append_scalar(b"a", s)
    delta = commit_vec(d_vec, r_delta, gens_n)
    append_point(tr, b"delta", delta)
    beta = commit_one(dot(a_vec, d_vec), r_beta, gens_1)
    append_point(tr, b"beta", beta)
    c = tr.challenge_scalar(b"c")
    z = [(c * x + d) % R_MOD for x, d in zip(x_vec, d_vec)]
    z_delta = (c * blind_x + r_delta) % R_MOD
    z_beta = (c * blind_y + r_beta) % R_MOD
    return dict(delta=delta, beta=beta, z=z, z_delta=z_delta, z_beta=z_beta), Cx, Cy


def dotproduct_verify(tr, proof, gens_1, gens_n, a, Cx, Cy):
    """nizk/mod.rs:368-400 -> bool"""
    assert len(gens_n[0]) == len(a)
    tr.append_message(b"protocol-name", b"dot product proof")
    append_point(tr, b"Cx", Cx); append_point(tr, b"Cy", Cy)
    for s in a:
        tr.append_scalar(b"a", s)
    append_point(tr, b"delta", proof["delta"]); append_point(tr, b"beta", proof["beta"])
    c = tr.challenge_scalar(b"c")
    ok = ol.g1_add(mul(Cx, c), proof["delta"]) == commit_vec(proof["z"], proof["z_delta"], gens_n)
    ok &= ol.g1_add(mul(Cy, c), proof["beta"]) == commit_one(dot(proof["z"], a), proof["z_beta"], gens_1)
    return bool(ok)


def a_vector(w, r_j, n):
    """sumcheck.rs:597-619: w[0] * [2, 1, 1 ..] + w[1] * [1, r, r^2 ..]"""
    a_sc = [2] + [1] * (n - 1)
    a_eval = [pow(r_j, k, R_MOD) for k in range(n)]
    return [(w[0] * s + w[1] * e) % R_MOD for s, e in zip(a_sc, a_eval)]


class _State:
    """what a prover carries from round to round"""

    def __init__(self, claim, blind_claim, gens_1, blinds_poly, blinds_evals):
        self.claim, self.blind_claim = claim % R_MOD, blind_claim
        self.comm_claim = commit_one(claim, blind_claim, gens_1)      # sumcheck.rs:487
        self.blinds_poly, self.blinds_evals = blinds_poly, blinds_evals
        self.r, self.comm_polys, self.comm_evals, self.proofs = [], [], [], []


def round_from_sums(tr, tape, st, j, sums, gens_1, gens_n):
    """the body of the round loop behind the sums (sumcheck.rs:532-640 / :701-802) -> r_j; sums = (e0, e2, e3) or (e0, e2)"""
    evals = [sums[0], (st.claim - sums[0]) % R_MOD] + list(sums[1:])
    poly = pyref.unipoly_from_evals(evals)
    assert len(poly) == len(evals) == len(gens_n[0])
    comm_poly = commit_vec(poly, st.blinds_poly[j], gens_n)
    append_point(tr, b"comm_poly", comm_poly)
    r_j = tr.challenge_scalar(b"challenge_nextround")
    ev = pyref.unipoly_eval(poly, r_j)
    comm_eval = commit_one(ev, st.blinds_evals[j], gens_1)
    append_point(tr, b"comm_claim_per_round", st.comm_claim)
    append_point(tr, b"comm_eval", comm_eval)
    w = [tr.challenge_scalar(b"combine_two_claims_to_one") for _ in range(2)]
    target = (w[0] * st.claim + w[1] * ev) % R_MOD
    blind_sc = st.blind_claim if j == 0 else st.blinds_evals[j - 1]
    blind = (w[0] * blind_sc + w[1] * st.blinds_evals[j]) % R_MOD
    assert commit_one(target, blind, gens_1) == ol.g1_add(mul(st.comm_claim, w[0]), mul(comm_eval, w[1]))      # debug_assert_eq, :595
    a = a_vector(w, r_j, len(poly))
    proof, Cx, _ = dotproduct_prove(tr, tape, gens_1, gens_n, poly, st.blinds_poly[j], a, target, blind)
    assert Cx == comm_poly
    st.proofs.append(proof); st.comm_polys.append(comm_poly); st.comm_evals.append(comm_eval); st.r.append(r_j)
    st.claim, st.comm_claim = ev, comm_eval
    return r_j


def _prove(tr, rnd, claim, blind_claim, tables, gens_1, gens_n, eval_fn):
    num_rounds = len(tables[0]).bit_length() - 1
    assert all(len(t) == 1 << num_rounds for t in tables) and num_rounds >= 1
    tape = Tape(rnd)
    blinds_poly = tape.take(num_rounds)                    # random_vector(b"blinds_poly", num_rounds)
    blinds_evals = tape.take(num_rounds)
    st = _State(claim, blind_claim, gens_1, blinds_poly, blinds_evals)
    tables = [list(t) for t in tables]
    for j in range(num_rounds):
        r_j = round_from_sums(tr, tape, st, j, eval_fn(*tables), gens_1, gens_n)
        tables = [pyref.bind_top(t, r_j) for t in tables]
    assert tape.pos == len(tape.rnd), "rnd holds more than num_rounds * (n + 4) scalars"
    proof = dict(comm_polys=st.comm_polys, comm_evals=st.comm_evals, proofs=st.proofs)
    return proof, st.r, [t[0] for t in tables], blinds_evals[num_rounds - 1]


def prove_r1cs(tr, rnd, claim, blind_claim, tau, Az, Bz, Cz, gens_1, gens_4):
    """sumcheck.rs:465-649 -> (proof dict, r, [tau[0], Az[0], Bz[0], Cz[0]], blinds_evals[-1])"""
    return _prove(tr, rnd, claim, blind_claim, [tau, Az, Bz, Cz], gens_1, gens_4, pyref.sc_eval_r1cs)


def prove_quad(tr, rnd, claim, blind_claim, Z, ABC, gens_1, gens_3):
    """sumcheck.rs:657-811 -> (proof dict, r, [z[0], ABC[0]], blinds_evals[-1])"""
    return _prove(tr, rnd, claim, blind_claim, [Z, ABC], gens_1, gens_3, pyref.sc_eval_quad)


def replay(tr, rnd, claim, blind_claim, round_sums, gens_1, gens_n):
    """the prover's transcript and commitments from round sums computed elsewhere -> (proof dict, r)"""
    num_rounds = len(round_sums)
    tape = Tape(rnd)
    blinds_poly = tape.take(num_rounds); blinds_evals = tape.take(num_rounds)
    st = _State(claim, blind_claim, gens_1, blinds_poly, blinds_evals)
    for j, sums in enumerate(round_sums):
        round_from_sums(tr, tape, st, j, sums, gens_1, gens_n)
    return dict(comm_polys=st.comm_polys, comm_evals=st.comm_evals, proofs=st.proofs), st.r


def verify(tr, proof, comm_claim, num_rounds, degree_bound, gens_1, gens_n):
    """sumcheck.rs:366-457 -> (comm_evals[-1], r) or None"""
    if len(proof["comm_polys"]) != num_rounds or len(proof["proofs"]) != num_rounds or len(proof["comm_evals"]) != num_rounds:
        return None
    comm_claim_per_round = comm_claim
    r = []
    for i in range(num_rounds):
        append_point(tr, b"comm_poly", proof["comm_polys"][i])
        r_i = tr.challenge_scalar(b"challenge_nextround")
        append_point(tr, b"comm_claim_per_round", comm_claim_per_round)
        append_point(tr, b"comm_eval", proof["comm_evals"][i])
        w = [tr.challenge_scalar(b"combine_two_claims_to_one") for _ in range(2)]
        comm_target = ol.g1_add(mul(comm_claim_per_round, w[0]), mul(proof["comm_evals"][i], w[1]))
        a = a_vector(w, r_i, degree_bound + 1)
        if not dotproduct_verify(tr, proof["proofs"][i], gens_1, gens_n, a, proof["comm_polys"][i], comm_target):
            return None
        comm_claim_per_round = proof["comm_evals"][i]
        r.append(r_i)
    return proof["comm_evals"][-1], r


def proof_bytes(p):
    """the layout of out_proof: per round comm_poly, comm_eval, delta, beta (compressed), z[n], z_delta, z_beta"""
    out = b""
    for cp, ce, dp in zip(p["comm_polys"], p["comm_evals"], p["proofs"]):
        out += ol.g1_compress(cp) + ol.g1_compress(ce) + ol.g1_compress(dp["delta"]) + ol.g1_compress(dp["beta"])
        out += b"".join(sb(z) for z in dp["z"]) + sb(dp["z_delta"]) + sb(dp["z_beta"])
    return out


def proof_from_bytes(b, n):
    """-> proof dict, or None when a point does not decompress or a scalar is not canonical (the reference's deserialisation fails)"""
    stride = (6 + n) * 32
    assert len(b) % stride == 0
    p = dict(comm_polys=[], comm_evals=[], proofs=[])
    for o in range(0, len(b), stride):
        pts = [ol.g1_decompress(b[o + 32 * i:o + 32 * i + 32]) for i in range(4)]
        sc = [ib(b[o + 128 + 32 * i:o + 160 + 32 * i]) for i in range(n + 2)]
        if any(x is None for x in pts) or any(s >= R_MOD for s in sc):
            return None
        p["comm_polys"].append(pts[0]); p["comm_evals"].append(pts[1])
        p["proofs"].append(dict(delta=pts[2], beta=pts[3], z=sc[:n], z_delta=sc[n], z_beta=sc[n + 1]))
    return p


def split_gens(xy, n):
    """sbn_gens_new(n, label)'s n + 1 points -> ([G_0 .. G_{n-1}], h)"""
    pts = [xy[64 * i:64 * i + 64] for i in range(n + 1)]
    return pts[:n], pts[n]


def gens_1_of(xy):
    G, h = split_gens(xy, 1)
    return G[0], h
