"""SparseMatPolyEvalProof of the KZG build (--features kzg) in plain Python: a literal restatement of the reference's prover AND verifier, the
checker of sbn_sparse_eval_prove_kzg and sbn_derefs_key.

    prove:   SparseMatPolyEvalProof::prove (sparse_mlpoly_full.rs:1757-1813) -> Derefs::commit_kzg (:307-312) with DerefsCommitment's transcript
             lines (:349-356, kzg.rs:386-404), PolyEvalNetworkProof::prove -> HashLayerProof::prove with DerefsEvalProof::prove (:503-550) ->
             KZGProof::prove (kzg.rs:174-192)
    verify:  SparseMatPolyEvalProof::verify -> ... -> DerefsEvalProof::verify (:552-595) -> KZGProof::verify (kzg.rs:196-217)

Everything that is the same in both builds comes from sparse_eval_model (layers, the product layer, the two Hyrax openings of comb_ops and
comb_mem); kzg_model gives evaluate_poly and compute_quotient.  The SRS comes from a KNOWN tau, so C = [p(tau)]G and pi = [q(tau)]G are one
scalar multiplication each, and the pairing check e(C - eval G, G2) == e(pi, (tau - z) G2) is stated as C - eval G == (tau - z) pi.
Scalars are Python integers mod r; points are 64-byte canonical affine x || y (the identity: 64 zero bytes).
"""
import dense_model as dm
import kzg_model as km
import oracle_lib as ol
import polyeval_model as pm
import product_proof_model as ppm
import sparse_eval_model as sem
from sparse_eval_model import R, Transcript  # noqa: F401

NAME = sem.NAME
G = (1).to_bytes(32, "little") + (2).to_bytes(32, "little")
INF = bytes(64)
FIELDS = sem.FIELDS
KINDS = ("ops", "mem")


class Srs:
    """powers_g1[i] = [tau^i]G for i < n (KZGSrs), held as the scalars tau^i: a commitment is one scalar multiplication"""

    def __init__(self, tau, n):
        self.tau, self.n = tau % R, n

    def powers(self, n):
        out, x = [], 1
        for _ in range(n):
            out.append(x); x = x * self.tau % R
        return out

    def commit_scalar(self, coeffs):
        """sum_i coeffs[i] tau^i over the coefficients the SRS covers"""
        return km.evaluate_poly(list(coeffs)[:self.n], self.tau)


def mul_g(k):
    return ol.g1_mul(G, pm.sb(k % R)) if k % R else INF


def sizes(nx, ny, N, batch):
    """(scalars of rnd, bytes of the proof) — counted from the structure"""
    s = sem.Shape(nx, ny, N, batch)
    b, n, m = s.b, s.n, s.m
    rnd = sum(3 + 2 * s.lg[k] for k in KINDS)
    pcepb = lambda c, l, d: 128 * sum(range(l)) + 32 * (2 * c * l + 3 * d)
    scalars = 2 * (2 + 2 * b) + 2 * b + 2 * (2 * b + 1) + b + 2 * b
    return rnd, 32 + 32 * scalars + pcepb(4, m, 0) + pcepb(4 * b, n, 2 * b) + sum(64 * s.lg[k] + 128 for k in KINDS) + 64


def split_rnd(rnd, shape):
    out, o = {}, 0
    for k in KINDS:                                                                              # the derefs opening draws nothing (:510 _random_tape)
        n = 3 + 2 * shape.lg[k]
        out[k] = list(rnd[o:o + n]); o += n
    assert o == len(rnd)
    return out


def commit_kzg(comb, srs):
    """KZGPolyCommitment::commit (kzg.rs:386-397): the first min(len, srs) coefficients"""
    return mul_g(srs.commit_scalar(comb))


def append_derefs_commitment(tr, C):
    """:349-356 with kzg.rs:399-403"""
    tr.append_message(b"derefs_commitment", b"begin_derefs_commitment")
    tr.append_message(b"comm_poly_row_col_ops_val", ol.g1_compress(C))
    tr.append_message(b"derefs_commitment", b"end_derefs_commitment")


def derefs_reduce(tr, evals):
    """the lines DerefsEvalProof::prove and ::verify share (:512-538) -> kzg_eval_point"""
    tr.append_message(b"protocol-name", b"Derefs evaluation proof (KZG)")
    sem.append_scalars(tr, b"evals_ops_val", evals)
    ch = [tr.challenge_scalar(b"challenge_combine_n_to_one") for _ in range(sem.log2(len(evals)))]
    tr.append_scalar(b"joint_claim_eval", sem.bound_bot(evals, ch))
    return tr.challenge_scalar(b"kzg_eval_point")


def kzg_prove(coeffs, z, srs):
    """KZGProof::prove (kzg.rs:174-192) -> (pi, eval); panics (AssertionError) where the reference slices past the SRS (:186)"""
    y = km.evaluate_poly(coeffs, z)
    q = km.compute_quotient(coeffs, z, y)
    assert len(q) <= srs.n, "kzg.rs:186: the quotient has %d coefficients, the SRS %d points" % (len(q), srs.n)
    return mul_g(km.evaluate_poly(q, srs.tau)), y


def kzg_verify(C, z, y, pi, srs):
    """KZGProof::verify (kzg.rs:196-217), the pairing check as a relation in G1: C - y G == (tau - z) pi"""
    lhs = ol.g1_add(C, ol.g1_neg(mul_g(y))) if y % R else C
    rhs = ol.g1_mul(pi, pm.sb((srs.tau - z) % R)) if pi != INF and (srs.tau - z) % R else INF
    return lhs == rhs


def hash_layer_prove(tr, rand_mem, rand_ops, dense, row_ops_val, col_ops_val, derefs_comb, gens, srs, rnd, shape):
    """HashLayerProof::prove (:922-1046), KZG build"""
    tr.append_message(b"protocol-name", b"Sparse polynomial hash layer proof")
    ev = lambda z, r: ppm.evaluate_mle(z, r)
    e_row_val = [ev(p, rand_ops) for p in row_ops_val]
    e_col_val = [ev(p, rand_ops) for p in col_ops_val]
    z = derefs_reduce(tr, sem.pad(e_row_val + e_col_val))
    pi, y = kzg_prove(derefs_comb, z, srs)
    sides = []
    for side in (0, 1):
        sides.append(([ev([a % R for a in p], rand_ops) for p in dense.addr[side]], [ev(p, rand_ops) for p in dense.read_ts[side]],
                      ev(dense.audit_ts[side], rand_mem)))
    e_val = [ev(v, rand_ops) for v in dense.val]
    evals_ops = sem.pad(sides[0][0] + sides[0][1] + sides[1][0] + sides[1][1] + e_val)
    _, _, proof_ops, _, _ = pm.prove_single(tr, gens["ops"], dense.comb_ops, rand_ops, evals_ops, rnd["ops"], sem.OPS_LABELS)
    _, _, proof_mem, _, _ = pm.prove_single(tr, gens["mem"], dense.comb_mem, rand_mem, [sides[0][2], sides[1][2]], rnd["mem"], sem.MEM_LABELS)
    return {"eval_row": sides[0], "eval_col": sides[1], "eval_val": e_val, "eval_derefs": (e_row_val, e_col_val),
            "proof_ops": proof_ops, "proof_mem": proof_mem, "proof_derefs": (pi, y)}


def derefs_comb(dense, rx, ry):
    """dense.deref and Derefs::new (:275-279, :293-297) -> (mem_rx, mem_ry, row_ops_val, col_ops_val, comb)"""
    rx_ext, ry_ext = sem.equalize(rx, ry)
    mem_rx, mem_ry = pm.eq_evals(rx_ext), pm.eq_evals(ry_ext)
    row_ops_val = [dm.deref(a, mem_rx) for a in dense.addr[0]]
    col_ops_val = [dm.deref(a, mem_ry) for a in dense.addr[1]]
    return mem_rx, mem_ry, row_ops_val, col_ops_val, dm.merge(row_ops_val + col_ops_val)


def prove(tr, nx, ny, mats, rx, ry, evals, gens, srs, rnd):
    """SparseMatPolyEvalProof::prove, KZG build (:1757-1813).  gens: {"ops", "mem"}; `tr` moves on"""
    dense = dm.Dense(nx, ny, mats)
    shape = sem.Shape(nx, ny, dense.N, dense.batch)
    assert len(rx) == nx and len(ry) == ny
    tr.append_message(b"protocol-name", NAME)
    assert len(evals) == dense.batch                                                             # :1769
    mem_rx, mem_ry, row_ops_val, col_ops_val, comb = derefs_comb(dense, rx, ry)
    comm = commit_kzg(comb, srs)
    append_derefs_commitment(tr, comm)
    r_hash, r_multiset = tr.challenge_scalar(b"challenge_r_hash"), tr.challenge_scalar(b"challenge_r_hash")
    row = sem.layers_new(mem_rx, dense.addr[0], dense.read_ts[0], dense.audit_ts[0], row_ops_val, r_hash, r_multiset)
    col = sem.layers_new(mem_ry, dense.addr[1], dense.read_ts[1], dense.audit_ts[1], col_ops_val, r_hash, r_multiset)
    tr.append_message(b"protocol-name", NAME)
    prod, rand_mem, rand_ops = sem.product_layer_prove(tr, row, col, dense, row_ops_val, col_ops_val, evals)
    hashp = hash_layer_prove(tr, rand_mem, rand_ops, dense, row_ops_val, col_ops_val, comb, gens, srs, split_rnd(rnd, shape), shape)
    return {"comm_derefs": comm, "prod": prod, "hash": hashp}


def hash_layer_verify(tr, hp, rand_mem, rand_ops, claims_row, claims_col, claims_dotp, comm, comm_derefs, gens, srs, rx, ry, r_hash, r_multiset):
    """HashLayerProof::verify (:1114-1265), KZG build.  As the reference's DerefsEvalProof::verify (:552-595), the KZG opening is checked at
    kzg_eval_point against the proof's own eval: the joint claim is absorbed, not compared"""
    tr.append_message(b"protocol-name", b"Sparse polynomial hash layer proof")
    e_row_val, e_col_val = hp["eval_derefs"]
    z = derefs_reduce(tr, sem.pad(list(e_row_val) + list(e_col_val)))
    pi, y = hp["proof_derefs"]
    if not kzg_verify(comm_derefs, z, y, pi, srs):
        return False
    row_addr, row_read_ts, row_audit = hp["eval_row"]
    col_addr, col_read_ts, col_audit = hp["eval_col"]
    if not sem.verify_helper(rand_mem, claims_row, e_row_val, row_addr, row_read_ts, row_audit, rx, r_hash, r_multiset):
        return False
    if not sem.verify_helper(rand_mem, claims_col, e_col_val, col_addr, col_read_ts, col_audit, ry, r_hash, r_multiset):
        return False
    b = len(e_row_val)
    if len(claims_dotp) != 3 * b:
        return False
    for i in range(b):
        if claims_dotp[3 * i] != e_row_val[i] or claims_dotp[3 * i + 1] != e_col_val[i] or claims_dotp[3 * i + 2] != hp["eval_val"][i]:
            return False
    evals_ops = sem.pad(list(row_addr) + list(row_read_ts) + list(col_addr) + list(col_read_ts) + list(hp["eval_val"]))
    if not sem.joint_verify(tr, hp["proof_ops"], gens["ops"], rand_ops, evals_ops, comm[0], sem.OPS_LABELS):
        return False
    return sem.joint_verify(tr, hp["proof_mem"], gens["mem"], rand_mem, [row_audit, col_audit], comm[1], sem.MEM_LABELS)


def verify(tr, proof, comm, num_ops, num_mem_cells, rx, ry, evals, gens, srs):
    """SparseMatPolyEvalProof::verify (:1815-1845), KZG build -> bool.  comm = sem.commit_dense(...)"""
    tr.append_message(b"protocol-name", NAME)
    rx_ext, ry_ext = sem.equalize(rx, ry)
    assert 1 << len(rx_ext) == num_mem_cells
    append_derefs_commitment(tr, proof["comm_derefs"])
    r_hash, r_multiset = tr.challenge_scalar(b"challenge_r_hash"), tr.challenge_scalar(b"challenge_r_hash")
    tr.append_message(b"protocol-name", NAME)
    b = len(evals)
    got = sem.product_layer_verify(tr, proof["prod"], num_ops, num_mem_cells, evals)
    if got is None:
        return False
    claims_mem, rand_mem, claims_ops, claims_dotp, rand_ops = got
    if len(claims_mem) != 4 or len(claims_ops) != 4 * b:
        return False
    claims_row = (claims_mem[0], claims_ops[:b], claims_ops[b:2 * b], claims_mem[1])
    claims_col = (claims_mem[2], claims_ops[2 * b:3 * b], claims_ops[3 * b:], claims_mem[3])
    return hash_layer_verify(tr, proof["hash"], rand_mem, rand_ops, claims_row, claims_col, claims_dotp, comm, proof["comm_derefs"], gens, srs,
                             rx_ext, ry_ext, r_hash, r_multiset)


# ---- the proof as bytes, in the layout of include/sbn254.h --------------------------------------------------------------------

def field_lengths(shape):
    fl = dict(sem.field_lengths(shape))
    fl["comm_derefs"] = 32
    fl["hash.proof_derefs"] = 64
    return fl


def field_spans(shape):
    out, o = {}, 0
    fl = field_lengths(shape)
    for f in FIELDS:
        out[f] = (o, o + fl[f]); o += fl[f]
    return out


def _hyrax_view(proof):
    """the proof with the two KZG fields replaced by Hyrax-shaped stand-ins, for sparse_eval_model's serialisers of the shared fields"""
    return {"comm_derefs": [], "prod": proof["prod"], "hash": dict(proof["hash"], proof_derefs=proof["hash"]["proof_ops"])}


def field_bytes(proof):
    fb = dict(sem.field_bytes(_hyrax_view(proof)))
    fb["comm_derefs"] = ol.g1_compress(proof["comm_derefs"])
    pi, y = proof["hash"]["proof_derefs"]
    fb["hash.proof_derefs"] = ol.g1_compress(pi) + pm.sb(y)
    return fb


def proof_bytes(proof):
    fb = field_bytes(proof)
    return b"".join(fb[f] for f in FIELDS)


def proof_from_bytes(data, shape):
    """-> proof dict, or None when a point does not decompress"""
    sp = field_spans(shape)
    assert len(data) == sp[FIELDS[-1]][1]
    f = {k: data[lo:hi] for k, (lo, hi) in sp.items()}
    # the shared fields through sparse_eval_model's parser: a Hyrax-shaped byte string with stand-ins for the two KZG fields
    hs = sem.field_spans(shape)
    stand = dict(f)
    stand["comm_derefs"] = ol.g1_compress(G) * shape.Ld
    stand["hash.proof_derefs"] = ol.g1_compress(G) * (2 * shape.lg["derefs"] + 2) + bytes(64)
    assert all(len(stand[k]) == hs[k][1] - hs[k][0] for k in FIELDS)
    p = sem.proof_from_bytes(b"".join(stand[k] for k in FIELDS), shape)
    C = ol.g1_decompress(f["comm_derefs"])
    pi = ol.g1_decompress(f["hash.proof_derefs"][:32])
    y = int.from_bytes(f["hash.proof_derefs"][32:], "little")
    if p is None or C is None or pi is None or y >= R:
        return None
    p["comm_derefs"] = C
    p["hash"]["proof_derefs"] = (pi, y)
    return p


# ---- the key: per-cell sums of SRS powers -------------------------------------------------------------------------------------

def key_scalars(dense, srs):
    """{(side, a): sum of tau^((side b + k) N + i) over the ops i of polynomial k of that side that read cell a}: S[side][a] = [that]G"""
    b, N = dense.batch, dense.N
    pw = srs.powers(2 * b * N)
    out = {}
    for side in (0, 1):
        for k in range(b):
            for i, a in enumerate(dense.addr[side][k]):
                out[(side, a)] = (out.get((side, a), 0) + pw[(side * b + k) * N + i]) % R
    return out


def key_commit_scalar(dense, srs, mem_rx, mem_ry):
    """sum_a eq[a] S_a as a scalar multiple of G"""
    return sum(((mem_ry if side else mem_rx)[a] * s) for (side, a), s in key_scalars(dense, srs).items()) % R


def instance(shape_key, seed=0):
    """(mats, rx, ry, evals, rnd) of a shape: sparse_eval_model's instance with the KZG build's draws"""
    nx, ny, nnz = shape_key
    mats, rx, ry, evals, _ = sem.instance(shape_key, seed)
    return mats, rx, ry, evals, sem.random_scalars(sizes(nx, ny, dm.num_ops(mats), len(nnz))[0], 400 + seed)
