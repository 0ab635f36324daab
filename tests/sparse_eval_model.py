"""SparseMatPolyEvalProof in plain Python: a literal restatement of the reference's prover AND verifier (the Hyrax build), the checker of
sbn_sparse_eval_prove.

    prove:   SparseMatPolyEvalProof::prove (sparse_mlpoly_full.rs:1700-1755) -> equalize (:1681-1697), Derefs::new / ::commit (:293-304, :341-347),
             PolyEvalNetwork::new -> Layers::new -> build_hash_layer (:745-866), PolyEvalNetworkProof::prove (:1546-1579) ->
             ProductLayerProof::prove (:1306-1428) and HashLayerProof::prove (:922-1046) with DerefsEvalProof::prove (:412-432)
    verify:  SparseMatPolyEvalProof::verify (:1815-1845) -> PolyEvalNetworkProof::verify (:1581-1650) -> ProductLayerProof::verify (:1436-1520),
             ProductCircuitEvalProofBatched::verify (product_tree.rs:394-537) and HashLayerProof::verify / verify_helper (:1048-1265),
             DerefsEvalProof::verify (:459-481)

It stands on dense_model (the dense representation), product_proof_model (the layered prover), polyeval_model (the openings, prover and
verifier) and transcript_model (Merlin).  product_proof_model's verifier compares against the prover's `rand` and `claims_final`, which are
not part of a proof and do not return the folded dot-product claims, so the batched verifier is restated here (pcepb_verify).
Scalars are Python integers mod r; points are 64-byte canonical affine x || y.  A matrix is (rows, cols, vals) as in dense_model.
"""
import dense_model as dm
import oracle_lib as ol
import polyeval_model as pm
import product_proof_model as ppm
import transcript_model as tm
from transcript_model import R_MOD, Transcript  # noqa: F401

R = R_MOD
NAME = b"Sparse polynomial evaluation proof"
# the fields of the proof in declaration order, nested structs flattened (the layout of include/sbn254.h)
FIELDS = ("comm_derefs", "prod.eval_row", "prod.eval_col", "prod.eval_val", "prod.proof_mem", "prod.proof_ops",
          "hash.eval_row", "hash.eval_col", "hash.eval_val", "hash.eval_derefs", "hash.proof_ops", "hash.proof_mem", "hash.proof_derefs")


def log2(n):
    return n.bit_length() - 1


def npo2(n):
    return dm.next_power_of_two(n)


class Shape:
    """the sizes SparseMatPolyCommitmentGens::new derives (:619-627) and what follows from them"""

    def __init__(self, nx, ny, N, batch):
        assert 1 <= batch and N >= 2 and N & (N - 1) == 0 and max(nx, ny) >= 1
        self.nx, self.ny, self.N, self.b = nx, ny, N, batch
        self.n, self.m = log2(N), max(nx, ny)
        self.cells = 1 << self.m
        self.ell = {"ops": self.n + log2(npo2(5 * batch)), "mem": self.m + 1, "derefs": self.n + log2(npo2(2 * batch))}
        self.lg = {k: pm.factored_lens(v)[1] for k, v in self.ell.items()}
        self.Ld = 1 << pm.factored_lens(self.ell["derefs"])[0]

    def R(self, k):
        return 1 << self.lg[k]


def sizes(nx, ny, N, batch):
    """(scalars of rnd, bytes of the proof) — counted from the structure, not from the header's closed formula"""
    s = Shape(nx, ny, N, batch)
    b, n, m = s.b, s.n, s.m
    rnd = sum(3 + 2 * s.lg[k] for k in ("derefs", "ops", "mem"))
    pcepb = lambda c, l, d: 128 * sum(range(l)) + 32 * (2 * c * l + 3 * d)
    scalars = 2 * (2 + 2 * b) + 2 * b + 2 * (2 * b + 1) + b + 2 * b
    return rnd, 32 * s.Ld + 32 * scalars + pcepb(4, m, 0) + pcepb(4 * b, n, 2 * b) + sum(64 * s.lg[k] + 128 for k in ("ops", "mem", "derefs"))


def make_gens(xy_by_kind, shape):
    """{"ops" | "mem" | "derefs": the R_k + 2 points sbn_gens_new(R_k + 1, label) returns} -> {kind: (G, Q_base, h)}"""
    return {k: pm.split_gens(xy_by_kind[k], shape.R(k)) for k in ("ops", "mem", "derefs")}


def equalize(rx, ry):
    """:1681-1697: the shorter point gets zeros in front"""
    if len(rx) < len(ry):
        return [0] * (len(ry) - len(rx)) + list(rx), list(ry)
    if len(rx) > len(ry):
        return list(rx), [0] * (len(rx) - len(ry)) + list(ry)
    return list(rx), list(ry)


def true_evals(nx, ny, mats, rx, ry):
    """the evaluations the proof is about: M_k(rx, ry) = sum over the entries of val * eq(rx)[row] * eq(ry)[col]"""
    rx_ext, ry_ext = equalize(rx, ry)
    ex, ey = pm.eq_evals(rx_ext), pm.eq_evals(ry_ext)
    return [sum(v * ex[r] * ey[c] for r, c, v in zip(*mat)) % R for mat in mats]


def commit_dense(dense, gens, shape):
    """SparseMatPolyCommitment's two PolyCommitments (multi_sparse_to_dense_rep's caller, :176-193): what the verifier holds"""
    return (pm.commit_poly(gens["ops"], dense.comb_ops, None, shape.ell["ops"]), pm.commit_poly(gens["mem"], dense.comb_mem, None, shape.ell["mem"]))


def append_poly_commitment(tr, label, C):
    """PolyCommitment::append_to_transcript (hyrax.rs:44-51)"""
    tr.append_message(label, b"poly_commitment_begin")
    for c in C:
        pm.append_point(tr, b"poly_commitment_share", c)
    tr.append_message(label, b"poly_commitment_end")


def append_derefs_commitment(tr, C):
    """:341-347"""
    tr.append_message(b"derefs_commitment", b"begin_derefs_commitment")
    append_poly_commitment(tr, b"comm_poly_row_col_ops_val", C)
    tr.append_message(b"derefs_commitment", b"end_derefs_commitment")


def append_scalars(tr, label, xs):
    for x in xs:
        tr.append_scalar(label, x)


def hash_func(addr, val, ts, r_hash):
    return (ts * (r_hash * r_hash % R) + val * r_hash + addr) % R


def build_hash_layer(eval_table, addrs_vec, derefs_vec, read_ts_vec, audit_ts, r_hash, r_multiset):
    """:745-796 -> (init, [read], [write], audit)"""
    cells = len(eval_table)
    init = [(hash_func(i, eval_table[i], 0, r_hash) - r_multiset) % R for i in range(cells)]
    audit = [(hash_func(i, eval_table[i], audit_ts[i], r_hash) - r_multiset) % R for i in range(cells)]
    reads, writes = [], []
    for addrs, derefs, read_ts in zip(addrs_vec, derefs_vec, read_ts_vec):
        reads.append([(hash_func(a, v, t, r_hash) - r_multiset) % R for a, v, t in zip(addrs, derefs, read_ts)])
        writes.append([(hash_func(a, v, t + 1, r_hash) - r_multiset) % R for a, v, t in zip(addrs, derefs, read_ts)])
    return init, reads, writes, audit


def layers_new(eval_table, addrs_vec, read_ts_vec, audit_ts, ops_val, r_hash, r_multiset):
    """Layers::new (:798-840) -> {"init", "read", "write", "audit"} as product circuits"""
    init, reads, writes, audit = build_hash_layer(eval_table, addrs_vec, ops_val, read_ts_vec, audit_ts, r_hash, r_multiset)
    return {"init": ppm.product_circuit(init), "read": [ppm.product_circuit(p) for p in reads], "write": [ppm.product_circuit(p) for p in writes],
            "audit": ppm.product_circuit(audit)}


def bound_bot(evals, ch):
    pe = list(evals)
    for i in range(len(ch) - 1, -1, -1):                   # bound_poly_var_bot from the last challenge down (hyrax.rs:206-214)
        pe = [(pe[2 * k] + ch[i] * (pe[2 * k + 1] - pe[2 * k])) % R for k in range(len(pe) // 2)]
    assert len(pe) == 1
    return pe[0]


def pad(evals):
    return list(evals) + [0] * (npo2(len(evals)) - len(evals))


OPS_LABELS = (b"claim_evals_ops", b"challenge_combine_n_to_one", b"joint_claim_eval_ops")
MEM_LABELS = (b"claim_evals_mem", b"challenge_combine_two_to_one", b"joint_claim_eval_mem")
DEREFS_LABELS = (b"evals_ops_val", b"challenge_combine_n_to_one", b"joint_claim_eval")


# ---- the prover ----------------------------------------------------------------------------------------------------------------

def product_layer_prove(tr, row, col, dense, row_ops_val, col_ops_val, evals):
    """ProductLayerProof::prove (:1306-1428) -> (proof part, rand_mem, rand_ops)"""
    tr.append_message(b"protocol-name", b"Sparse polynomial product layer proof")
    out = {}
    for name, lay in (("row", row), ("col", col)):
        e_init, e_audit = ppm.circuit_evaluate(lay["init"]), ppm.circuit_evaluate(lay["audit"])
        e_read = [ppm.circuit_evaluate(c) for c in lay["read"]]
        e_write = [ppm.circuit_evaluate(c) for c in lay["write"]]
        assert e_init * dm.product(e_write) % R == dm.product(e_read) * e_audit % R            # :1324, :1339
        tr.append_scalar(b"claim_%s_eval_init" % name.encode(), e_init)
        append_scalars(tr, b"claim_%s_eval_read" % name.encode(), e_read)
        append_scalars(tr, b"claim_%s_eval_write" % name.encode(), e_write)
        tr.append_scalar(b"claim_%s_eval_audit" % name.encode(), e_audit)
        out["eval_" + name] = (e_init, e_read, e_write, e_audit)
    assert len(evals) == len(row_ops_val)
    dotps, lefts, rights = [], [], []
    for i in range(len(row_ops_val)):
        left, right, weights = row_ops_val[i], col_ops_val[i], dense.val[i]
        idx = len(left) // 2
        assert idx * 2 == len(left)                                                            # DotProductCircuit::split, product_tree.rs:87-105
        d_left, d_right = (left[:idx], right[:idx], weights[:idx]), (left[idx:], right[idx:], weights[idx:])
        e_left, e_right = ppm.dotp_evaluate(d_left), ppm.dotp_evaluate(d_right)
        tr.append_scalar(b"claim_eval_dotp_left", e_left)
        tr.append_scalar(b"claim_eval_dotp_right", e_right)
        assert (e_left + e_right) % R == evals[i] % R, "eval_dotp_left + eval_dotp_right != evals[%d]  (:1366)" % i
        lefts.append(e_left); rights.append(e_right)
        dotps += [d_left, d_right]
    out["eval_val"] = (lefts, rights)
    ops_circuits = row["read"] + row["write"] + col["read"] + col["write"]
    proof_ops = ppm.prove(tr, ops_circuits, dotps)
    proof_mem = ppm.prove(tr, [row["init"], row["audit"], col["init"], col["audit"]], [])
    out["proof_mem"], out["proof_ops"] = _strip(proof_mem), _strip(proof_ops)
    return out, proof_mem["rand"], proof_ops["rand"]


def _strip(p):
    """what a ProductCircuitEvalProofBatched holds: the polynomials and the claims, not the prover's rand / claims_to_verify"""
    return {"polys": p["polys"], "claims": p["claims"], "claims_dotp": p["claims_dotp"]}


def hash_layer_prove(tr, rand_mem, rand_ops, dense, row_ops_val, col_ops_val, derefs_comb, gens, rnd, shape):
    """HashLayerProof::prove (:922-1046); rnd = {"derefs" | "ops" | "mem": the opening's draws}"""
    tr.append_message(b"protocol-name", b"Sparse polynomial hash layer proof")
    ev = lambda z, r: ppm.evaluate_mle(z, r)
    e_row_val = [ev(p, rand_ops) for p in row_ops_val]
    e_col_val = [ev(p, rand_ops) for p in col_ops_val]
    # DerefsEvalProof::prove (:412-432)
    tr.append_message(b"protocol-name", b"Derefs evaluation proof")
    _, _, proof_derefs, _, _ = pm.prove_single(tr, gens["derefs"], derefs_comb, rand_ops, pad(e_row_val + e_col_val), rnd["derefs"], DEREFS_LABELS)
    sides = []
    for side in (0, 1):                                                                          # prove_helper (:901-920)
        sides.append(([ev([a % R for a in p], rand_ops) for p in dense.addr[side]], [ev(p, rand_ops) for p in dense.read_ts[side]],
                      ev(dense.audit_ts[side], rand_mem)))
    e_val = [ev(v, rand_ops) for v in dense.val]
    evals_ops = pad(sides[0][0] + sides[0][1] + sides[1][0] + sides[1][1] + e_val)
    _, _, proof_ops, _, _ = pm.prove_single(tr, gens["ops"], dense.comb_ops, rand_ops, evals_ops, rnd["ops"], OPS_LABELS)
    _, _, proof_mem, _, _ = pm.prove_single(tr, gens["mem"], dense.comb_mem, rand_mem, [sides[0][2], sides[1][2]], rnd["mem"], MEM_LABELS)
    return {"eval_row": sides[0], "eval_col": sides[1], "eval_val": e_val, "eval_derefs": (e_row_val, e_col_val),
            "proof_ops": proof_ops, "proof_mem": proof_mem, "proof_derefs": proof_derefs}


def split_rnd(rnd, shape):
    out, o = {}, 0
    for k in ("derefs", "ops", "mem"):                                                           # the order HashLayerProof::prove opens in
        n = 3 + 2 * shape.lg[k]
        out[k] = list(rnd[o:o + n]); o += n
    assert o == len(rnd)
    return out


def prove(tr, nx, ny, mats, rx, ry, evals, gens, rnd):
    """SparseMatPolyEvalProof::prove (:1700-1755).  `tr` moves on.  Raises AssertionError where the reference asserts."""
    dense = dm.Dense(nx, ny, mats)
    shape = Shape(nx, ny, dense.N, dense.batch)
    assert len(rx) == nx and len(ry) == ny
    tr.append_message(b"protocol-name", NAME)
    assert len(evals) == dense.batch                                                             # :1711
    rx_ext, ry_ext = equalize(rx, ry)
    mem_rx, mem_ry = pm.eq_evals(rx_ext), pm.eq_evals(ry_ext)
    row_ops_val = [dm.deref(a, mem_rx) for a in dense.addr[0]]                                   # dense.deref (:275-279)
    col_ops_val = [dm.deref(a, mem_ry) for a in dense.addr[1]]
    comb = dm.merge(row_ops_val + col_ops_val)                                                   # Derefs::new (:293-297)
    comm_derefs = pm.commit_poly(gens["derefs"], comb, None, shape.ell["derefs"])                # Derefs::commit (:301-304)
    assert len(comm_derefs) == shape.Ld
    append_derefs_commitment(tr, comm_derefs)
    r_hash, r_multiset = tr.challenge_scalar(b"challenge_r_hash"), tr.challenge_scalar(b"challenge_r_hash")
    row = layers_new(mem_rx, dense.addr[0], dense.read_ts[0], dense.audit_ts[0], row_ops_val, r_hash, r_multiset)      # PolyEvalNetwork::new (:853-866)
    col = layers_new(mem_ry, dense.addr[1], dense.read_ts[1], dense.audit_ts[1], col_ops_val, r_hash, r_multiset)
    tr.append_message(b"protocol-name", NAME)                                                    # PolyEvalNetworkProof::prove (:1555)
    prod, rand_mem, rand_ops = product_layer_prove(tr, row, col, dense, row_ops_val, col_ops_val, evals)
    hashp = hash_layer_prove(tr, rand_mem, rand_ops, dense, row_ops_val, col_ops_val, comb, gens, split_rnd(rnd, shape), shape)
    return {"comm_derefs": comm_derefs, "prod": prod, "hash": hashp}


# ---- the verifier --------------------------------------------------------------------------------------------------------------

def pcepb_verify(tr, proof, claims_prod_vec, claims_dotp_vec, length):
    """ProductCircuitEvalProofBatched::verify (product_tree.rs:394-537) -> (claims_to_verify, claims_to_verify_dotp, rand), or None where
    the reference panics (an assert or the sumcheck verifier's unwrap)"""
    num_layers = log2(length)
    n = len(claims_prod_vec)
    if len(proof["polys"]) != num_layers or len(proof["claims"]) != num_layers:
        return None
    rand, claims_to_verify, claims_dotp_out = [], list(claims_prod_vec), []
    for i in range(num_layers):
        last = i == num_layers - 1
        if last:
            claims_to_verify = claims_to_verify + list(claims_dotp_vec)
        coeffs = [tr.challenge_scalar(b"rand_coeffs_next_layer") for _ in claims_to_verify]
        e = sum(a * b for a, b in zip(claims_to_verify, coeffs)) % R
        if len(proof["polys"][i]) != i:
            return None
        rand_prod = []
        for co in proof["polys"][i]:                                                             # SumcheckInstanceProof::verify (sumcheck.rs:35-85), degree 3
            if len(co) != 4 or (2 * co[0] + co[1] + co[2] + co[3] - e) % R:
                return None
            tr.append_message(b"poly", b"UniPoly_begin")
            append_scalars(tr, b"coeff", co)
            tr.append_message(b"poly", b"UniPoly_end")
            r = tr.challenge_scalar(b"challenge_nextround")
            rand_prod.append(r)
            e = tm.unipoly_eval(co, r)
        lefts, rights = proof["claims"][i]
        if len(lefts) != n or len(rights) != n:
            return None
        for a, b in zip(lefts, rights):
            tr.append_scalar(b"claim_prod_left", a); tr.append_scalar(b"claim_prod_right", b)
        eq = 1
        for x, y in zip(rand, rand_prod):
            eq = eq * (x * y + (1 - x) * (1 - y)) % R
        expected = sum(c * a * b * eq for c, a, b in zip(coeffs, lefts, rights)) % R
        dl, dr, dw = proof["claims_dotp"]
        if last:
            if not (len(dl) == len(dr) == len(dw) == len(claims_dotp_vec)):
                return None
            for k in range(len(dl)):
                tr.append_scalar(b"claim_dotp_left", dl[k]); tr.append_scalar(b"claim_dotp_right", dr[k]); tr.append_scalar(b"claim_dotp_weight", dw[k])
                expected = (expected + coeffs[n + k] * dl[k] * dr[k] * dw[k]) % R
        if expected != e:
            return None
        r_layer = tr.challenge_scalar(b"challenge_r_layer")
        claims_to_verify = [(a + r_layer * (b - a)) % R for a, b in zip(lefts, rights)]
        if last:
            for k in range(len(claims_dotp_vec) // 2):                                           # :516-530
                for v in (dl, dr, dw):
                    claims_dotp_out.append((v[2 * k] + r_layer * (v[2 * k + 1] - v[2 * k])) % R)
        rand = [r_layer] + rand_prod
    return claims_to_verify, claims_dotp_out, rand


def product_layer_verify(tr, prod, num_ops, num_mem_cells, evals):
    """ProductLayerProof::verify (:1436-1520) -> (claims_mem, rand_mem, claims_ops, claims_dotp, rand_ops) or None"""
    tr.append_message(b"protocol-name", b"Sparse polynomial product layer proof")
    b = len(evals)
    for name in ("row", "col"):
        e_init, e_read, e_write, e_audit = prod["eval_" + name]
        if len(e_read) != b or len(e_write) != b:
            return None
        if e_init * dm.product(e_write) % R != dm.product(e_read) * e_audit % R:
            return None
        tr.append_scalar(b"claim_%s_eval_init" % name.encode(), e_init)
        append_scalars(tr, b"claim_%s_eval_read" % name.encode(), e_read)
        append_scalars(tr, b"claim_%s_eval_write" % name.encode(), e_write)
        tr.append_scalar(b"claim_%s_eval_audit" % name.encode(), e_audit)
    lefts, rights = prod["eval_val"]
    claims_dotp_circuit = []
    for i in range(b):
        if (lefts[i] + rights[i]) % R != evals[i] % R:
            return None
        tr.append_scalar(b"claim_eval_dotp_left", lefts[i]); tr.append_scalar(b"claim_eval_dotp_right", rights[i])
        claims_dotp_circuit += [lefts[i], rights[i]]
    row, col = prod["eval_row"], prod["eval_col"]
    got = pcepb_verify(tr, prod["proof_ops"], row[1] + row[2] + col[1] + col[2], claims_dotp_circuit, num_ops)
    if got is None:
        return None
    claims_ops, claims_dotp, rand_ops = got
    got = pcepb_verify(tr, prod["proof_mem"], [row[0], row[3], col[0], col[3]], [], num_mem_cells)
    if got is None:
        return None
    claims_mem, _, rand_mem = got
    return claims_mem, rand_mem, claims_ops, claims_dotp, rand_ops


def identity_evaluate(r):
    """IdentityPolynomial::evaluate (:1278-1285)"""
    out = 0
    for x in r:
        out = (out * 2 + x) % R
    return out


def eq_evaluate(r, x):
    """EqPolynomial::evaluate"""
    out = 1
    for a, b in zip(r, x):
        out = out * (a * b + (1 - a) * (1 - b)) % R
    return out


def verify_helper(rand_mem, claims, e_ops_val, e_ops_addr, e_read_ts, e_audit_ts, r, r_hash, r_multiset):
    """:1048-1112"""
    claim_init, claim_read, claim_write, claim_audit = claims
    e_init_addr, e_init_val = identity_evaluate(rand_mem), eq_evaluate(r, rand_mem)
    if claim_init != (hash_func(e_init_addr, e_init_val, 0, r_hash) - r_multiset) % R:
        return False
    if claim_audit != (hash_func(e_init_addr, e_init_val, e_audit_ts, r_hash) - r_multiset) % R:
        return False
    for i in range(len(e_ops_val)):
        if claim_read[i] != (hash_func(e_ops_addr[i], e_ops_val[i], e_read_ts[i], r_hash) - r_multiset) % R:
            return False
        if claim_write[i] != (hash_func(e_ops_addr[i], e_ops_val[i], e_read_ts[i] + 1, r_hash) - r_multiset) % R:
            return False
    return True


def joint_verify(tr, proof, gens, r, evals, comm_C, labels):
    """DerefsEvalProof::verify_single (:434-457) and its two siblings in HashLayerProof::verify (:1215-1262)"""
    le, lch, lcl = labels
    append_scalars(tr, le, evals)
    ch = [tr.challenge_scalar(lch) for _ in range(log2(len(evals)))]
    claim = bound_bot(evals, ch)
    tr.append_scalar(lcl, claim)
    return pm.verify_plain(tr, proof, gens, ch + list(r), claim, comm_C)


def hash_layer_verify(tr, hp, rand_mem, rand_ops, claims_row, claims_col, claims_dotp, comm, comm_derefs, gens, rx, ry, r_hash, r_multiset):
    """HashLayerProof::verify (:1114-1265)"""
    tr.append_message(b"protocol-name", b"Sparse polynomial hash layer proof")
    e_row_val, e_col_val = hp["eval_derefs"]
    tr.append_message(b"protocol-name", b"Derefs evaluation proof")                              # DerefsEvalProof::verify (:459-481)
    if not joint_verify(tr, hp["proof_derefs"], gens["derefs"], rand_ops, pad(list(e_row_val) + list(e_col_val)), comm_derefs, DEREFS_LABELS):
        return False
    row_addr, row_read_ts, row_audit = hp["eval_row"]
    col_addr, col_read_ts, col_audit = hp["eval_col"]
    if not verify_helper(rand_mem, claims_row, e_row_val, row_addr, row_read_ts, row_audit, rx, r_hash, r_multiset):
        return False
    if not verify_helper(rand_mem, claims_col, e_col_val, col_addr, col_read_ts, col_audit, ry, r_hash, r_multiset):
        return False
    b = len(e_row_val)
    if len(claims_dotp) != 3 * b:
        return False
    for i in range(b):
        if claims_dotp[3 * i] != e_row_val[i] or claims_dotp[3 * i + 1] != e_col_val[i] or claims_dotp[3 * i + 2] != hp["eval_val"][i]:
            return False
    evals_ops = pad(list(row_addr) + list(row_read_ts) + list(col_addr) + list(col_read_ts) + list(hp["eval_val"]))
    if not joint_verify(tr, hp["proof_ops"], gens["ops"], rand_ops, evals_ops, comm[0], OPS_LABELS):
        return False
    return joint_verify(tr, hp["proof_mem"], gens["mem"], rand_mem, [row_audit, col_audit], comm[1], MEM_LABELS)


def verify(tr, proof, comm, num_ops, num_mem_cells, rx, ry, evals, gens):
    """SparseMatPolyEvalProof::verify (:1815-1845) with PolyEvalNetworkProof::verify (:1581-1650) -> bool.  comm = commit_dense(...)"""
    tr.append_message(b"protocol-name", NAME)
    rx_ext, ry_ext = equalize(rx, ry)
    assert 1 << len(rx_ext) == num_mem_cells                                                     # :1828
    append_derefs_commitment(tr, proof["comm_derefs"])
    r_hash, r_multiset = tr.challenge_scalar(b"challenge_r_hash"), tr.challenge_scalar(b"challenge_r_hash")
    tr.append_message(b"protocol-name", NAME)
    b = len(evals)
    got = product_layer_verify(tr, proof["prod"], num_ops, num_mem_cells, evals)
    if got is None:
        return False
    claims_mem, rand_mem, claims_ops, claims_dotp, rand_ops = got
    if len(claims_mem) != 4 or len(claims_ops) != 4 * b:
        return False
    claims_row = (claims_mem[0], claims_ops[:b], claims_ops[b:2 * b], claims_mem[1])
    claims_col = (claims_mem[2], claims_ops[2 * b:3 * b], claims_ops[3 * b:], claims_mem[3])
    return hash_layer_verify(tr, proof["hash"], rand_mem, rand_ops, claims_row, claims_col, claims_dotp, comm, proof["comm_derefs"], gens,
                             rx_ext, ry_ext, r_hash, r_multiset)


# ---- the proof as bytes, in the layout of include/sbn254.h --------------------------------------------------------------------

def _sbs(xs):
    return b"".join(pm.sb(x) for x in xs)


def _pcepb_bytes(p):
    polys, claims, _, _ = ppm.proof_to_flat(dict(p, rand=[], claims_final=[]))
    return polys + claims


def field_bytes(proof):
    """{field: bytes} in FIELDS order"""
    pr, hp = proof["prod"], proof["hash"]
    four = lambda t: _sbs([t[0]] + list(t[1]) + list(t[2]) + [t[3]])
    three = lambda t: _sbs(list(t[0]) + list(t[1]) + [t[2]])
    return {
        "comm_derefs": b"".join(ol.g1_compress(c) for c in proof["comm_derefs"]),
        "prod.eval_row": four(pr["eval_row"]), "prod.eval_col": four(pr["eval_col"]), "prod.eval_val": _sbs(list(pr["eval_val"][0]) + list(pr["eval_val"][1])),
        "prod.proof_mem": _pcepb_bytes(pr["proof_mem"]), "prod.proof_ops": _pcepb_bytes(pr["proof_ops"]),
        "hash.eval_row": three(hp["eval_row"]), "hash.eval_col": three(hp["eval_col"]), "hash.eval_val": _sbs(hp["eval_val"]),
        "hash.eval_derefs": _sbs(list(hp["eval_derefs"][0]) + list(hp["eval_derefs"][1])),
        "hash.proof_ops": pm.proof_bytes(hp["proof_ops"]), "hash.proof_mem": pm.proof_bytes(hp["proof_mem"]), "hash.proof_derefs": pm.proof_bytes(hp["proof_derefs"]),
    }


def proof_bytes(proof):
    fb = field_bytes(proof)
    return b"".join(fb[f] for f in FIELDS)


def field_lengths(shape):
    b, n, m = shape.b, shape.n, shape.m
    pcepb = lambda c, l, d: 128 * sum(range(l)) + 32 * (2 * c * l + 3 * d)
    return {"comm_derefs": 32 * shape.Ld, "prod.eval_row": 32 * (2 + 2 * b), "prod.eval_col": 32 * (2 + 2 * b), "prod.eval_val": 64 * b,
            "prod.proof_mem": pcepb(4, m, 0), "prod.proof_ops": pcepb(4 * b, n, 2 * b), "hash.eval_row": 32 * (2 * b + 1), "hash.eval_col": 32 * (2 * b + 1),
            "hash.eval_val": 32 * b, "hash.eval_derefs": 64 * b, "hash.proof_ops": 64 * shape.lg["ops"] + 128, "hash.proof_mem": 64 * shape.lg["mem"] + 128,
            "hash.proof_derefs": 64 * shape.lg["derefs"] + 128}


def field_spans(shape):
    out, o = {}, 0
    fl = field_lengths(shape)
    for f in FIELDS:
        out[f] = (o, o + fl[f]); o += fl[f]
    return out


def _ints(b):
    return [int.from_bytes(b[32 * i:32 * i + 32], "little") for i in range(len(b) // 32)]


def proof_from_bytes(data, shape):
    """-> proof dict, or None when a point does not decompress (the reference's deserialisation fails)"""
    b, n, m = shape.b, shape.n, shape.m
    sp = field_spans(shape)
    assert len(data) == sp[FIELDS[-1]][1]
    f = {k: data[lo:hi] for k, (lo, hi) in sp.items()}
    comm = [ol.g1_decompress(f["comm_derefs"][32 * i:32 * i + 32]) for i in range(shape.Ld)]
    opens = {k: pm.proof_from_bytes(f[k]) for k in ("hash.proof_ops", "hash.proof_mem", "hash.proof_derefs")}
    if any(c is None for c in comm) or any(v is None for v in opens.values()):
        return None

    def four(x):
        v = _ints(x)
        return (v[0], v[1:1 + b], v[1 + b:1 + 2 * b], v[1 + 2 * b])

    def three(x):
        v = _ints(x)
        return (v[:b], v[b:2 * b], v[2 * b])

    def pcepb(x, c, l, d):
        npoly = 128 * sum(range(l))
        return _strip(ppm.proof_from_flat(x[:npoly], x[npoly:], b"", b"", c, d, l))
    ev, ed = _ints(f["prod.eval_val"]), _ints(f["hash.eval_derefs"])
    return {"comm_derefs": comm,
            "prod": {"eval_row": four(f["prod.eval_row"]), "eval_col": four(f["prod.eval_col"]), "eval_val": (ev[:b], ev[b:]),
                     "proof_mem": pcepb(f["prod.proof_mem"], 4, m, 0), "proof_ops": pcepb(f["prod.proof_ops"], 4 * b, n, 2 * b)},
            "hash": {"eval_row": three(f["hash.eval_row"]), "eval_col": three(f["hash.eval_col"]), "eval_val": _ints(f["hash.eval_val"]),
                     "eval_derefs": (ed[:b], ed[b:]), "proof_ops": opens["hash.proof_ops"], "proof_mem": opens["hash.proof_mem"],
                     "proof_derefs": opens["hash.proof_derefs"]}}


# ---- instances for the tests ---------------------------------------------------------------------------------------------------

# (nx, ny, nnz per matrix).  (1,1,[2,2,2]): N = 2, one-layer ops circuits, one-entry dot-product halves, cells = 2.  (2,3,[3,4,1]): rx shorter than
# ry, ragged padding, N = 4, one all-padding row of the derefs matrix (an identity in comm_derefs).  (3,2,[5,0,8]): rx longer than ry, an empty matrix.
# (3,3,[8,8,8]): repeated addresses and zero values.  Then batch 1, 2 and 4 (24 instances in proof_ops: the cap).
SHAPES = [(1, 1, (2, 2, 2)), (2, 3, (3, 4, 1)), (3, 2, (5, 0, 8)), (3, 3, (8, 8, 8)), (2, 2, (4,)), (2, 2, (3, 4)), (2, 2, (4, 4, 4, 4))]


def instance(shape_key, seed=0):
    """(mats, rx, ry, evals, rnd) of a shape, the evaluations true"""
    nx, ny, nnz = shape_key
    special = shape_key == (3, 3, (8, 8, 8))
    mats = random_mats(nx, ny, nnz, 100 + seed + 8 * nx + ny + len(nnz), repeat=special, zero_vals=special)
    rx, ry = random_scalars(nx, 200 + seed + nx), random_scalars(ny, 300 + seed + ny)
    rnd = random_scalars(sizes(nx, ny, dm.num_ops(mats), len(nnz))[0], 400 + seed)
    return mats, rx, ry, true_evals(nx, ny, mats, rx, ry), rnd


def random_mats(nx, ny, nnz, seed, repeat=False, zero_vals=False):
    """one (rows, cols, vals) per entry of nnz; repeat: addresses drawn from two cells only; zero_vals: every third value is 0"""
    import random
    rng = random.Random(seed)
    cells_r, cells_c = (2, 2) if repeat else (1 << nx, 1 << ny)
    mats = []
    for k in nnz:
        rows = [rng.randrange(cells_r) for _ in range(k)]
        cols = [rng.randrange(cells_c) for _ in range(k)]
        vals = [0 if zero_vals and i % 3 == 0 else rng.randrange(R) for i in range(k)]
        mats.append((rows, cols, vals))
    return mats


def random_scalars(n, seed):
    import random
    rng = random.Random(seed)
    return [rng.randrange(R) for _ in range(n)]
