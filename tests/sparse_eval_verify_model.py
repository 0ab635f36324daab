"""The literal verdict of SparseMatPolyEvalProof::verify on BYTES, and the field half of the verifier cut out of tests/sparse_eval_model.py
for comparison with csrc/sparse_verify_host.hpp.

    verify_bytes      the canonical check of every scalar (Scalar::from_bytes fails on a value >= r, scalar.rs:87-95), then
                      sparse_eval_model.proof_from_bytes (a point that does not decompress), then sparse_eval_model.verify
    field_half        what the host header computes: the transcript up to the product layer, ProductLayerProof::verify, and the field part of
                      HashLayerProof::verify with the padded evaluation vectors of the three joint openings
"""
import sparse_eval_model as sem
from sparse_eval_model import R

SCALAR_FIELDS = sem.FIELDS[1:10]
OPENINGS = sem.FIELDS[10:]


def scalars_canonical(data, shape):
    sp = sem.field_spans(shape)
    spans = [sp[f] for f in SCALAR_FIELDS] + [(sp[f][1] - 64, sp[f][1]) for f in OPENINGS]
    return all(int.from_bytes(data[o:o + 32], "little") < R for lo, hi in spans for o in range(lo, hi, 32))


def verify_bytes(tr, data, shape, comm, rx, ry, evals, gens):
    """-> bool; `tr` moves as the literal verifier moves it (a caller that needs it untouched on a refusal passes a copy)"""
    if not scalars_canonical(data, shape):
        return False
    proof = sem.proof_from_bytes(data, shape)
    if proof is None:
        return False
    return sem.verify(tr, proof, comm, shape.N, shape.cells, rx, ry, evals, gens)


def begin(tr, comm_derefs):
    """SparseMatPolyEvalProof::verify up to and with PolyEvalNetworkProof::verify's protocol name, as sparse_eval_model.verify writes it -> (r_hash, r_multiset)"""
    tr.append_message(b"protocol-name", sem.NAME)
    sem.append_derefs_commitment(tr, comm_derefs)
    r_hash, r_multiset = tr.challenge_scalar(b"challenge_r_hash"), tr.challenge_scalar(b"challenge_r_hash")
    tr.append_message(b"protocol-name", sem.NAME)
    return r_hash, r_multiset


def hash_layer_field(hp, b, rand_mem, claims_mem, claims_ops, claims_dotp, rx_ext, ry_ext, r_hash, r_multiset):
    """the field part of HashLayerProof::verify (sparse_eval_model.hash_layer_verify without its three openings) ->
    (evals_derefs, evals_ops, evals_mem), padded, or None"""
    if len(claims_mem) != 4 or len(claims_ops) != 4 * b:
        return None
    claims_row = (claims_mem[0], claims_ops[:b], claims_ops[b:2 * b], claims_mem[1])
    claims_col = (claims_mem[2], claims_ops[2 * b:3 * b], claims_ops[3 * b:], claims_mem[3])
    e_row_val, e_col_val = hp["eval_derefs"]
    row_addr, row_read_ts, row_audit = hp["eval_row"]
    col_addr, col_read_ts, col_audit = hp["eval_col"]
    if not sem.verify_helper(rand_mem, claims_row, e_row_val, row_addr, row_read_ts, row_audit, rx_ext, r_hash, r_multiset):
        return None
    if not sem.verify_helper(rand_mem, claims_col, e_col_val, col_addr, col_read_ts, col_audit, ry_ext, r_hash, r_multiset):
        return None
    if len(claims_dotp) != 3 * b:
        return None
    for i in range(b):
        if claims_dotp[3 * i] != e_row_val[i] or claims_dotp[3 * i + 1] != e_col_val[i] or claims_dotp[3 * i + 2] != hp["eval_val"][i]:
            return None
    return (sem.pad(list(e_row_val) + list(e_col_val)),
            sem.pad(list(row_addr) + list(row_read_ts) + list(col_addr) + list(col_read_ts) + list(hp["eval_val"])), [row_audit, col_audit])
