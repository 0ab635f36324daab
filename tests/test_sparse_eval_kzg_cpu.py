"""CPU: tests/sparse_eval_kzg_model.py — the literal restatement of the KZG build's SparseMatPolyEvalProof::prove / ::verify
(sparse_mlpoly_full.rs:1757-1845 with DerefsEvalProof :503-595 and kzg.rs:174-217) that sbn_sparse_eval_prove_kzg is checked against — the
host-only sbn_sparse_eval_kzg_sizes, and the two identities the device path rests on: the commitment as a sum over memory cells, and the
division stopped at the non-zero prefix."""
import random

import pytest

import dense_model as dm
import kzg_model as km
import sparse_eval_kzg_model as skm
import sparse_eval_model as sem
from sparse_eval_model import R, Transcript

SHAPES = sem.SHAPES
LABEL = b"gens_sparse_eval_kzg_cpu"
TR_LABEL = b"sparse eval kzg cpu"
TAU = random.Random(2025).randrange(1, R)
_CACHE = {}


def model_gens(ol, shape, label=LABEL):
    key = ("gens", label, shape.lg["ops"], shape.lg["mem"])
    if key not in _CACHE:
        _CACHE[key] = {k: sem.pm.split_gens(ol.gens_new(shape.R(k) + 1, label + b"_" + k.encode())[0], shape.R(k)) for k in skm.KINDS}
    return _CACHE[key]


def _proved(ol, shape_key):
    """one honest proof per shape for the whole module; the SRS has the reference's size, n_d + 1"""
    if shape_key not in _CACHE:
        nx, ny, nnz = shape_key
        mats, rx, ry, evals, rnd = skm.instance(shape_key)
        dense = dm.Dense(nx, ny, mats)
        shape = sem.Shape(nx, ny, dense.N, dense.batch)
        gens = model_gens(ol, shape)
        srs = skm.Srs(TAU, (1 << shape.ell["derefs"]) + 1)
        tr = Transcript(TR_LABEL)
        proof = skm.prove(tr, nx, ny, mats, rx, ry, evals, gens, srs, rnd)
        comm = (sem.pm.commit_poly(gens["ops"], dense.comb_ops, None, shape.ell["ops"]), sem.pm.commit_poly(gens["mem"], dense.comb_mem, None, shape.ell["mem"]))
        _CACHE[shape_key] = (mats, rx, ry, evals, dense, shape, gens, srs, proof, tr.state(), comm)
    return _CACHE[shape_key]


@pytest.mark.parametrize("shape_key", SHAPES)
def test_prove_then_verify_accepts_and_ends_in_the_same_state(ol, shape_key):
    nx, ny, nnz = shape_key
    mats, rx, ry, evals, dense, shape, gens, srs, proof, state, comm = _proved(ol, shape_key)
    tv = Transcript(TR_LABEL)
    assert skm.verify(tv, proof, comm, dense.N, dense.cells, rx, ry, evals, gens, srs)
    assert tv.state() == state
    b = skm.proof_bytes(proof)
    assert len(b) == skm.sizes(nx, ny, dense.N, dense.batch)[1]
    back = skm.proof_from_bytes(b, shape)
    assert skm.proof_bytes(back) == b
    tv = Transcript(TR_LABEL)
    assert skm.verify(tv, back, comm, dense.N, dense.cells, rx, ry, evals, gens, srs) and tv.state() == state


@pytest.mark.parametrize("field", skm.FIELDS)
def test_verifier_rejects_a_flipped_byte_in_each_field(ol, field):
    shape_key = (2, 3, (3, 4, 1))
    mats, rx, ry, evals, dense, shape, gens, srs, proof, _, comm = _proved(ol, shape_key)
    b = bytearray(skm.proof_bytes(proof))
    lo, hi = skm.field_spans(shape)[field]
    b[hi - 32] ^= 1                                      # the lowest byte of the field's last element, an x coordinate or a scalar
    bad = skm.proof_from_bytes(bytes(b), shape)
    assert bad is None or not skm.verify(Transcript(TR_LABEL), bad, comm, dense.N, dense.cells, rx, ry, evals, gens, srs)
    if field == "hash.proof_derefs":                     # its other element: the opening proof pi
        b = bytearray(skm.proof_bytes(proof)); b[lo] ^= 1
        bad = skm.proof_from_bytes(bytes(b), shape)
        assert bad is None or not skm.verify(Transcript(TR_LABEL), bad, comm, dense.N, dense.cells, rx, ry, evals, gens, srs)


def test_sizes_against_the_models_counts(sbn):
    for nx, ny, nnz in SHAPES:
        N = max(dm.next_power_of_two(k) for k in nnz)
        assert sbn.sparse_eval_kzg_sizes(nx, ny, N, len(nnz)) == skm.sizes(nx, ny, N, len(nnz)), (nx, ny, nnz)
    for nx, ny, N, b in ((10, 10, 1 << 10, 3), (13, 13, 1 << 13, 3), (10, 10, 1 << 14, 1), (21, 21, 1 << 22, 3), (5, 20, 2, 1), (20, 5, 1 << 20, 4)):
        assert sbn.sparse_eval_kzg_sizes(nx, ny, N, b) == skm.sizes(nx, ny, N, b), (nx, ny, N, b)
    # the keyless shape by the header's closed formula: ell_ops = 26 -> lg 13; ell_mem = 22 -> lg 11
    assert sbn.sparse_eval_kzg_sizes(21, 21, 1 << 22, 3) == (6 + 2 * 24, 32 * 45 + 64 * (21 * 20 + 22 * 21) + 256 * (21 + 66) + 576 + 64 * 24 + 352)


@pytest.mark.parametrize("args", [(2, 2, 4, 0), (2, 2, 4, 5), (2, 2, 1, 3), (2, 2, 6, 3), (0, 0, 4, 3)])
def test_sizes_refuses(sbn, args):
    import ctypes as C
    a, b = C.c_size_t(7), C.c_size_t(7)
    assert sbn.lib().sbn_sparse_eval_kzg_sizes(*[C.c_size_t(x) for x in args], C.byref(a), C.byref(b)) == -1          # SBN_EINVAL
    assert (a.value, b.value) == (7, 7)
    with pytest.raises(sbn.SbnError):
        sbn.sparse_eval_kzg_sizes(*args)


@pytest.mark.parametrize("shape_key", SHAPES)
def test_key_identity_sum_over_cells_equals_commit_of_the_merged_derefs(shape_key):
    """sum_a eq[a] S_a == commit(merged derefs), on integers mod r with [tau^i] as scalars"""
    nx, ny, nnz = shape_key
    mats, rx, ry, _, _ = skm.instance(shape_key)
    dense = dm.Dense(nx, ny, mats)
    mem_rx, mem_ry, _, _, comb = skm.derefs_comb(dense, rx, ry)
    srs = skm.Srs(TAU, len(comb) + 1)
    assert skm.key_commit_scalar(dense, srs, mem_rx, mem_ry) == srs.commit_scalar(comb)
    ks = skm.key_scalars(dense, srs)
    for side in (0, 1):                                  # the key holds exactly the cells read at least once
        assert sorted(a for s, a in ks if s == side) == [a for a in range(dense.cells) if dense.audit_ts[side][a] > 0]
    # the padding behind n' = 2 b N is zero: the commitment of the prefix is the commitment
    assert comb[2 * dense.batch * dense.N:] == [0] * (len(comb) - 2 * dense.batch * dense.N)
    assert km.evaluate_poly(comb[:2 * dense.batch * dense.N], TAU) == srs.commit_scalar(comb)


@pytest.mark.parametrize("N", [4, 64])
def test_the_trim_quotient_of_the_prefix_padded_is_the_quotient(N):
    """b = 3: 6 of 8 blocks are real; the quotient's coefficients from n' - 1 on are zero and the evaluation is the prefix's"""
    rng = random.Random(N)
    n_prefix, n_d = 6 * N, 8 * N
    p = [rng.randrange(R) for _ in range(n_prefix)] + [0] * (n_d - n_prefix)
    z = rng.randrange(R)
    y = km.evaluate_poly(p, z)
    assert km.evaluate_poly(p[:n_prefix], z) == y
    q_full, q_trim = km.compute_quotient(p, z, y), km.compute_quotient(p[:n_prefix], z, y)
    assert len(q_full) == n_d - 1 and len(q_trim) == n_prefix - 1
    assert q_trim + [0] * (n_d - n_prefix) == q_full
    assert km.evaluate_poly(q_trim, TAU) == km.evaluate_poly(q_full, TAU)
