"""CPU: tests/sparse_eval_model.py — the literal restatement of SparseMatPolyEvalProof::prove / ::verify (sparse_mlpoly_full.rs:1700-1845) that
sbn_sparse_eval_prove is checked against — and the host-only sbn_sparse_eval_sizes.  The model's prover and verifier must agree with each
other (completeness and the same transcript), the verifier must reject what it should, and the library's size formulas must give what the
model counts from the structure."""
import pytest

import sparse_eval_model as sem
from sparse_eval_model import R, Transcript

SHAPES = sem.SHAPES
LABEL = b"gens_sparse_eval_cpu"
TR_LABEL = b"sparse eval cpu"
_CACHE = {}


def model_gens(ol, shape, label=LABEL):
    key = ("gens", label, tuple(sorted(shape.lg.items())))
    if key not in _CACHE:
        _CACHE[key] = sem.make_gens({k: ol.gens_new(shape.R(k) + 1, label + b"_" + k.encode())[0] for k in ("ops", "mem", "derefs")}, shape)
    return _CACHE[key]


def _proved(ol, shape_key):
    """one honest proof per shape for the whole module"""
    if shape_key not in _CACHE:
        import dense_model as dm
        nx, ny, nnz = shape_key
        mats, rx, ry, evals, rnd = sem.instance(shape_key)
        dense = dm.Dense(nx, ny, mats)
        shape = sem.Shape(nx, ny, dense.N, dense.batch)
        gens = model_gens(ol, shape)
        tr = Transcript(TR_LABEL)
        proof = sem.prove(tr, nx, ny, mats, rx, ry, evals, gens, rnd)
        _CACHE[shape_key] = (mats, rx, ry, evals, dense, shape, gens, proof, tr.state(), sem.commit_dense(dense, gens, shape))
    return _CACHE[shape_key]


@pytest.mark.parametrize("shape_key", SHAPES)
def test_prove_then_verify_accepts_and_ends_in_the_same_state(ol, shape_key):
    nx, ny, nnz = shape_key
    mats, rx, ry, evals, dense, shape, gens, proof, state, comm = _proved(ol, shape_key)
    tv = Transcript(TR_LABEL)
    assert sem.verify(tv, proof, comm, dense.N, dense.cells, rx, ry, evals, gens)
    assert tv.state() == state
    b = sem.proof_bytes(proof)
    assert len(b) == sem.sizes(nx, ny, dense.N, dense.batch)[1]
    back = sem.proof_from_bytes(b, shape)
    assert sem.proof_bytes(back) == b
    tv = Transcript(TR_LABEL)
    assert sem.verify(tv, back, comm, dense.N, dense.cells, rx, ry, evals, gens) and tv.state() == state


@pytest.mark.parametrize("field", sem.FIELDS)
def test_verifier_rejects_a_flipped_byte_in_each_field(ol, field):
    shape_key = (2, 3, (3, 4, 1))
    mats, rx, ry, evals, dense, shape, gens, proof, _, comm = _proved(ol, shape_key)
    b = bytearray(sem.proof_bytes(proof))
    lo, hi = sem.field_spans(shape)[field]
    # the lowest byte of the field's last element, an x coordinate or a scalar; comm_derefs ends in the identity at this shape (its last row is
    # all padding), whose x bytes the decompression does not read: its first element instead
    b[lo if field == "comm_derefs" else hi - 32] ^= 1
    bad = sem.proof_from_bytes(bytes(b), shape)
    assert bad is None or not sem.verify(Transcript(TR_LABEL), bad, comm, dense.N, dense.cells, rx, ry, evals, gens)


def test_verifier_rejects_wrong_evals_and_the_prover_asserts(ol):
    shape_key = (2, 3, (3, 4, 1))
    nx, ny, _ = shape_key
    mats, rx, ry, evals, dense, shape, gens, proof, _, comm = _proved(ol, shape_key)
    wrong = [evals[0], (evals[1] + 1) % R, evals[2]]
    assert not sem.verify(Transcript(TR_LABEL), proof, comm, dense.N, dense.cells, rx, ry, wrong, gens)
    with pytest.raises(AssertionError, match="evals"):
        sem.prove(Transcript(TR_LABEL), nx, ny, mats, rx, ry, wrong, gens, sem.instance(shape_key)[4])


def test_equalize():
    assert sem.equalize([5], [6, 7, 8]) == ([0, 0, 5], [6, 7, 8])           # nx < ny: zeros in FRONT of rx
    assert sem.equalize([5, 6], [7, 8]) == ([5, 6], [7, 8])
    assert sem.equalize([5, 6, 7], [8]) == ([5, 6, 7], [0, 0, 8])
    assert sem.equalize([], [3]) == ([0], [3])


def test_sizes_against_the_models_counts(sbn):
    import dense_model as dm
    for nx, ny, nnz in SHAPES:
        N = max(dm.next_power_of_two(k) for k in nnz)
        assert sbn.sparse_eval_sizes(nx, ny, N, len(nnz)) == sem.sizes(nx, ny, N, len(nnz)), (nx, ny, nnz)
    for nx, ny, N, b in ((10, 10, 1 << 10, 3), (13, 13, 1 << 13, 3), (17, 17, 1 << 17, 3), (21, 21, 1 << 22, 3), (5, 20, 2, 1), (20, 5, 1 << 20, 4)):
        assert sbn.sparse_eval_sizes(nx, ny, N, b) == sem.sizes(nx, ny, N, b), (nx, ny, N, b)
    # the keyless shape by hand: ell_derefs = 25 -> L = 2^12, lg = 13; ell_ops = 26 -> lg 13; ell_mem = 22 -> lg 11
    assert sbn.sparse_eval_sizes(21, 21, 1 << 22, 3) == (9 + 2 * 37, 32 * 4096 + 32 * 45 + 64 * (21 * 20 + 22 * 21) + 256 * (21 + 66) + 576 + 64 * 37 + 384)


@pytest.mark.parametrize("args", [(2, 2, 4, 0), (2, 2, 4, 5), (2, 2, 1, 3), (2, 2, 6, 3), (2, 2, 0, 3), (0, 0, 4, 3)])
def test_sizes_refuses(sbn, args):
    """batch 0, batch 5, N = 1, N not a power of two, N = 0, no memory variable"""
    import ctypes as C
    a, b = C.c_size_t(7), C.c_size_t(7)
    assert sbn.lib().sbn_sparse_eval_sizes(*[C.c_size_t(x) for x in args], C.byref(a), C.byref(b)) == -1          # SBN_EINVAL
    assert (a.value, b.value) == (7, 7)
    with pytest.raises(sbn.SbnError):
        sbn.sparse_eval_sizes(*args)
