"""CPU: dense_model.py (the reference's sequential loops behind MultiSparseMatPolynomialAsDense) pinned independently of itself — a
hand-worked instance, the sizes and offsets, the memory-checking identity the protocol rests on, the numpy expectation the keyless GPU
test uses — and the library's new entry points without a device."""
import ctypes as C
import random

import numpy as np
import pytest

import dense_model as dm
import r1cs_model as rm

R = dm.R


def test_hand_worked_instance():
    """num_vars_x = 2, num_vars_y = 1: cells = 4.  Two matrices with 5 and 3 entries: N = 8.

    A: rows 1 3 1 0 1, cols 0 2 2 3 0        B: rows 3 1 0, cols 2 2 2        (both padded with zeros to 8 ops: the padding reads cell 0)

    row side, ops in (k, i) order, count of earlier ops on the same cell:
      A addr 1 3 1 0 1 0 0 0 -> read_ts 0 0 1 0 2 1 2 3     (cell 0 now has 4 ops, cell 1 three, cell 3 one)
      B addr 3 1 0 0 0 0 0 0 -> read_ts 1 3 4 5 6 7 8 9
      audit_ts = 10 4 0 2
    col side:
      A addr 0 2 2 3 0 0 0 0 -> read_ts 0 0 1 0 1 2 3 4     (cell 0 now has 5 ops, cell 2 two, cell 3 one)
      B addr 2 2 2 0 0 0 0 0 -> read_ts 2 3 4 5 6 7 8 9
      audit_ts = 10 0 5 1"""
    A = ([1, 3, 1, 0, 1], [0, 2, 2, 3, 0], [7, 0, 1, R - 1, 5])
    B = ([3, 1, 0], [2, 2, 2], [2, 3, 4])
    d = dm.Dense(2, 1, [A, B])
    assert (d.batch, d.N, d.cells) == (2, 8, 4)
    assert d.addr[0] == [[1, 3, 1, 0, 1, 0, 0, 0], [3, 1, 0, 0, 0, 0, 0, 0]]
    assert d.read_ts[0] == [[0, 0, 1, 0, 2, 1, 2, 3], [1, 3, 4, 5, 6, 7, 8, 9]]
    assert d.audit_ts[0] == [10, 4, 0, 2]
    assert d.addr[1] == [[0, 2, 2, 3, 0, 0, 0, 0], [2, 2, 2, 0, 0, 0, 0, 0]]
    assert d.read_ts[1] == [[0, 0, 1, 0, 1, 2, 3, 4], [2, 3, 4, 5, 6, 7, 8, 9]]
    assert d.audit_ts[1] == [10, 0, 5, 1]
    assert d.val == [[7, 0, 1, R - 1, 5, 0, 0, 0], [2, 3, 4, 0, 0, 0, 0, 0]]
    assert len(d.comb_ops) == 128 and d.comb_ops[80:] == [0] * 48
    assert d.comb_ops[16:32] == [0, 0, 1, 0, 2, 1, 2, 3, 1, 3, 4, 5, 6, 7, 8, 9]          # group 1: row read_ts of A, then B
    assert d.comb_ops[d.ops_start(2, 1):d.ops_start(2, 1) + 8] == [2, 2, 2, 0, 0, 0, 0, 0]
    assert d.comb_ops[d.ops_start(4, 0):d.ops_start(4, 0) + 8] == [7, 0, 1, R - 1, 5, 0, 0, 0]
    assert d.comb_mem == [10, 4, 0, 2, 10, 0, 5, 1]


@pytest.mark.parametrize("nx,ny,nnz,N,cells", [
    (3, 5, (0,), 1, 32), (5, 3, (0, 0, 0), 1, 32), (4, 4, (1, 0), 1, 16), (2, 6, (8, 3, 5), 8, 64), (6, 2, (9, 3, 5), 16, 64),
    (1, 1, (33,), 64, 2), (0, 0, (2, 2), 2, 1), (3, 3, (4, 4, 4, 4, 4, 4, 4, 4), 4, 8)])
def test_sizes_and_offsets(nx, ny, nnz, N, cells):
    rng = random.Random(nx * 100 + ny)
    mats = [([rng.randrange(cells) for _ in range(n)], [rng.randrange(cells) for _ in range(n)], [rng.randrange(R) for _ in range(n)]) for n in nnz]
    d = dm.Dense(nx, ny, mats)
    b = len(nnz)
    assert (d.N, d.cells, d.batch) == (N, cells, b)
    assert len(d.comb_ops) == dm.next_power_of_two(5 * b * N) and len(d.comb_mem) == 2 * cells
    for g, src in enumerate((d.addr[0], d.read_ts[0], d.addr[1], d.read_ts[1], d.val)):
        for j in range(b):
            assert d.ops_start(g, j) == (g * b + j) * N
            assert d.comb_ops[d.ops_start(g, j):d.ops_start(g, j) + N] == src[j]
    assert d.comb_ops[5 * b * N:] == [0] * (len(d.comb_ops) - 5 * b * N)
    for side in (0, 1):
        assert sum(d.audit_ts[side]) == b * N
        assert d.comb_mem[side * cells:(side + 1) * cells] == d.audit_ts[side]


def _random_mats(rng, batch, cells, nnz_max, skew):
    mats = []
    for _ in range(batch):
        n = rng.randrange(nnz_max + 1)
        pick = (lambda: rng.randrange(min(cells, 3))) if skew else (lambda: rng.randrange(cells))
        mats.append(([pick() for _ in range(n)], [pick() for _ in range(n)], [rng.randrange(R) for _ in range(n)]))
    return mats


@pytest.mark.parametrize("seed,batch,nx,ny,nnz_max,skew", [(1, 1, 3, 4, 20, False), (2, 3, 5, 3, 70, False), (3, 3, 2, 2, 100, True), (4, 2, 6, 6, 9, True)])
def test_memory_checking_identity(seed, batch, nx, ny, nnz_max, skew):
    """prod init * prod_k prod write_k == prod_k prod read_k * prod audit, per side, for any memory contents and challenges
    (sparse_mlpoly_full.rs:745-796 and the verifier's product check); one wrong rank or count breaks it"""
    rng = random.Random(seed)
    d = dm.Dense(nx, ny, _random_mats(rng, batch, 2 ** max(nx, ny), nnz_max, skew))
    for side in (0, 1):
        mem = [rng.randrange(R) for _ in range(d.cells)]
        g, tau = rng.randrange(R), rng.randrange(R)
        init, reads, writes, audit = dm.memory_products(d, side, mem, g, tau)
        assert init * dm.product(writes) % R == dm.product(reads) * audit % R
        # the check has teeth: one read_ts off by one, or one audit count moved to a neighbour, breaks it
        k = rng.randrange(d.batch); i = rng.randrange(d.N)
        d.read_ts[side][k][i] += 1
        init, reads, writes, audit = dm.memory_products(d, side, mem, g, tau)
        assert init * dm.product(writes) % R != dm.product(reads) * audit % R
        d.read_ts[side][k][i] -= 1
        if d.cells > 1:
            a = max(range(d.cells), key=lambda c: d.audit_ts[side][c])
            d.audit_ts[side][a] -= 1; d.audit_ts[side][(a + 1) % d.cells] += 1
            init, reads, writes, audit = dm.memory_products(d, side, mem, g, tau)
            assert init * dm.product(writes) % R != dm.product(reads) * audit % R


def test_numpy_expectation_agrees_with_model_on_keyless_prefix():
    """the keyless GPU test takes its expected arrays from dense_model.numpy_expectation (stable argsort + bincount); here that agrees with
    the sequential loops on an instance shaped like a prefix of the keyless one: the same skewed, shuffled triplets, about 2^12 ops per matrix"""
    nc, nv, mats = rm.keyless_instance(1)
    nx, ny = nc.bit_length() - 1, (2 * nv).bit_length() - 1
    assert (nx, ny) == (20, 21)
    small = [(r[:n], c[:n], v[:n]) for (r, c, v), n in zip(mats, (3151, 1040, 2940))]
    N, cells, addr, read_ts, audit = dm.numpy_expectation(nx, ny, small)
    d = dm.Dense(nx, ny, [([int(x) for x in r], [int(x) for x in c], rm.vals_as_ints(np.ascontiguousarray(v))) for r, c, v in small])
    assert (N, cells) == (d.N, d.cells) == (4096, 1 << 21)
    for side in (0, 1):
        assert addr[side].tolist() == d.addr[side]
        assert read_ts[side].tolist() == d.read_ts[side]
        assert audit[side].tolist() == d.audit_ts[side]
    # and on a tiny instance where every op shares one cell / no two ops share one
    one = [([2] * 7, [1] * 7, [1] * 7), ([2] * 8, [1] * 8, [1] * 8)]
    distinct = [(list(range(0, 8)), list(range(8, 16)), [1] * 8), (list(range(8, 16)), list(range(0, 8)), [1] * 8)]
    for mats2 in (one, distinct):
        N, cells, addr, read_ts, audit = dm.numpy_expectation(4, 3, mats2)
        d = dm.Dense(4, 3, mats2)
        for side in (0, 1):
            assert read_ts[side].tolist() == d.read_ts[side] and audit[side].tolist() == d.audit_ts[side] and addr[side].tolist() == d.addr[side]


def test_dense_entry_points_fail_loudly_without_gpu(sbn):
    """the library exports the dense calls; without a context they return an error (never a result), and the accessors of a NULL handle
    return 0 / NULL.  With no device, no context can be made, so no build can succeed: there is no CPU fallback."""
    L = sbn.lib()
    for name in ("sbn_dense_build", "sbn_dense_free", "sbn_dense_num_ops", "sbn_dense_num_cells", "sbn_dense_batch", "sbn_dense_addr_dev",
                 "sbn_dense_read_ts_dev", "sbn_dense_audit_ts_dev", "sbn_dense_comb_ops", "sbn_dense_comb_mem"):
        assert name in sbn.EXPORTED_SYMBOLS and hasattr(L, name)
    rows = (C.c_void_p * 1)(); nnz = (C.c_size_t * 1)(0); out = C.c_void_p(1)
    rc = L.sbn_dense_build(None, C.c_size_t(2), C.c_size_t(2), rows, rows, rows, nnz, C.c_size_t(1), C.c_uint32(0), C.byref(out))
    assert rc == -1
    assert L.sbn_dense_num_ops(None) == 0 and L.sbn_dense_num_cells(None) == 0 and L.sbn_dense_batch(None) == 0
    assert L.sbn_dense_addr_dev(None, 0, 0) is None and L.sbn_dense_read_ts_dev(None, 1, 0) is None and L.sbn_dense_audit_ts_dev(None, 0) is None
    assert L.sbn_dense_comb_ops(None) is None and L.sbn_dense_comb_mem(None) is None
    L.sbn_dense_free(None, None)
    import torch
    if not torch.cuda.is_available():
        with pytest.raises(sbn.SbnError):
            sbn.Context(0)
