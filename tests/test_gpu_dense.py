"""GPU: MultiSparseMatPolynomialAsDense on the device (sbn_dense_*) against the pure-int model of the reference's loops (dense_model.py),
all through the C ABI and bit for bit: every u32 array, the whole of comb_ops and comb_mem, the size accessors at small shapes; two builds
of one input; errors; the hand-off of the handle's arrays and tables to the gather, hash-layer, product-circuit, evaluate and commit calls;
and the keyless-shaped instance in full against a numpy expectation, then the memory-checking identity on the device at that size."""
import ctypes as C
import random

import numpy as np
import pytest

import dense_model as dm
import r1cs_model as rm
from conftest import rand_scalars

pytestmark = pytest.mark.gpu
R = dm.R
EINVAL = -1


def _u32(ctx, ptr, n):
    return np.frombuffer(ctx.dev_download(ptr, 4 * n), np.uint32)


def _download_np(ctx, sbn, t):
    """a table as an (len, 32) uint8 array of canonical little-endian scalars, without an intermediate copy"""
    out = np.empty((len(t), 32), np.uint8)
    rc = sbn.lib().sbn_table_download(ctx.h, t.h, out.ctypes.data_as(C.POINTER(C.c_uint8)))
    assert rc == 0, sbn.lib().sbn_last_error(ctx.h)
    return out


def _ints_as_scalars(a):
    """uint32 array -> (n, 32) uint8: Scalar::from_u64 as canonical bytes"""
    out = np.zeros((len(a), 8), np.uint32)
    out[:, 0] = a
    return out.view(np.uint8).reshape(len(a), 32)


def _build(ctx, nx, ny, mats, mont=False):
    conv = rm.ark_mont if mont else (lambda v: v)
    dev = [(np.array(r, np.uint32), np.array(c, np.uint32), rm.to_bytes([conv(v) for v in vals])) for r, c, vals in mats]
    return ctx.dense_build(nx, ny, dev, flags=1 if mont else 0)


def _val(rng):
    return (0, 1, R - 1, rng.randrange(R))[rng.randrange(4)]


def _mat(rng, n, cells, kind="uniform"):
    if kind == "one":
        a = rng.randrange(cells); rows = [a] * n; cols = [cells - 1 - a] * n
    elif kind == "distinct":
        assert n <= cells
        rows = rng.sample(range(cells), n); cols = rng.sample(range(cells), n)
    else:
        rows = [rng.randrange(cells) for _ in range(n)]; cols = [rng.randrange(cells) for _ in range(n)]
        for _ in range(min(n // 4, 40)):                              # duplicates of whole entries, a hot cell, the last cell
            i, j = rng.randrange(n), rng.randrange(n)
            rows[i], cols[i] = rows[j], cols[j]
        for i in range(0, n, 3):
            rows[i] = cells - 1
        for i in range(1, n, 5):
            cols[i] = cells - 1
    vals = [_val(rng) for _ in range(n)]
    perm = list(range(n)); rng.shuffle(perm)
    return [rows[i] for i in perm], [cols[i] for i in perm], [vals[i] for i in perm]


# (id, num_vars_x, num_vars_y, [(nnz, kind)])
SHAPES = [
    ("b1_x_gt_y_N_lt_cells", 7, 4, [(20, "uniform")]),
    ("b2_x_eq_y_N_gt_cells", 3, 3, [(100, "uniform"), (37, "uniform")]),
    ("b3_x_lt_y", 4, 9, [(300, "uniform"), (1, "uniform"), (513, "uniform")]),
    ("b3_one_empty", 5, 6, [(64, "uniform"), (0, "uniform"), (10, "uniform")]),
    ("b3_all_empty", 5, 6, [(0, "uniform")] * 3),
    ("b2_pow2_no_padding", 6, 6, [(256, "uniform"), (256, "uniform")]),
    ("b2_pow2_plus_one", 6, 8, [(257, "uniform"), (256, "uniform")]),
    ("b3_all_on_one_cell", 8, 5, [(3000, "one"), (4096, "one"), (5, "one")]),
    ("b2_all_distinct", 12, 13, [(4096, "distinct"), (8192, "distinct")]),
    ("b1_every_op_its_own_cell", 13, 12, [(8192, "distinct")]),
    ("b3_several_tiles_and_passes", 10, 17, [(9000, "uniform"), (16384, "uniform"), (16385, "uniform")]),
    ("b1_single_cell", 0, 0, [(9, "uniform")]),
    ("b8", 3, 2, [(5, "uniform")] * 8),
]


def _instance(shape, seed):
    _, nx, ny, spec = shape
    rng = random.Random(seed)
    cells = 2 ** max(nx, ny)
    if all(kind == "one" for _, kind in spec):                         # ONE address over the whole batch
        a = rng.randrange(cells)
        return [([a] * n, [cells - 1] * n, [_val(rng) for _ in range(n)]) for n, _ in spec]
    return [_mat(rng, n, cells, kind) for n, kind in spec]


def _check_against_model(ctx, sbn, h, d):
    assert (h.num_ops, h.num_cells, h.batch) == (d.N, d.cells, d.batch)
    assert len(h.comb_ops) == len(d.comb_ops) and len(h.comb_mem) == len(d.comb_mem)
    for side in (0, 1):
        for k in range(d.batch):
            assert _u32(ctx, h.addr_dev(side, k), d.N).tolist() == d.addr[side][k], f"addr side {side} matrix {k}"
            assert _u32(ctx, h.read_ts_dev(side, k), d.N).tolist() == d.read_ts[side][k], f"read_ts side {side} matrix {k}"
        assert _u32(ctx, h.audit_ts_dev(side), d.cells).tolist() == d.audit_ts[side], f"audit_ts side {side}"
    assert ctx.table_download(h.comb_ops) == rm.to_bytes(d.comb_ops), "comb_ops"
    assert ctx.table_download(h.comb_mem) == rm.to_bytes(d.comb_mem), "comb_mem"


@pytest.mark.parametrize("shape", SHAPES, ids=[s[0] for s in SHAPES])
def test_dense_small_vs_model(ctx, sbn, shape):
    _, nx, ny, _ = shape
    mats = _instance(shape, len(shape[0]) * 31 + nx)
    h = _build(ctx, nx, ny, mats)
    try:
        _check_against_model(ctx, sbn, h, dm.Dense(nx, ny, mats))
    finally:
        h.free()


@pytest.mark.parametrize("shape", [SHAPES[2], SHAPES[3], SHAPES[9]], ids=[SHAPES[2][0], SHAPES[3][0], SHAPES[9][0]])
def test_dense_mont_input(ctx, sbn, shape):
    _, nx, ny, _ = shape
    mats = _instance(shape, 77 + nx)
    h = _build(ctx, nx, ny, mats, mont=True)
    try:
        _check_against_model(ctx, sbn, h, dm.Dense(nx, ny, mats))
    finally:
        h.free()


def test_dense_two_builds_identical(ctx, sbn):
    shape = SHAPES[9]
    _, nx, ny, _ = shape
    mats = _instance(shape, 5)
    got = []
    for _ in range(2):
        h = _build(ctx, nx, ny, mats)
        try:
            n = 4 * h.batch * h.num_ops + 2 * h.num_cells             # the handle's u32 arrays are one allocation, in this order
            got.append((ctx.dev_download(h.addr_dev(0, 0), 4 * n), ctx.table_download(h.comb_ops), ctx.table_download(h.comb_mem)))
        finally:
            h.free()
    assert got[0] == got[1]


def _raw_build(ctx, sbn, nx, ny, rows, cols, vals, nnz, batch, flags=0):
    """through ctypes, for argument shapes the binding never produces -> (rc, message)"""
    out = C.c_void_p()
    rc = sbn.lib().sbn_dense_build(ctx.h, C.c_size_t(nx), C.c_size_t(ny), rows, cols, vals, nnz, C.c_size_t(batch), C.c_uint32(flags), C.byref(out))
    assert rc != 0 and not out.value
    return rc, sbn.lib().sbn_last_error(ctx.h).decode()


def test_dense_errors_leave_context_usable(ctx, sbn):
    nx, ny = 3, 4
    good = _instance(("e", nx, ny, [(20, "uniform"), (9, "uniform")]), 3)
    cells = 16

    def expect(mats, text, flags=0, raw_vals=None):
        dev = [(np.array(r, np.uint32), np.array(c, np.uint32), rm.to_bytes(v) if raw_vals is None else raw_vals[m]) for m, (r, c, v) in enumerate(mats)]
        with pytest.raises(sbn.SbnError, match="rc=-1.*" + text):
            ctx.dense_build(nx, ny, dev, flags=flags)

    r, c, v = good[1]
    expect([good[0], (r + [cells], c + [0], v + [1])], "matrix 1 entry 9: row 16 >= num_cells 16")
    expect([good[0], (r + [0], c + [cells + 3], v + [1])], "matrix 1 entry 9: col 19 >= num_cells 16")
    for flags in (0, 1):
        expect([good[0], (r + [0], c + [0], v + [0])], "matrix 1 entry 9: value >= r", flags=flags,
               raw_vals=[rm.to_bytes(good[0][2]), rm.to_bytes(v) + R.to_bytes(32, "little")])
    with pytest.raises(sbn.SbnError, match="rc=-1.*batch=0"):
        ctx.dense_build(nx, ny, [])
    with pytest.raises(sbn.SbnError, match="rc=-1.*batch=9"):
        ctx.dense_build(nx, ny, [([], [], b"")] * 9)
    with pytest.raises(sbn.SbnError, match="rc=-1.*at most 31 variables"):
        ctx.dense_build(32, 2, [([], [], b"")])
    # a NULL array where a matrix has entries
    null2 = (C.c_void_p * 2)(); nnz = (C.c_size_t * 2)(0, 1)
    rc, msg = _raw_build(ctx, sbn, nx, ny, null2, null2, null2, nnz, 2)
    assert rc == EINVAL and "matrix 1 has 1 entries and a NULL array" in msg
    # batch * N > 2^31 is refused from the counts alone, before any entry is read
    one = np.zeros(8, np.uint32); p = (C.c_void_p * 2)(one.ctypes.data, one.ctypes.data); nnz = (C.c_size_t * 2)((1 << 30) + 1, 1)
    rc, msg = _raw_build(ctx, sbn, nx, ny, p, p, p, nnz, 2)
    assert rc == EINVAL and "exceeds 2^31" in msg
    h = _build(ctx, nx, ny, good)                                       # the context still works
    try:
        _check_against_model(ctx, sbn, h, dm.Dense(nx, ny, good))
        assert h.addr_dev(2, 0) is None and h.read_ts_dev(0, 2) is None and h.audit_ts_dev(-1) is None
    finally:
        h.free()


def _device_products(ctx, h, side, mem, g, tau):
    """the four memory-checking products of one side from the handle's arrays: sbn_gather_merge, sbn_hash_layer_pair, sbn_product_circuit_many,
    sbn_table_read0_many -> (init, [read_k], [write_k], audit) as ints"""
    b, N = h.batch, h.num_ops
    live = []
    try:
        comb = ctx.gather_merge([mem] * b, [h.addr_dev(side, k) for k in range(b)], N); live.append(comb)
        ops = []
        for k in range(b):
            v = ctx.table_slice(comb, k * N, N); live.append(v)
            rd, wr = ctx.hash_layer_pair(h.addr_dev(side, k), v, h.read_ts_dev(side, k), 0, h.read_ts_dev(side, k), 1, g, tau)
            live += [rd, wr]; ops += [rd, wr]
        init, audit = ctx.hash_layer_pair(None, mem, None, 0, h.audit_ts_dev(side), 0, g, tau); live += [init, audit]
        tops = []
        for group in (ops, [init, audit]):
            if len(group[0]) == 1:
                tops += group
            else:
                circ = ctx.product_circuit_many(group)
                for layers in circ:
                    live += layers; tops.append(layers[-1])
        p = [int.from_bytes(x, "little") for x in ctx.table_read0_many(tops)]
        return p[2 * b], p[0:2 * b:2], p[1:2 * b:2], p[2 * b + 1]
    finally:
        for t in reversed(live):
            t.free()


def test_dense_handoff(ctx, sbn, ol):
    """about 2^12 ops: the handle's arrays and tables as the inputs of the calls a prove makes with them"""
    nx, ny = 9, 10
    shape = ("h", nx, ny, [(4096, "uniform"), (3000, "uniform"), (2049, "uniform")])
    mats = _instance(shape, 9)
    d = dm.Dense(nx, ny, mats)
    h = _build(ctx, nx, ny, mats)
    g, tau = rand_scalars(1, 41), rand_scalars(1, 42)
    gi, ti = int.from_bytes(g, "little"), int.from_bytes(tau, "little")
    try:
        for side in (0, 1):
            mem_i = rm.from_bytes(rand_scalars(d.cells, 50 + side))
            mem = ctx.table_upload(rm.to_bytes(mem_i))
            try:
                # deref + merge (sparse_mlpoly_full.rs:245-257, 293-297)
                comb = ctx.gather_merge([mem] * d.batch, [h.addr_dev(side, k) for k in range(d.batch)], d.N)
                try:
                    assert ctx.table_download(comb) == rm.to_bytes(dm.merge([dm.deref(a, mem_i) for a in d.addr[side]]))
                finally:
                    comb.free()
                init, reads, writes, audit = _device_products(ctx, h, side, mem, g, tau)
                assert (init, reads, writes, audit) == dm.memory_products(d, side, mem_i, gi, ti)
                assert init * dm.product(writes) % R == dm.product(reads) * audit % R
            finally:
                mem.free()
        # evaluations of the 15 polynomials inside comb_ops and the two inside comb_mem (sparse_mlpoly_full.rs:907-976)
        r_ops = rand_scalars(d.N.bit_length() - 1, 60); r_mem = rand_scalars(d.cells.bit_length() - 1, 61)
        views = [h.ops_slice(grp, j) for grp in range(5) for j in range(d.batch)]
        mviews = [ctx.table_slice(h.comb_mem, s * d.cells, d.cells) for s in (0, 1)]
        try:
            got = rm.from_bytes(ctx.table_evaluate_many(views, r_ops))
            want = [dm.evaluate(d.comb_ops[s:s + d.N], rm.from_bytes(r_ops)) for s in range(0, 5 * d.batch * d.N, d.N)]
            assert got == want
            got = rm.from_bytes(ctx.table_evaluate_many(mviews, r_mem))
            assert got == [dm.evaluate(d.audit_ts[s], rm.from_bytes(r_mem)) for s in (0, 1)]
        finally:
            for t in views + mviews:
                t.free()
        # the two encode-time commitments (sparse_mlpoly_full.rs:183-184) against the oracle's row commitments of the model's bytes
        for t, z in ((h.comb_ops, d.comb_ops), (h.comb_mem, d.comb_mem)):
            lv, rv = sbn.factored_lens(len(z).bit_length() - 1); left, right = 1 << lv, 1 << rv
            gx, _ = ol.gens_new(right, b"gens_ops_test")
            bs = ctx.bases_upload(gx[:64 * right], gx[64 * right:])
            try:
                assert ctx.commit_table(bs, t, None, left, right)[0] == ol.commit_rows(rm.to_bytes(z), None, left, right, gx[:64 * right], gx[64 * right:], 16)
            finally:
                bs.free()
    finally:
        h.free()


def test_dense_keyless_shape(ctx, sbn):
    """the bench's synthetic instance (num_vars_x = 20, num_vars_y = 21, N = 2^22, cells = 2^21): every u32 array, comb_mem and comb_ops in full
    against the numpy expectation (dense_model.numpy_expectation, checked against the sequential loops in test_dense_model_cpu.py), comb_ops
    one slice at a time; then the memory-checking identity on the device at full size"""
    nc, nv, mats = rm.keyless_instance(1)
    nx, ny = nc.bit_length() - 1, (2 * nv).bit_length() - 1
    N, cells, addr, read_ts, audit = dm.numpy_expectation(nx, ny, mats)
    assert (N, cells) == (1 << 22, 1 << 21)
    h = ctx.dense_build(nx, ny, mats)
    try:
        assert (h.num_ops, h.num_cells, h.batch) == (N, cells, 3)
        assert len(h.comb_ops) == 1 << 26 and len(h.comb_mem) == 1 << 22
        for side in (0, 1):
            for k in range(3):
                assert np.array_equal(_u32(ctx, h.addr_dev(side, k), N), addr[side][k]), f"addr side {side} matrix {k}"
                assert np.array_equal(_u32(ctx, h.read_ts_dev(side, k), N), read_ts[side][k]), f"read_ts side {side} matrix {k}"
            assert np.array_equal(_u32(ctx, h.audit_ts_dev(side), cells), audit[side]), f"audit_ts side {side}"
        assert np.array_equal(_download_np(ctx, sbn, h.comb_mem), _ints_as_scalars(np.concatenate(audit))), "comb_mem"
        groups = (addr[0], read_ts[0], addr[1], read_ts[1])
        for q in range(16):                                              # 15 polynomials and the zero tail, one slice held at a time
            if q < 12:
                want = _ints_as_scalars(groups[q // 3][q % 3])
            else:
                want = np.zeros((N, 32), np.uint8)
                if q < 15:
                    v = mats[q - 12][2]; want[:len(v)] = v
            view = ctx.table_slice(h.comb_ops, q * N, N)
            try:
                assert np.array_equal(_download_np(ctx, sbn, view), want), f"comb_ops slice {q}"
            finally:
                view.free()
            del want
        g, tau = rand_scalars(1, 71), rand_scalars(1, 72)
        for side in (0, 1):
            mem = ctx.table_upload(rm.random_vals(np.random.default_rng(80 + side), cells).tobytes())
            try:
                init, reads, writes, aud = _device_products(ctx, h, side, mem, g, tau)
                assert init * dm.product(writes) % R == dm.product(reads) * aud % R, f"memory check, side {side}"
            finally:
                mem.free()
    finally:
        h.free()
