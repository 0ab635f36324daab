"""GPU: sbn_sparse_eval_prove — SparseMatPolyEvalProof::prove (sparse_mlpoly_full.rs:1700-1755) in one call — against the literal model of the
reference (tests/sparse_eval_model.py), against the same proof assembled from the entry points that existed before it
(tests/sparse_eval_loop.py), and its edge inputs, state and refusals.  Every comparison is bit-exact."""
import ctypes as C
import random

import numpy as np
import pytest

import dense_model as dm
import r1cs_model as rm
import sparse_eval_loop as loop
import sparse_eval_model as sem
from sparse_eval_model import R, Transcript

pytestmark = pytest.mark.gpu
LABEL = b"gens_sparse_eval_gpu"
TR_LABEL = b"sparse eval gpu"
KINDS = ("ops", "mem", "derefs")
_GENS = {}
_MODEL = {}


def _sbs(xs):
    return b"".join(sem.pm.sb(x) for x in xs)


def _gens(ctx, shape, label=LABEL, points=True):
    """({kind: handle}, the model's gens or None) per size triple and label for the whole module: the derived sets are built once"""
    key = (tuple(shape.lg[k] for k in KINDS), label)
    if key not in _GENS:
        made = {k: ctx.gens_new(shape.R(k) + 1, label + b"_" + k.encode(), want_points=points) for k in KINDS}
        _GENS[key] = ({k: made[k][0] for k in KINDS}, sem.make_gens({k: made[k][1] for k in KINDS}, shape) if points else None)
    return _GENS[key]


@pytest.fixture(scope="module", autouse=True)
def _free_gens():
    yield
    for handles, _ in _GENS.values():
        for h in handles.values():
            h.free()
    _GENS.clear(); _MODEL.clear()


def _dense(ctx, nx, ny, mats):
    return ctx.dense_build(nx, ny, [(r, c, _sbs(v)) for r, c, v in mats])


def _device(ctx, sbn, nx, ny, mats, rx, ry, evals, handles, rnd, label=TR_LABEL):
    """-> (proof, transcript state); asserts that the dense representation's two tables are left as they were"""
    dense = _dense(ctx, nx, ny, mats)
    tr = sbn.Transcript(label)
    try:
        before = (ctx.table_download(dense.comb_ops), ctx.table_download(dense.comb_mem))
        proof = ctx.sparse_eval_prove(dense, _sbs(rx), _sbs(ry), _sbs(evals), handles["ops"], handles["mem"], handles["derefs"], _sbs(rnd), tr)
        assert (ctx.table_download(dense.comb_ops), ctx.table_download(dense.comb_mem)) == before
        return proof, tr.state()
    finally:
        dense.free()


def _model(key, nx, ny, inst, gens):
    """the model's proof once per key and module -> (inst, proof bytes, transcript state, dense, shape)"""
    if key not in _MODEL:
        mats, rx, ry, evals, rnd = inst
        tm_ = Transcript(TR_LABEL)
        proof = sem.prove(tm_, nx, ny, mats, rx, ry, evals, gens, rnd)
        dense = dm.Dense(nx, ny, mats)
        _MODEL[key] = (inst, sem.proof_bytes(proof), tm_.state(), dense, sem.Shape(nx, ny, dense.N, dense.batch))
    return _MODEL[key]


def _shape_of(nx, ny, mats):
    return sem.Shape(nx, ny, dm.num_ops(mats), len(mats))


@pytest.mark.parametrize("shape_key", sem.SHAPES)
def test_bit_exact_against_the_model(ctx, sbn, shape_key):
    nx, ny, _ = shape_key
    inst = sem.instance(shape_key)
    handles, gens = _gens(ctx, _shape_of(nx, ny, inst[0]))
    (mats, rx, ry, evals, rnd), want, want_state, dense, shape = _model(shape_key, nx, ny, inst, gens)
    proof, state = _device(ctx, sbn, nx, ny, mats, rx, ry, evals, handles, rnd)
    assert proof == want
    assert state == want_state
    tv = Transcript(TR_LABEL)
    assert sem.verify(tv, sem.proof_from_bytes(proof, shape), sem.commit_dense(dense, gens, shape), dense.N, dense.cells, rx, ry, evals, gens)
    assert tv.state() == state
    if shape_key == (2, 3, (3, 4, 1)):                      # 6 x 4 = 24 derefs in a 4 x 8 matrix: the last row is all padding
        lo, hi = sem.field_spans(shape)["comm_derefs"]
        assert proof[hi - 32:hi] == sbn.g1_compress(bytes(64)) and proof[lo:lo + 32] != sbn.g1_compress(bytes(64))


# the ops circuits start at N entries, the mem circuits at 2^max(nx, ny): 2^10 and 2^13 lie on both sides of the 2048-entry switch to the one-launch
# product tail; at 2^17 the combined product-proof kernels run on layers >= 2^16 with 12 circuits and the derefs commit is 1024 x 1024
@pytest.mark.parametrize("lg_n", [10, 13, 17])
def test_equals_the_loop_through_the_calls_that_existed_before(ctx, sbn, lg_n):
    nx = ny = lg_n
    N, b = 1 << lg_n, 3
    shape = sem.Shape(nx, ny, N, b)
    handles, _ = _gens(ctx, shape, LABEL + b"_loop", points=False)
    rng = np.random.default_rng(lg_n)
    dense = ctx.dense_build(nx, ny, loop.random_mats(nx, ny, N, b, 50 + lg_n))
    rx, ry = rm.random_vals(rng, nx).tobytes(), rm.random_vals(rng, ny).tobytes()
    rnd = rm.random_vals(rng, sem.sizes(nx, ny, N, b)[0]).tobytes()
    lg = loop.LoopGens(ctx, handles["derefs"], shape.R("derefs"), N)
    try:
        evals = loop.evals_of(sbn, ctx, dense, rx, ry)
        t1, t2 = sbn.Transcript(TR_LABEL), sbn.Transcript(TR_LABEL)
        one = ctx.sparse_eval_prove(dense, rx, ry, evals, handles["ops"], handles["mem"], handles["derefs"], rnd, t1)
        many = loop.prove_loop(sbn, ctx, dense, rx, ry, evals, handles["ops"], handles["mem"], handles["derefs"], lg, rnd, t2)
        assert len(one) == sem.sizes(nx, ny, N, b)[1]
        assert one == many
        assert t1.state() == t2.state()
    finally:
        lg.free(); dense.free()


def test_all_values_zero(ctx, sbn):
    """every dot-product claim and every evals[i] is 0"""
    nx, ny, nnz = 2, 2, (4, 3, 4)
    mats = [(r, c, [0] * len(v)) for r, c, v in sem.random_mats(nx, ny, nnz, 61)]
    rx, ry = sem.random_scalars(nx, 62), sem.random_scalars(ny, 63)
    evals = sem.true_evals(nx, ny, mats, rx, ry)
    assert evals == [0, 0, 0]
    inst = (mats, rx, ry, evals, sem.random_scalars(sem.sizes(nx, ny, 4, 3)[0], 64))
    handles, gens = _gens(ctx, _shape_of(nx, ny, mats))
    _, want, want_state, _, shape = _model("zero values", nx, ny, inst, gens)
    proof, state = _device(ctx, sbn, nx, ny, *inst[:4], handles, inst[4])
    assert (proof, state) == (want, want_state)
    lo, hi = sem.field_spans(shape)["prod.eval_val"]
    assert proof[lo:hi] == bytes(hi - lo)


def test_the_point_zero(ctx, sbn):
    """rx = ry = 0: both eq tables are the unit vector of cell 0"""
    nx, ny, nnz = 2, 3, (4, 2, 3)
    mats = sem.random_mats(nx, ny, nnz, 71)
    rx, ry = [0] * nx, [0] * ny
    inst = (mats, rx, ry, sem.true_evals(nx, ny, mats, rx, ry), sem.random_scalars(sem.sizes(nx, ny, 4, 3)[0], 72))
    handles, gens = _gens(ctx, _shape_of(nx, ny, mats))
    _, want, want_state, _, _ = _model("point zero", nx, ny, inst, gens)
    assert _device(ctx, sbn, nx, ny, *inst[:4], handles, inst[4]) == (want, want_state)


def test_a_wrong_eval_is_refused_and_the_next_call_is_right(ctx, sbn):
    shape_key = (2, 3, (3, 4, 1))
    nx, ny, _ = shape_key
    inst = sem.instance(shape_key)
    handles, gens = _gens(ctx, _shape_of(nx, ny, inst[0]))
    (mats, rx, ry, evals, rnd), want, want_state, _, shape = _model(shape_key, nx, ny, inst, gens)
    dense = _dense(ctx, nx, ny, mats)
    tr = sbn.Transcript(TR_LABEL)
    state0 = tr.state()
    proof = (C.c_uint8 * len(want))()
    wrong = [evals[0], (evals[1] + 1) % R, evals[2]]
    try:
        rc = sbn.lib().sbn_sparse_eval_prove(ctx.h, dense.h, _sbs(rx), C.c_size_t(nx), _sbs(ry), C.c_size_t(ny), _sbs(wrong), handles["ops"].h, handles["mem"].h,
                                             handles["derefs"].h, _sbs(rnd), tr.h, proof)
        assert rc == -1 and b"sparse_mlpoly_full.rs:1366" in sbn.lib().sbn_last_error(ctx.h)          # SBN_EINVAL: the reference panics there
        assert tr.state() == state0 and bytes(proof) == bytes(len(want))
        assert ctx.sparse_eval_prove(dense, _sbs(rx), _sbs(ry), _sbs(evals), handles["ops"], handles["mem"], handles["derefs"], _sbs(rnd), tr) == want
        assert tr.state() == want_state
    finally:
        dense.free()


def test_results_do_not_depend_on_what_the_context_and_the_handles_ran_before(ctx, sbn):
    """two proofs in a row on one context and one on a fresh context give equal bytes; the standalone joint opening and product proof on the
    same generator handles give before and after what they give on a fresh context"""
    shape_key = (3, 2, (5, 0, 8))
    nx, ny, _ = shape_key
    mats, rx, ry, evals, rnd = sem.instance(shape_key, seed=5)
    shape = _shape_of(nx, ny, mats)
    label = LABEL + b"_state"
    handles, _ = _gens(ctx, shape, label, points=False)

    def standalone(c, h):
        """sbn_joint_opening_prove over gens_ops and sbn_product_proof_prove at this shape's sizes"""
        rng = random.Random(81)
        ell_r, count = shape.n, 1 << (shape.ell["ops"] - shape.n)
        Z = [rng.randrange(R) for _ in range(1 << shape.ell["ops"])]
        zt = c.table_upload(_sbs(Z))
        tr = sbn.Transcript(b"standalone")
        ins = [c.table_upload(_sbs([rng.randrange(R) for _ in range(8)])) for _ in range(4)]
        pcs = c.product_circuit_many(ins)
        try:
            o1 = c.joint_opening_prove(h["ops"], zt, _sbs([rng.randrange(R) for _ in range(count)]), sem.OPS_LABELS, _sbs([rng.randrange(R) for _ in range(ell_r)]),
                                       _sbs([rng.randrange(R) for _ in range(3 + 2 * shape.lg["ops"])]), tr)
            o2 = c.product_proof_prove([[ins[i]] + pcs[i][:-1] for i in range(4)], [], tr)
            return o1, o2, tr.state()
        finally:
            zt.free()
            for t in [x for pc in pcs for x in pc] + ins:
                t.free()
    before = standalone(ctx, handles)
    first = _device(ctx, sbn, nx, ny, mats, rx, ry, evals, handles, rnd)
    second = _device(ctx, sbn, nx, ny, mats, rx, ry, evals, handles, rnd)
    assert first == second
    after = standalone(ctx, handles)
    assert before == after
    fresh_ctx = sbn.Context(0)
    try:
        fresh = {k: fresh_ctx.gens_new(shape.R(k) + 1, label + b"_" + k.encode(), want_points=False)[0] for k in KINDS}
        try:
            assert _device(fresh_ctx, sbn, nx, ny, mats, rx, ry, evals, fresh, rnd) == first
            assert standalone(fresh_ctx, fresh) == before
        finally:
            for h in fresh.values():
                h.free()
    finally:
        fresh_ctx.close()


def test_refusals_leave_everything_as_it_was(ctx, sbn):
    shape_key = (2, 3, (3, 4, 1))
    nx, ny, _ = shape_key
    inst = sem.instance(shape_key)
    handles, gens = _gens(ctx, _shape_of(nx, ny, inst[0]))
    (mats, rx, ry, evals, rnd), want, want_state, _, shape = _model(shape_key, nx, ny, inst, gens)
    dense = _dense(ctx, nx, ny, mats)
    dense_b5 = _dense(ctx, nx, ny, sem.random_mats(nx, ny, (2, 2, 2, 2, 2), 91))
    dense_n1 = _dense(ctx, nx, ny, sem.random_mats(nx, ny, (1, 0, 1), 92))
    Rk = {k: shape.R(k) for k in KINDS}
    no_h = {k: ctx.bases_upload(ctx.bases_download(handles[k], 0, Rk[k] + 1)) for k in KINDS}
    longer = {k: ctx.gens_new(Rk[k] + 2, LABEL + b"_" + k.encode(), want_points=False)[0] for k in KINDS}
    tr = sbn.Transcript(TR_LABEL)
    state0 = tr.state()
    big = R.to_bytes(32, "little")
    rx_b, ry_b, ev_b, rnd_b = _sbs(rx), _sbs(ry), _sbs(evals), _sbs(rnd)
    proof = (C.c_uint8 * len(want))()
    tables0 = (ctx.table_download(dense.comb_ops), ctx.table_download(dense.comb_mem))

    def raw(**kw):
        a = dict(ctx=ctx.h, dense=dense.h, rx=rx_b, nx=nx, ry=ry_b, ny=ny, evals=ev_b, ops=handles["ops"].h, mem=handles["mem"].h, derefs=handles["derefs"].h,
                 rnd=rnd_b, tr=tr.h, proof=proof)
        a.update(kw)
        return sbn.lib().sbn_sparse_eval_prove(a["ctx"], a["dense"], a["rx"], C.c_size_t(a["nx"]), a["ry"], C.c_size_t(a["ny"]), a["evals"], a["ops"], a["mem"], a["derefs"],
                                               a["rnd"], a["tr"], a["proof"])
    cases = {k: {k: None} for k in ("dense", "rx", "ry", "evals", "ops", "mem", "derefs", "rnd", "tr", "proof")}      # a null pointer
    cases.update({
        "batch = 5": dict(dense=dense_b5.h, evals=ev_b + ev_b[:64]),
        "N = 1": dict(dense=dense_n1.h),
        "nx, ny too short for the handle": dict(rx=rx_b[:32], nx=1, ry=ry_b[:64], ny=2),
        "ny too long for the handle": dict(ry=ry_b + ry_b[:32], ny=ny + 1),
        "rx[0] >= r": dict(rx=big + rx_b[32:]),
        "ry[last] >= r": dict(ry=ry_b[:-32] + big),
        "evals[1] >= r": dict(evals=ev_b[:32] + big + ev_b[64:]),
        "rnd[0] >= r": dict(rnd=big + rnd_b[32:]),
        "rnd[last] >= r": dict(rnd=rnd_b[:-32] + big),
    })
    for k in KINDS:
        cases["gens_%s without h" % k] = {k: no_h[k].h}
        cases["gens_%s of the wrong size" % k] = {k: longer[k].h}
    try:
        assert raw(ctx=None) == -1
        for name, kw in cases.items():
            assert raw(**kw) == -1, name                    # SBN_EINVAL
            assert tr.state() == state0 and bytes(proof) == bytes(len(want)), name
        assert (ctx.table_download(dense.comb_ops), ctx.table_download(dense.comb_mem)) == tables0
        assert raw(dense=dense_n1.h) == -1 and b"product_tree.rs:89" in sbn.lib().sbn_last_error(ctx.h)      # the text cites the reference's assert
        assert raw(derefs=no_h["derefs"].h) == -1 and b"nizk/mod.rs" in sbn.lib().sbn_last_error(ctx.h)
        got = ctx.sparse_eval_prove(dense, rx_b, ry_b, ev_b, handles["ops"], handles["mem"], handles["derefs"], rnd_b, tr)
        assert got == want and tr.state() == want_state
    finally:
        for h in [dense, dense_b5, dense_n1] + list(no_h.values()) + list(longer.values()):
            h.free()


# ---- sbn_hash_layer_pair_product: the hashing pass that also leaves the first product layer ------------------------------------------

def _u32_dev(ctx, arr):
    p = ctx.dev_alloc(4 * len(arr))
    ctx.dev_upload(p, np.ascontiguousarray(arr, dtype=np.uint32).tobytes())
    return p


# 2 and 4: one and two indices; 512: one block of 256 indices; 2^13: several blocks; 2^17: 256 blocks
@pytest.mark.parametrize("kind", ["read / write", "init / audit"])
@pytest.mark.parametrize("n", [2, 4, 512, 1 << 13, 1 << 17])
def test_hash_layer_pair_product_equals_the_pair_and_the_product_layers(ctx, sbn, n, kind):
    """against sbn_hash_layer_pair + sbn_product_layer after download, for both pair kinds; timestamps of 2^32 - 1 sit at both ends and in the
    middle, so the write set (add 1) holds 2^32: the sum must not wrap before it enters the field"""
    rng = np.random.default_rng(n + len(kind))
    val_b = rm.random_vals(rng, n).tobytes()
    addr = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    ts = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    ts[0] = ts[n // 2] = ts[n - 1] = 0xffffffff
    r_hash, r_multiset = rm.random_vals(rng, 1).tobytes(), rm.random_vals(rng, 1).tobytes()
    val = ctx.table_upload(val_b)
    d_addr, d_ts = _u32_dev(ctx, addr), _u32_dev(ctx, ts)
    args = (d_addr, val, d_ts, 0, d_ts, 1) if kind == "read / write" else (None, val, None, 0, d_ts, 0)
    made = []
    try:
        a, b = ctx.hash_layer_pair(*args, r_hash, r_multiset); made += [a, b]
        pa, pb = ctx.product_layer(a), ctx.product_layer(b); made += [pa, pb]
        fused = ctx.hash_layer_pair_product(*args, r_hash, r_multiset); made += list(fused)
        assert [len(t) for t in fused] == [n, n, n // 2, n // 2]
        want = [ctx.table_download(t) for t in (a, b, pa, pb)]
        assert [ctx.table_download(t) for t in fused] == want
        assert ctx.table_download(val) == val_b
        # entry 0 of the second set by hand: (ts + add) g^2 + val g + addr - tau with ts + add = 2^32 (write) or 2^32 - 1 (audit)
        g, tau, v0 = (int.from_bytes(x[:32], "little") for x in (r_hash, r_multiset, val_b))
        t0, a0 = ((1 << 32), int(addr[0])) if kind == "read / write" else ((1 << 32) - 1, 0)
        assert int.from_bytes(want[1][:32], "little") == (t0 * g * g + v0 * g + a0 - tau) % R
    finally:
        for t in made + [val]:
            t.free()
        ctx.dev_free(d_addr); ctx.dev_free(d_ts)


def test_hash_layer_pair_product_with_r_hash_zero_and_its_refusals(ctx, sbn):
    """r_hash = 0: every hash is addr - tau.  Tables of 1, 3 and 6 entries are refused (the first product layer halves the set, and the layers
    above need a power of two): SBN_EINVAL, the four out-handles left null, nothing launched.  sbn_gather_merge_rows returns nrows * R entries
    for any nrows, which is how a caller comes to hold a table of 3 or 6"""
    n = 8
    rng = np.random.default_rng(5)
    val = ctx.table_upload(rm.random_vals(rng, n).tobytes())
    one = ctx.table_upload(rm.random_vals(rng, 1).tobytes())
    addr = np.arange(3, 3 + n, dtype=np.uint32)
    d_addr, d_id = _u32_dev(ctx, addr), _u32_dev(ctx, np.arange(n, dtype=np.uint32))
    zero, tau = bytes(32), rm.random_vals(rng, 1).tobytes()
    made = []
    try:
        fused = ctx.hash_layer_pair_product(d_addr, val, d_addr, 0, d_addr, 1, zero, tau); made += list(fused)
        t = int.from_bytes(tau, "little")
        h = [(int(x) - t) % R for x in addr]
        assert ctx.table_download(fused[0]) == ctx.table_download(fused[1]) == _sbs(h)
        assert ctx.table_download(fused[2]) == _sbs([h[i] * h[i + n // 2] % R for i in range(n // 2)])
        three = ctx.gather_merge_rows([val], [d_id], 4, 1, 0, 1, 3); made.append(three)         # rows 0 .. 2 of the 4 x 1 view of val[:4]
        six = ctx.gather_merge_rows([val], [d_id], 8, 2, 0, 1, 3); made.append(six)             # rows 0 .. 2 of the 4 x 2 view of val
        assert (len(three), len(six)) == (3, 6) and ctx.table_download(six) == ctx.table_download(val)[:6 * 32]
        ctx.sync(); ctx.prof_reset(); ctx.prof_enable(True)
        try:
            for bad in (one, three, six):
                hs = [C.c_void_p() for _ in range(4)]
                rc = sbn.lib().sbn_hash_layer_pair_product(ctx.h, C.c_void_p(d_addr), bad.h, C.c_void_p(d_addr), C.c_uint32(0), C.c_void_p(d_addr), C.c_uint32(1), zero, tau, *[C.byref(x) for x in hs])
                assert rc == -1 and all(x.value is None for x in hs), len(bad)          # SBN_EINVAL
                assert b"power of two" in sbn.lib().sbn_last_error(ctx.h)
            assert ctx.prof_get() == {}                             # no kernel ran
        finally:
            ctx.prof_enable(False)
        hs = [C.c_void_p() for _ in range(4)]
        rc = sbn.lib().sbn_hash_layer_pair_product(ctx.h, None, val.h, None, C.c_uint32(0), None, C.c_uint32(1), R.to_bytes(32, "little"), tau, *[C.byref(x) for x in hs])
        assert rc == -1
    finally:
        for x in made + [val, one]:
            x.free()
        ctx.dev_free(d_addr); ctx.dev_free(d_id)
