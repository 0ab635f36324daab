"""GPU: sbn_sparse_eval_prove_kzg — the KZG build's SparseMatPolyEvalProof::prove (sparse_mlpoly_full.rs:1757-1813) in one call — and
sbn_derefs_key, the per-cell SRS sums its commitment can run over: against the literal model of the reference (tests/sparse_eval_kzg_model.py),
against the same proof assembled from the entry points that existed before it on the full padded length (tests/sparse_eval_kzg_loop.py),
the key against the oracle's scalar multiplications, and the edge inputs, state and refusals.  Every comparison is bit-exact."""
import ctypes as C
import random

import numpy as np
import pytest

import dense_model as dm
import r1cs_model as rm
import sparse_eval_kzg_loop as loop
import sparse_eval_kzg_model as skm
import sparse_eval_model as sem
from sparse_eval_model import R, Transcript

pytestmark = pytest.mark.gpu
LABEL = b"gens_sparse_eval_kzg_gpu"
TR_LABEL = b"sparse eval kzg gpu"
KINDS = skm.KINDS
TAU = random.Random(1757).randrange(1, R)
_GENS, _SRS, _MODEL = {}, {}, {}


def _sbs(xs):
    return b"".join(sem.pm.sb(x) for x in xs)


def _gens(ctx, shape, label=LABEL, points=True):
    """({kind: handle}, the model's gens or None) per size pair and label for the whole module"""
    key = (tuple(shape.lg[k] for k in KINDS), label)
    if key not in _GENS:
        made = {k: ctx.gens_new(shape.R(k) + 1, label + b"_" + k.encode(), want_points=points) for k in KINDS}
        _GENS[key] = ({k: made[k][0] for k in KINDS}, {k: sem.pm.split_gens(made[k][1], shape.R(k)) for k in KINDS} if points else None)
    return _GENS[key]


def _srs(ctx, n):
    """the device SRS of n points from TAU, once per length and module"""
    if n not in _SRS:
        _SRS[n] = ctx.kzg_srs_from_tau(_sbs([TAU]), n)
    return _SRS[n]


@pytest.fixture(scope="module", autouse=True)
def _free_handles():
    yield
    for handles, _ in _GENS.values():
        for h in handles.values():
            h.free()
    for s in _SRS.values():
        s.free()
    _GENS.clear(); _SRS.clear(); _MODEL.clear()


def _dense(ctx, nx, ny, mats):
    return ctx.dense_build(nx, ny, [(r, c, _sbs(v)) for r, c, v in mats])


def _shape_of(nx, ny, mats):
    return sem.Shape(nx, ny, dm.num_ops(mats), len(mats))


def _n_d(shape):
    return 1 << shape.ell["derefs"]


def _device(ctx, sbn, nx, ny, mats, rx, ry, evals, handles, srs, rnd, with_key, label=TR_LABEL):
    """-> (proof, transcript state); the dense representation's two tables must be left as they were"""
    dense = _dense(ctx, nx, ny, mats)
    key = ctx.derefs_key_build(dense, srs) if with_key else None
    tr = sbn.Transcript(label)
    try:
        before = (ctx.table_download(dense.comb_ops), ctx.table_download(dense.comb_mem))
        proof = ctx.sparse_eval_prove_kzg(dense, _sbs(rx), _sbs(ry), _sbs(evals), handles["ops"], handles["mem"], srs, key, _sbs(rnd), tr)
        assert (ctx.table_download(dense.comb_ops), ctx.table_download(dense.comb_mem)) == before
        return proof, tr.state()
    finally:
        if key is not None:
            key.free()
        dense.free()


def _model(key, nx, ny, inst, gens, srs_n):
    """the model's proof once per key and module -> (inst, proof bytes, transcript state, dense, shape)"""
    if key not in _MODEL:
        mats, rx, ry, evals, rnd = inst
        tm_ = Transcript(TR_LABEL)
        proof = skm.prove(tm_, nx, ny, mats, rx, ry, evals, gens, skm.Srs(TAU, srs_n), rnd)
        dense = dm.Dense(nx, ny, mats)
        _MODEL[key] = (inst, skm.proof_bytes(proof), tm_.state(), dense, sem.Shape(nx, ny, dense.N, dense.batch))
    return _MODEL[key]


# ---- against the model ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("with_key", [True, False], ids=["key", "no key"])
@pytest.mark.parametrize("shape_key", sem.SHAPES)
def test_bit_exact_against_the_model(ctx, sbn, ol, shape_key, with_key):
    """an SRS of n_d + 1 points: the reference's size"""
    nx, ny, _ = shape_key
    inst = skm.instance(shape_key)
    shp = _shape_of(nx, ny, inst[0])
    handles, gens = _gens(ctx, shp)
    srs_n = _n_d(shp) + 1
    (mats, rx, ry, evals, rnd), want, want_state, dense, shape = _model(shape_key, nx, ny, inst, gens, srs_n)
    proof, state = _device(ctx, sbn, nx, ny, mats, rx, ry, evals, handles, _srs(ctx, srs_n), rnd, with_key)
    assert len(proof) == sbn.sparse_eval_kzg_sizes(nx, ny, dense.N, dense.batch)[1]
    assert proof == want
    assert state == want_state
    if with_key:
        comm = (sem.pm.commit_poly(gens["ops"], dense.comb_ops, None, shape.ell["ops"]), sem.pm.commit_poly(gens["mem"], dense.comb_mem, None, shape.ell["mem"]))
        tv = Transcript(TR_LABEL)
        assert skm.verify(tv, skm.proof_from_bytes(proof, shape), comm, dense.N, dense.cells, rx, ry, evals, gens, skm.Srs(TAU, srs_n))
        assert tv.state() == state


# ---- against the loop through the entry points that existed before, on the full padded n_d ----------------------------------------------

# b = 3: n' = 6 N of n_d = 8 N, the division and both MSMs of the one call stop two blocks early; b = 1: n' = n_d.  2^10 and 2^13 lie on both sides of
# the 2048-entry switch of the product tail and of the division's single-tile level
@pytest.mark.parametrize("b,lg_n", [(3, 10), (3, 13), (1, 10)])
def test_equals_the_loop_through_the_calls_that_existed_before(ctx, sbn, b, lg_n):
    nx = ny = lg_n
    N = 1 << lg_n
    shape = sem.Shape(nx, ny, N, b)
    handles, _ = _gens(ctx, shape, LABEL + b"_loop", points=False)
    srs = _srs(ctx, _n_d(shape) + 1)
    rng = np.random.default_rng(100 * b + lg_n)
    dense = ctx.dense_build(nx, ny, loop.random_mats(nx, ny, N, b, 50 + lg_n + b))
    rx, ry = rm.random_vals(rng, nx).tobytes(), rm.random_vals(rng, ny).tobytes()
    rnd = rm.random_vals(rng, skm.sizes(nx, ny, N, b)[0]).tobytes()
    lg = loop.LoopGens(ctx, None, 0, N)
    key = ctx.derefs_key_build(dense, srs)
    try:
        evals = loop.evals_of(sbn, ctx, dense, rx, ry)
        t0, t1, t2 = sbn.Transcript(TR_LABEL), sbn.Transcript(TR_LABEL), sbn.Transcript(TR_LABEL)
        many = loop.prove_loop(sbn, ctx, dense, rx, ry, evals, handles["ops"], handles["mem"], srs, lg, rnd, t0)
        keyed = ctx.sparse_eval_prove_kzg(dense, rx, ry, evals, handles["ops"], handles["mem"], srs, key, rnd, t1)
        plain = ctx.sparse_eval_prove_kzg(dense, rx, ry, evals, handles["ops"], handles["mem"], srs, None, rnd, t2)
        assert len(many) == skm.sizes(nx, ny, N, b)[1]
        assert keyed == many and plain == many
        assert t1.state() == t0.state() and t2.state() == t0.state()
    finally:
        key.free(); lg.free(); dense.free()


# ---- the key against the oracle ------------------------------------------------------------------------------------------------------

def _key_expect(ol, dense_model, srs_n):
    """{side << 31 | a: S[side][a]} from the oracle: one scalar multiplication of G per cell"""
    return {(side << 31) | a: skm.mul_g(s) for (side, a), s in skm.key_scalars(dense_model, skm.Srs(TAU, srs_n)).items()}


@pytest.mark.parametrize("shape_key", sem.SHAPES)
def test_key_every_point_against_the_oracle(ctx, sbn, ol, shape_key):
    nx, ny, _ = shape_key
    mats, rx, ry, _, _ = skm.instance(shape_key)
    dm_ = dm.Dense(nx, ny, mats)
    srs_n = 2 * dm_.batch * dm_.N                          # exactly n': the least the build takes
    dense = _dense(ctx, nx, ny, mats)
    key = ctx.derefs_key_build(dense, _srs(ctx, srs_n))
    try:
        want = _key_expect(ol, dm_, srs_n)
        ids, pts = key.download()
        assert len(key) == len(want) and ids == sorted(want)
        assert pts == [want[i] for i in ids]
        assert key.download(1, len(ids) - 1) == (ids[1:], pts[1:]) and key.download(len(ids), 0) == ([], [])
        with pytest.raises(sbn.SbnError):
            key.download(1, len(ids))
        rx_ext, ry_ext = sem.equalize(rx, ry)
        mem_rx, mem_ry = ctx.eq_evals(_sbs(rx_ext)), ctx.eq_evals(_sbs(ry_ext))
        try:
            xy, inf = ctx.derefs_key_commit(key, mem_rx, mem_ry)
            mx, my, _, _, comb = skm.derefs_comb(dm_, rx, ry)
            assert not inf and xy == skm.mul_g(skm.Srs(TAU, srs_n).commit_scalar(comb))
        finally:
            mem_rx.free(); mem_ry.free()
    finally:
        key.free(); dense.free()


def test_key_of_a_skewed_circuit(ctx, sbn, ol):
    """b = 1, nx = ny = 10, N = 2^14.  Row side: one cell holds N - 250 ops, a second 200, 50 ops are spread singly, the other cells are unread;
    column side: uniform.  With SEG = 32 the heavy cell is cut into ~500 segments (k_acc_extra, the wave form of k_acc_merge), the second into 7
    (the lane form); the premises are asserted, not assumed"""
    nx = ny = 10
    N, cells = 1 << 14, 1 << 10
    rng = np.random.default_rng(14)
    heavy, second = 777, 5
    singles = [c for c in rng.permutation(cells) if c not in (heavy, second)][:50]
    rows = np.array([heavy] * (N - 250) + [second] * 200 + [int(c) for c in singles], dtype=np.uint32)
    rows = rows[rng.permutation(N)]
    cols = rng.integers(0, cells, N, dtype=np.uint32)
    vals = rm.random_vals(rng, N)
    srs_n = 2 * N + 1
    srs = _srs(ctx, srs_n)
    dense = ctx.dense_build(nx, ny, [(rows, cols, vals)])
    key = ctx.derefs_key_build(dense, srs)
    made = []
    try:
        acc = ctx.prof_last_acc()
        SEG = acc["SEG"]
        assert acc["LPB"] == 1
        assert N - 250 > 13 * SEG and SEG < 200 <= 13 * SEG, acc            # both merge forms and k_acc_extra have run
        assert acc["big_count"] >= 2 and acc["extra_count"] >= (N - 250 + SEG - 1) // SEG - 1 + (200 + SEG - 1) // SEG - 1
        pw = skm.Srs(TAU, srs_n).powers(2 * N)
        by_cell = {}
        for side, arr in ((0, rows), (1, cols)):
            for i, a in enumerate(arr.tolist()):
                by_cell.setdefault((side << 31) | a, []).append(side * N + i)
        ids, pts = key.download()
        assert len(key) == len(by_cell) == len(ids) and ids == sorted(by_cell)        # no unread cell, every read one
        assert sum(1 for i in ids if not i >> 31) == 52
        pick = random.Random(3).sample(ids, 64) + [heavy, second]
        for i in pick:
            assert pts[ids.index(i)] == skm.mul_g(sum(pw[e] for e in by_cell[i]) % R), hex(i)
        rx, ry = rm.random_vals(rng, nx).tobytes(), rm.random_vals(rng, ny).tobytes()
        mem_rx, mem_ry = ctx.eq_evals(rx), ctx.eq_evals(ry); made += [mem_rx, mem_ry]
        derefs = ctx.gather_merge([mem_rx, mem_ry], [dense.addr_dev(0, 0), dense.addr_dev(1, 0)], N); made.append(derefs)
        assert ctx.derefs_key_commit(key, mem_rx, mem_ry) == ctx.kzg_commit(srs, derefs, 2 * N)
    finally:
        for t in made:
            t.free()
        key.free(); dense.free()


# ---- edges ---------------------------------------------------------------------------------------------------------------------------

def _edge(ctx, sbn, name, nx, ny, mats, rx, ry, rnd_seed):
    evals = sem.true_evals(nx, ny, mats, rx, ry)
    shp = _shape_of(nx, ny, mats)
    inst = (mats, rx, ry, evals, sem.random_scalars(skm.sizes(nx, ny, shp.N, shp.b)[0], rnd_seed))
    handles, gens = _gens(ctx, shp)
    srs_n = _n_d(shp) + 1
    _, want, want_state, _, shape = _model(name, nx, ny, inst, gens, srs_n)
    for with_key in (True, False):
        assert _device(ctx, sbn, nx, ny, *inst[:4], handles, _srs(ctx, srs_n), inst[4], with_key) == (want, want_state), with_key
    return want, shape, evals


def test_the_point_zero(ctx, sbn, ol):
    """rx = ry = 0: both eq tables are the unit vector of cell 0, derefs is 0 / 1"""
    nx, ny, nnz = 2, 3, (4, 2, 3)
    _edge(ctx, sbn, "point zero", nx, ny, sem.random_mats(nx, ny, nnz, 71), [0] * nx, [0] * ny, 72)


def test_all_values_zero(ctx, sbn, ol):
    nx, ny, nnz = 2, 2, (4, 3, 4)
    mats = [(r, c, [0] * len(v)) for r, c, v in sem.random_mats(nx, ny, nnz, 61)]
    want, shape, evals = _edge(ctx, sbn, "zero values", nx, ny, mats, sem.random_scalars(nx, 62), sem.random_scalars(ny, 63), 64)
    assert evals == [0, 0, 0]
    lo, hi = skm.field_spans(shape)["prod.eval_val"]
    assert want[lo:hi] == bytes(hi - lo)


def test_an_srs_of_exactly_n_d_minus_1_points_with_batch_1(ctx, sbn, ol):
    """b = 1: n' = n_d.  The commit drops the last real coefficient as kzg.rs:388 does, the quotient's n_d - 1 bases just fit, the key build
    refuses (it needs all n' points)"""
    shape_key = (2, 2, (4,))
    nx, ny, _ = shape_key
    inst = skm.instance(shape_key, seed=3)
    shp = _shape_of(nx, ny, inst[0])
    handles, gens = _gens(ctx, shp)
    srs_n = _n_d(shp) - 1
    assert srs_n == 2 * shp.N - 1
    (mats, rx, ry, evals, rnd), want, want_state, dense_m, _ = _model("srs n_d - 1", nx, ny, inst, gens, srs_n)
    assert _device(ctx, sbn, nx, ny, mats, rx, ry, evals, handles, _srs(ctx, srs_n), rnd, False) == (want, want_state)
    _, _, _, _, comb = skm.derefs_comb(dense_m, rx, ry)
    assert comb[-1] != 0                                   # the dropped coefficient is a real one
    dense = _dense(ctx, nx, ny, mats)
    try:
        h = C.c_void_p(5)
        assert sbn.lib().sbn_derefs_key_build(ctx.h, dense.h, _srs(ctx, srs_n).h, C.byref(h)) == -1 and h.value is None
    finally:
        dense.free()


def test_an_srs_of_exactly_n_prefix_points_with_batch_3(ctx, sbn):
    """b = 3: the key builds on n' = 6 N points, the prove keeps the reference's requirement of n_d - 1 and refuses"""
    shape_key = (2, 3, (3, 4, 1))
    nx, ny, _ = shape_key
    mats, rx, ry, evals, rnd = skm.instance(shape_key)
    shp = _shape_of(nx, ny, mats)
    handles, _ = _gens(ctx, shp)
    srs = _srs(ctx, 6 * shp.N)
    dense = _dense(ctx, nx, ny, mats)
    key = ctx.derefs_key_build(dense, srs)
    tr = sbn.Transcript(TR_LABEL)
    state0 = tr.state()
    try:
        assert len(key) >= 2
        for k in (key, None):
            with pytest.raises(sbn.SbnError, match="kzg.rs:186"):
                ctx.sparse_eval_prove_kzg(dense, _sbs(rx), _sbs(ry), _sbs(evals), handles["ops"], handles["mem"], srs, k, _sbs(rnd), tr)
        assert tr.state() == state0
    finally:
        key.free(); dense.free()


# ---- state and refusals --------------------------------------------------------------------------------------------------------------

def test_a_wrong_eval_is_refused_and_the_next_call_is_right(ctx, sbn, ol):
    shape_key = (2, 3, (3, 4, 1))
    nx, ny, _ = shape_key
    inst = skm.instance(shape_key)
    shp = _shape_of(nx, ny, inst[0])
    handles, gens = _gens(ctx, shp)
    srs_n = _n_d(shp) + 1
    srs = _srs(ctx, srs_n)
    (mats, rx, ry, evals, rnd), want, want_state, _, shape = _model(shape_key, nx, ny, inst, gens, srs_n)
    dense = _dense(ctx, nx, ny, mats)
    key = ctx.derefs_key_build(dense, srs)
    tr = sbn.Transcript(TR_LABEL)
    state0 = tr.state()
    proof = (C.c_uint8 * len(want))()
    wrong = [evals[0], (evals[1] + 1) % R, evals[2]]
    try:
        rc = sbn.lib().sbn_sparse_eval_prove_kzg(ctx.h, dense.h, _sbs(rx), C.c_size_t(nx), _sbs(ry), C.c_size_t(ny), _sbs(wrong), handles["ops"].h, handles["mem"].h,
                                                 srs.h, key.h, _sbs(rnd), tr.h, proof)
        assert rc == -1 and b"sparse_mlpoly_full.rs:1366" in sbn.lib().sbn_last_error(ctx.h)
        assert tr.state() == state0 and bytes(proof) == bytes(len(want))
        assert ctx.sparse_eval_prove_kzg(dense, _sbs(rx), _sbs(ry), _sbs(evals), handles["ops"], handles["mem"], srs, key, _sbs(rnd), tr) == want
        assert tr.state() == want_state
    finally:
        key.free(); dense.free()


def test_results_do_not_depend_on_what_the_context_the_srs_and_the_key_ran_before(ctx, sbn):
    """keyed, plain, the Hyrax call on the same dense handle, a KZG commit and open over the same SRS, then keyed and plain again, and a fresh
    context with a fresh SRS and key: equal bytes and states throughout"""
    shape_key = (3, 2, (5, 0, 8))
    nx, ny, _ = shape_key
    mats, rx, ry, evals, rnd = skm.instance(shape_key, seed=5)
    shp = _shape_of(nx, ny, mats)
    label = LABEL + b"_state"
    handles, _ = _gens(ctx, shp, label, points=False)
    srs_n = _n_d(shp) + 1
    srs = _srs(ctx, srs_n)
    args = (_sbs(rx), _sbs(ry), _sbs(evals))

    def run(c, dense, h, s, key):
        tr = sbn.Transcript(TR_LABEL)
        return c.sparse_eval_prove_kzg(dense, *args, h["ops"], h["mem"], s, key, _sbs(rnd), tr), tr.state()
    dense = _dense(ctx, nx, ny, mats)
    key = ctx.derefs_key_build(dense, srs)
    g_der = ctx.gens_new((1 << sem.Shape(nx, ny, shp.N, shp.b).lg["derefs"]) + 1, label + b"_derefs", want_points=False)[0]
    z = ctx.table_upload(_sbs(sem.random_scalars(64, 9)))
    try:
        first = run(ctx, dense, handles, srs, key)
        assert run(ctx, dense, handles, srs, None) == first
        hy_rnd = _sbs(sem.random_scalars(sem.sizes(nx, ny, shp.N, shp.b)[0], 6))
        hyrax = [ctx.sparse_eval_prove(dense, *args, handles["ops"], handles["mem"], g_der, hy_rnd, sbn.Transcript(TR_LABEL)) for _ in range(2)]
        assert hyrax[0] == hyrax[1]
        other = (ctx.kzg_commit(srs, z, 64), ctx.kzg_open(srs, z, 64, _sbs([12345])))
        assert run(ctx, dense, handles, srs, key) == first
        assert run(ctx, dense, handles, srs, None) == first
        assert (ctx.kzg_commit(srs, z, 64), ctx.kzg_open(srs, z, 64, _sbs([12345]))) == other
        fresh_ctx = sbn.Context(0)
        made = []
        try:
            fh = {k: fresh_ctx.gens_new(shp.R(k) + 1, label + b"_" + k.encode(), want_points=False)[0] for k in KINDS}; made += list(fh.values())
            fs = fresh_ctx.kzg_srs_from_tau(_sbs([TAU]), srs_n); made.append(fs)
            fd = fresh_ctx.dense_build(nx, ny, [(r, c, _sbs(v)) for r, c, v in mats])
            fk = fresh_ctx.derefs_key_build(fd, fs)
            try:
                assert run(fresh_ctx, fd, fh, fs, None) == first
                assert run(fresh_ctx, fd, fh, fs, fk) == first
            finally:
                fk.free(); fd.free()
        finally:
            for h in made:
                h.free()
            fresh_ctx.close()
    finally:
        z.free(); g_der.free(); key.free(); dense.free()


def test_refusals_leave_everything_as_it_was(ctx, sbn, ol):
    shape_key = (2, 3, (3, 4, 1))
    nx, ny, _ = shape_key
    inst = skm.instance(shape_key)
    shp = _shape_of(nx, ny, inst[0])
    handles, gens = _gens(ctx, shp)
    srs_n = _n_d(shp) + 1
    srs = _srs(ctx, srs_n)
    (mats, rx, ry, evals, rnd), want, want_state, _, shape = _model(shape_key, nx, ny, inst, gens, srs_n)
    dense = _dense(ctx, nx, ny, mats)
    dense_same = _dense(ctx, nx, ny, mats)                                   # the same circuit, another handle
    dense_b5 = _dense(ctx, nx, ny, sem.random_mats(nx, ny, (2, 2, 2, 2, 2), 91))
    dense_n1 = _dense(ctx, nx, ny, sem.random_mats(nx, ny, (1, 0, 1), 92))
    Rk = {k: shape.R(k) for k in KINDS}
    no_h = {k: ctx.bases_upload(ctx.bases_download(handles[k], 0, Rk[k] + 1)) for k in KINDS}
    longer = {k: ctx.gens_new(Rk[k] + 2, LABEL + b"_" + k.encode(), want_points=False)[0] for k in KINDS}
    srs_h = ctx.gens_new(srs_n - 1, LABEL + b"_srs_with_h", want_points=False)[0]      # srs_n points, the last one an h
    srs_short, srs_long = _srs(ctx, _n_d(shp) - 2), _srs(ctx, srs_n + 1)
    key = ctx.derefs_key_build(dense, srs)
    key_other_dense = ctx.derefs_key_build(dense_same, srs)
    key_other_srs = ctx.derefs_key_build(dense, srs_long)
    tr = sbn.Transcript(TR_LABEL)
    state0 = tr.state()
    big = R.to_bytes(32, "little")
    rx_b, ry_b, ev_b, rnd_b = _sbs(rx), _sbs(ry), _sbs(evals), _sbs(rnd)
    proof = (C.c_uint8 * len(want))()
    tables0 = (ctx.table_download(dense.comb_ops), ctx.table_download(dense.comb_mem))

    def raw(**kw):
        a = dict(ctx=ctx.h, dense=dense.h, rx=rx_b, nx=nx, ry=ry_b, ny=ny, evals=ev_b, ops=handles["ops"].h, mem=handles["mem"].h, srs=srs.h, key=key.h,
                 rnd=rnd_b, tr=tr.h, proof=proof)
        a.update(kw)
        return sbn.lib().sbn_sparse_eval_prove_kzg(a["ctx"], a["dense"], a["rx"], C.c_size_t(a["nx"]), a["ry"], C.c_size_t(a["ny"]), a["evals"], a["ops"], a["mem"], a["srs"],
                                                   a["key"], a["rnd"], a["tr"], a["proof"])
    cases = {k: {k: None} for k in ("dense", "rx", "ry", "evals", "ops", "mem", "srs", "rnd", "tr", "proof")}      # a null pointer (a null key is no refusal)
    cases.update({
        "batch = 5": dict(dense=dense_b5.h, evals=ev_b + ev_b[:64], key=None),
        "N = 1": dict(dense=dense_n1.h, key=None),
        "nx, ny too short for the handle": dict(rx=rx_b[:32], nx=1, ry=ry_b[:64], ny=2),
        "ny too long for the handle": dict(ry=ry_b + ry_b[:32], ny=ny + 1),
        "rx[0] >= r": dict(rx=big + rx_b[32:]),
        "ry[last] >= r": dict(ry=ry_b[:-32] + big),
        "evals[1] >= r": dict(evals=ev_b[:32] + big + ev_b[64:]),
        "rnd[0] >= r": dict(rnd=big + rnd_b[32:]),
        "rnd[last] >= r": dict(rnd=rnd_b[:-32] + big),
        "an SRS with h": dict(srs=srs_h.h, key=None),
        "an SRS of n_d - 2 points": dict(srs=srs_short.h, key=None),
        "a key of another dense handle": dict(key=key_other_dense.h),
        "a key of another SRS length": dict(key=key_other_srs.h),
        "the key's dense handle, another SRS": dict(srs=srs_long.h),
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
        assert raw(srs=srs_short.h, key=None) == -1 and b"kzg.rs:186" in sbn.lib().sbn_last_error(ctx.h)      # the text cites the reference's slice
        # the key build's own refusals: an SRS with h, fewer than n' points
        for bad in (srs_h, _srs(ctx, 6 * shp.N - 1)):
            h = C.c_void_p(5)
            assert sbn.lib().sbn_derefs_key_build(ctx.h, dense.h, bad.h, C.byref(h)) == -1 and h.value is None
        # each key is good for its own pair
        for d, s, k in ((dense_same, srs, key_other_dense), (dense, srs_long, key_other_srs), (dense, srs, key)):
            t2 = sbn.Transcript(TR_LABEL)
            assert ctx.sparse_eval_prove_kzg(d, rx_b, ry_b, ev_b, handles["ops"], handles["mem"], s, k, rnd_b, t2) == want and t2.state() == want_state
        assert tr.state() == state0
    finally:
        for h in [key, key_other_dense, key_other_srs, dense, dense_same, dense_b5, dense_n1, srs_h] + list(no_h.values()) + list(longer.values()):
            h.free()
