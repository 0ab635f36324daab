"""GPU: the R1CS matrices on the device (sbn_r1cs_*) against the pure-int model of the reference's three loops (r1cs_model.py):
multiply_vec, the phase-2 table and evaluate, bit for bit at small shapes; the hand-off of their tables to the sumcheck calls; errors;
and the keyless-shaped synthetic instance through the phase-2 claim identities and sampled rows and columns."""
import random

import numpy as np
import pytest

import r1cs_model as rm
from conftest import rand_scalars

pytestmark = pytest.mark.gpu
R = rm.R
EINVAL = "rc=-1"
SHAPES = [(2, 1), (1 << 4, 1 << 6), (1 << 10, 1 << 9), (1 << 12, 1 << 12)]


def _log2(n):
    return n.bit_length() - 1


def _val(rng):
    k = rng.randrange(4)
    return (0, 1, R - 1, rng.randrange(R))[k]


def _instance(nc, nv, seed, empty=None):
    """random triplets in random order with duplicates and 0 / 1 / r-1 / uniform values, empty rows (the top quarter of the rows), one
    row and one column longer than a chunk (and, at the largest shape, longer than one fix-up pass), matrix `empty` with nnz = 0.
    The seams a random draw cannot reach (the last rows of A and B, the fix-up pass counts, the carry cadence) are pinned in test_gpu_r1cs_seams.py"""
    rng = random.Random(seed)
    nz = 2 * nv
    live = max(1, (3 * nc) // 4)
    mats = []
    for m in range(3):
        if m == empty:
            mats.append(([], [], []))
            continue
        cnt = rng.randrange(1, 4 * nc + 8)
        rows = [rng.randrange(live) for _ in range(cnt)]
        cols = [rng.randrange(nz) for _ in range(cnt)]
        long = 40 if nc < 1024 else (600 if nc < 4096 else 20000)
        rows += [rng.randrange(live)] * long                        # one long row
        cols += [rng.randrange(nz) for _ in range(long)]
        rows += [rng.randrange(live) for _ in range(long)]          # one long column (the constant column of z)
        cols += [nv] * long
        dup = rng.randrange(len(rows))
        rows += [rows[dup]] * 3; cols += [cols[dup]] * 3            # duplicates add
        vals = [_val(rng) for _ in rows]
        perm = list(range(len(rows))); rng.shuffle(perm)
        mats.append(([rows[i] for i in perm], [cols[i] for i in perm], [vals[i] for i in perm]))
    return mats


def _upload(ctx, nc, nv, mats, mont=False):
    conv = rm.ark_mont if mont else (lambda v: v)
    dev = [(np.array(r, np.uint32), np.array(c, np.uint32), rm.to_bytes([conv(v) for v in vals])) for r, c, vals in mats]
    return ctx.r1cs_upload(nc, nv, dev, flags=1 if mont else 0)


def _rand(n, seed):
    return rm.from_bytes(rand_scalars(n, seed)) if n else []


def _points(ell, seed):
    """a random point and points with 0 / 1 coordinates (where the evaluation picks single cells)"""
    rng = random.Random(seed)
    return [_rand(ell, seed), [rng.randrange(2) for _ in range(ell)], [1] * ell, [0] * ell]


def _download(ctx, t):
    try:
        return rm.from_bytes(ctx.table_download(t))
    finally:
        t.free()


def _check_all(ctx, h, nc, nv, mats, z, seed):
    lx, ly = _log2(nc), _log2(2 * nv)
    tz = ctx.table_upload(rm.to_bytes(z))
    try:
        got = [_download(ctx, t) for t in ctx.r1cs_multiply(h, tz)]
    finally:
        tz.free()
    assert tuple(got) == rm.multiply_vec(nc, nv, mats, z), f"multiply ({nc}, {nv})"
    rs = [(0, 0, 0), (1, 1, 1), tuple(_rand(3, seed + 1)), (0, 1, R - 1)]
    for i, (rA, rB, rC) in enumerate(rs):
        rx = _points(lx, seed + 2 + i)[i % 4]
        t = ctx.r1cs_eval_table(h, rm.to_bytes(rx), *(rm.to_bytes([v]) for v in (rA, rB, rC)))
        assert len(t) == 2 * nv
        assert _download(ctx, t) == rm.eval_table(nc, nv, mats, rx, rA, rB, rC), f"eval_table ({nc}, {nv}) r={i}"
    for i, (rx, ry) in enumerate(zip(_points(lx, seed + 10), _points(ly, seed + 20))):
        got = tuple(rm.from_bytes(b"".join(ctx.r1cs_evaluate(h, rm.to_bytes(rx), rm.to_bytes(ry)))))
        assert got == rm.evaluate(nc, nv, mats, rx, ry), f"evaluate ({nc}, {nv}) point {i}"


@pytest.mark.parametrize("nc,nv", SHAPES)
def test_r1cs_small_vs_model(ctx, nc, nv):
    mats = _instance(nc, nv, nc * 7 + nv, empty=1 if nc == 16 else None)
    h = _upload(ctx, nc, nv, mats)
    try:
        _check_all(ctx, h, nc, nv, mats, _rand(2 * nv, nc + 3), nc + 5)
    finally:
        h.free()


@pytest.mark.parametrize("nc,nv", [(1 << 4, 1 << 6), (1 << 10, 1 << 9)])
def test_r1cs_mont_input(ctx, nc, nv):
    mats = _instance(nc, nv, 99 + nc, empty=2)
    h = _upload(ctx, nc, nv, mats, mont=True)
    try:
        _check_all(ctx, h, nc, nv, mats, _rand(2 * nv, 5), 17)
    finally:
        h.free()


def test_r1cs_all_empty(ctx):
    nc, nv = 16, 8
    mats = [([], [], [])] * 3
    h = _upload(ctx, nc, nv, mats)
    try:
        _check_all(ctx, h, nc, nv, mats, _rand(2 * nv, 6), 23)
    finally:
        h.free()


def test_r1cs_lazy_z_from_bind(ctx):
    """z is a bound table (lazy representatives, not what table_upload writes)"""
    nc, nv = 1 << 10, 1 << 9
    mats = _instance(nc, nv, 5)
    h = _upload(ctx, nc, nv, mats)
    full = _rand(4 * nv, 31); r = _rand(1, 32)[0]
    t = ctx.table_upload(rm.to_bytes(full))
    try:
        ctx.bind_top(t, rm.to_bytes([r]))
        z = [(lo + r * (hi - lo)) % R for lo, hi in zip(full[:2 * nv], full[2 * nv:])]
        got = tuple(_download(ctx, x) for x in ctx.r1cs_multiply(h, t))
        assert got == rm.multiply_vec(nc, nv, mats, z)
    finally:
        t.free(); h.free()


def test_r1cs_dropped_columns(ctx):
    """col >= 2 num_vars is dropped, as all three reference loops skip it"""
    nc, nv = 1 << 4, 1 << 3
    mats = _instance(nc, nv, 77)
    mats = [(r + [1, 2], c + [2 * nv, 2 * nv + 5], v + [3, R - 1]) for r, c, v in mats]
    h = _upload(ctx, nc, nv, mats)
    try:
        _check_all(ctx, h, nc, nv, mats, _rand(2 * nv, 8), 41)
    finally:
        h.free()


def test_r1cs_errors_leave_context_usable(ctx, sbn):
    nc, nv = 1 << 4, 1 << 3
    good = _instance(nc, nv, 3)
    bad_row = [(good[0][0] + [nc], good[0][1] + [0], good[0][2] + [1])] + good[1:]
    with pytest.raises(sbn.SbnError, match=EINVAL):
        _upload(ctx, nc, nv, bad_row)
    rows, cols, vals = good[1]
    bad_val = [(np.array(rows + [0], np.uint32), np.array(cols + [0], np.uint32), rm.to_bytes(vals) + R.to_bytes(32, "little"))]
    for flags in (0, 1):
        with pytest.raises(sbn.SbnError, match=EINVAL):
            ctx.r1cs_upload(nc, nv, [([], [], b""), bad_val[0], ([], [], b"")], flags=flags)
    # a NULL array where a matrix has non-zeros (through the C ABI: the binding never passes one)
    import ctypes as C
    null3 = (C.c_void_p * 3)(); nnz = (C.c_size_t * 3)(1, 0, 0); out = C.c_void_p()
    assert sbn.lib().sbn_r1cs_upload(ctx.h, C.c_size_t(nc), C.c_size_t(nv), null3, null3, null3, nnz, C.c_uint32(0), C.byref(out)) == -1
    with pytest.raises(sbn.SbnError, match=EINVAL):
        ctx.r1cs_upload(12, nv, [([], [], b"")] * 3)
    h = _upload(ctx, nc, nv, good)
    try:
        for n in (nv, 4 * nv):
            tz = ctx.table_upload(rm.to_bytes(_rand(n, 4)))
            try:
                with pytest.raises(sbn.SbnError, match=EINVAL):
                    ctx.r1cs_multiply(h, tz)
            finally:
                tz.free()
        one = rm.to_bytes([1])
        for lx in (_log2(nc) - 1, _log2(nc) + 1):
            with pytest.raises(sbn.SbnError, match=EINVAL):
                ctx.r1cs_eval_table(h, rm.to_bytes(_rand(lx, 1)), one, one, one)
            with pytest.raises(sbn.SbnError, match=EINVAL):
                ctx.r1cs_evaluate(h, rm.to_bytes(_rand(lx, 1)), rm.to_bytes(_rand(_log2(2 * nv), 2)))
        for ly in (_log2(nv), _log2(nv) + 2):
            with pytest.raises(sbn.SbnError, match=EINVAL):
                ctx.r1cs_evaluate(h, rm.to_bytes(_rand(_log2(nc), 1)), rm.to_bytes(_rand(ly, 2)))
        with pytest.raises(sbn.SbnError, match=EINVAL):
            ctx.r1cs_eval_table(h, rm.to_bytes(_rand(_log2(nc), 1)), R.to_bytes(32, "little"), one, one)      # r_A >= r
        _check_all(ctx, h, nc, nv, good, _rand(2 * nv, 9), 51)      # the context still works
    finally:
        h.free()


def test_r1cs_tables_feed_sumcheck(ctx, ol):
    """Az/Bz/Cz into sbn_sc_eval_r1cs with eq(tau) and ABC into sbn_sc_eval_quad with z, against the C oracle on the model's tables"""
    nc, nv = 1 << 10, 1 << 9
    mats = _instance(nc, nv, 11)
    h = _upload(ctx, nc, nv, mats)
    z = _rand(2 * nv, 12); tau = _rand(_log2(nc), 13); rx = _rand(_log2(nc), 14); rABC = _rand(3, 15)
    tz = ctx.table_upload(rm.to_bytes(z))
    teq = ctx.eq_evals(rm.to_bytes(tau))
    Az, Bz, Cz = ctx.r1cs_multiply(h, tz)
    abc = ctx.r1cs_eval_table(h, rm.to_bytes(rx), *(rm.to_bytes([v]) for v in rABC))
    try:
        mA, mB, mC = rm.multiply_vec(nc, nv, mats, z)
        want = ol.sc_eval_r1cs(rm.to_bytes(rm.eq_evals(tau)), rm.to_bytes(mA), rm.to_bytes(mB), rm.to_bytes(mC))
        assert ctx.sc_eval_r1cs(teq, Az, Bz, Cz) == want
        mabc = rm.eval_table(nc, nv, mats, rx, *rABC)
        assert ctx.sc_eval_quad(tz, abc) == ol.sc_eval_quad(rm.to_bytes(z), rm.to_bytes(mabc))
    finally:
        for t in (tz, teq, Az, Bz, Cz, abc):
            t.free()
        h.free()


def _z_keyless(n, seed):
    rng = np.random.default_rng(seed)
    return rm.random_vals(rng, n).tobytes()


def test_r1cs_keyless_shape(ctx):
    """the bench's synthetic instance: the phase-2 claim identities on the device and sampled rows / columns against the model"""
    nc, nv, mats = rm.keyless_instance(1)
    lx, ly = _log2(nc), _log2(2 * nv)
    h = ctx.r1cs_upload(nc, nv, mats)
    zb = _z_keyless(2 * nv, 2)
    tz = ctx.table_upload(zb)
    rx, ry, rABC = _rand(lx, 3), _rand(ly, 4), _rand(3, 5)
    Az, Bz, Cz = ctx.r1cs_multiply(h, tz)
    abc = ctx.r1cs_eval_table(h, rm.to_bytes(rx), *(rm.to_bytes([v]) for v in rABC))
    ex = ctx.eq_evals(rm.to_bytes(rx)); ey = ctx.eq_evals(rm.to_bytes(ry))
    try:
        # r1csproof.rs:373: <ABC, z> = r_A <eq(rx), Az> + r_B <eq(rx), Bz> + r_C <eq(rx), Cz>
        dots = [int.from_bytes(ctx.table_dot(ex, t), "little") for t in (Az, Bz, Cz)]
        lhs = int.from_bytes(ctx.table_dot(abc, tz), "little")
        assert lhs == sum(r * d for r, d in zip(rABC, dots)) % R
        # <ABC, eq(ry)> = sum_M r_M M(rx, ry)
        ev = rm.from_bytes(b"".join(ctx.r1cs_evaluate(h, rm.to_bytes(rx), rm.to_bytes(ry))))
        assert int.from_bytes(ctx.table_dot(abc, ey), "little") == sum(r * e for r, e in zip(rABC, ev)) % R
        # sampled rows of Az / Bz / Cz (the long row included) against the model
        z_all = np.frombuffer(zb, np.uint8).reshape(-1, 32)
        rng = np.random.default_rng(6)
        sample = np.unique(np.concatenate([rng.integers(0, nc, 2000), [rm.KEYLESS_LONG_ROW[0], rm.KEYLESS_REAL_ROWS - 1, nc - 1]]))
        for m, t in enumerate((Az, Bz, Cz)):
            dev = np.frombuffer(ctx.table_download(t), np.uint8).reshape(-1, 32)
            rows, cols, vals = mats[m]
            sel = np.nonzero(np.isin(rows, sample))[0]
            want = {int(r): 0 for r in sample}
            zs = rm.vals_as_ints(np.ascontiguousarray(z_all[cols[sel]]))
            for r, v, zc in zip(rows[sel], rm.vals_as_ints(np.ascontiguousarray(vals[sel])), zs):
                want[int(r)] = (want[int(r)] + v * zc) % R
            got = {int(r): int.from_bytes(dev[r].tobytes(), "little") for r in sample}
            assert got == want, f"sampled rows of matrix {m}"
        # sampled columns of ABC, the constant column included
        exl = rm.eq_evals(rx)
        dev = np.frombuffer(ctx.table_download(abc), np.uint8).reshape(-1, 32)
        csample = np.unique(np.concatenate([rng.integers(0, 2 * nv, 200), [nv]]))
        want = {int(c): 0 for c in csample}
        for m, (rows, cols, vals) in enumerate(mats):
            sel = np.nonzero(np.isin(cols, csample))[0]
            for r, c, v in zip(rows[sel], cols[sel], rm.vals_as_ints(np.ascontiguousarray(vals[sel]))):
                want[int(c)] = (want[int(c)] + rABC[m] * exl[int(r)] % R * v) % R
        got = {int(c): int.from_bytes(dev[c].tobytes(), "little") for c in csample}
        assert got == want, "sampled columns of ABC"
    finally:
        for t in (tz, Az, Bz, Cz, abc, ex, ey):
            t.free()
        h.free()
