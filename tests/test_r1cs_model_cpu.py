"""CPU: the pure-int model of the R1CS loops (r1cs_model.py) against itself and the shape of the synthetic keyless instance the GPU
test and tools/bench_r1cs.py share.  The model's three loops must agree on the identities the prover relies on (r1csproof.rs:373)."""
import random

import numpy as np

import r1cs_model as rm

R = rm.R


def _mats(nc, nv, seed):
    rng = random.Random(seed)
    out = []
    for _ in range(3):
        n = rng.randrange(1, 3 * nc)
        out.append(([rng.randrange(nc) for _ in range(n)], [rng.randrange(2 * nv + 2) for _ in range(n)], [rng.randrange(R) for _ in range(n)]))
    return out


def test_model_identities():
    nc, nv = 16, 8
    mats = _mats(nc, nv, 1)
    rng = random.Random(2)
    z = [rng.randrange(R) for _ in range(2 * nv)]
    rx = [rng.randrange(R) for _ in range(4)]; ry = [rng.randrange(R) for _ in range(4)]
    rA, rB, rC = (rng.randrange(R) for _ in range(3))
    ex, ey = rm.eq_evals(rx), rm.eq_evals(ry)
    Az, Bz, Cz = rm.multiply_vec(nc, nv, mats, z)
    abc = rm.eval_table(nc, nv, mats, rx, rA, rB, rC)
    dot = lambda a, b: sum(x * y for x, y in zip(a, b)) % R
    assert dot(abc, z) == (rA * dot(ex, Az) + rB * dot(ex, Bz) + rC * dot(ex, Cz)) % R
    ev = rm.evaluate(nc, nv, mats, rx, ry)
    assert dot(abc, ey) == (rA * ev[0] + rB * ev[1] + rC * ev[2]) % R
    # at a Boolean point the evaluation is the sum of the entries of one cell
    cell = rm.evaluate(nc, nv, mats, [0, 0, 1, 1], [0, 0, 1, 0])
    for m, (rows, cols, vals) in enumerate(mats):
        assert cell[m] == sum(v for r, c, v in zip(rows, cols, vals) if r == 3 and c == 2) % R


def test_eq_evals_order():
    r = [3, 5]
    assert rm.eq_evals(r) == [(1 - 3) * (1 - 5) % R, (1 - 3) * 5 % R, 3 * (1 - 5) % R, 15]


def test_keyless_instance_shape():
    nc, nv, mats = rm.keyless_instance(1)
    assert nc == nv == 1 << 20
    assert tuple(len(m[0]) for m in mats) == rm.KEYLESS_NNZ and sum(rm.KEYLESS_NNZ) == 7_132_133
    for rows, cols, vals in mats:
        assert rows.dtype == np.uint32 and cols.dtype == np.uint32 and vals.shape == (len(rows), 32)
        assert int(rows.max()) < rm.KEYLESS_REAL_ROWS and int(cols.max()) < 2 * nv
    a_rows, a_cols, a_vals = mats[0]
    assert int(np.bincount(a_rows).max()) >= 1 << 16
    const_rows = np.unique(a_rows[a_cols == nv])
    assert abs(len(const_rows) - rm.KEYLESS_REAL_ROWS // 2) < rm.KEYLESS_REAL_ROWS // 50
    ints = rm.vals_as_ints(np.ascontiguousarray(a_vals[:4000]))
    assert all(v < R for v in ints)
    ones, rm1 = sum(v == 1 for v in ints), sum(v == R - 1 for v in ints)
    assert 800 < ones < 1200 and 800 < rm1 < 1200
