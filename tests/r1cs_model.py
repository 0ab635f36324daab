"""Pure-int model of the reference's three loops over the sparse R1CS matrices, written from their semantics:
  multiply_vec       Az[row] += val * z[col] over every entry with col < len(z)                       (r1cs.rs:132-146)
  eval_table         r_A evals_A + r_B evals_B + r_C evals_C, evals_M[col] += eq(rx)[row] * val      (r1cs.rs:148-163, r1csproof.rs:376-387)
  evaluate           M(rx, ry) = sum val * eq(rx)[row] * eq(ry)[col]                                  (r1cs.rs:126-129)
A matrix is a triplet (rows, cols, vals) of equally long sequences of ints; columns >= 2 num_vars are skipped by all three loops.
Also the synthetic keyless-shaped instance that tools/bench_r1cs.py and tests/test_gpu_r1cs.py share."""
import numpy as np

R = 0x30644e72e131a029b85045b68181585d2833e84879b9709143e1f593f0000001


def to_bytes(vals):
    return b"".join((v % R).to_bytes(32, "little") for v in vals)


def from_bytes(b):
    return [int.from_bytes(b[i:i + 32], "little") for i in range(0, len(b), 32)]


def eq_evals(r):
    """EqPolynomial::evals: entry i = prod_j (r_j if bit j of i, counted from the top, is set else 1 - r_j)"""
    ev = [1]
    for rj in r:
        nxt = []
        for e in ev:
            hi = e * rj % R
            nxt += [(e - hi) % R, hi]
        ev = nxt
    return ev


def multiply_vec(num_cons, num_vars, mats, z):
    assert len(z) == 2 * num_vars
    out = []
    for rows, cols, vals in mats:
        y = [0] * num_cons
        for r, c, v in zip(rows, cols, vals):
            if c < 2 * num_vars:
                y[r] = (y[r] + v * z[c]) % R
        out.append(y)
    return tuple(out)


def eval_table(num_cons, num_vars, mats, rx, rA, rB, rC):
    ex = eq_evals(rx)
    assert len(ex) == num_cons
    t = [0] * (2 * num_vars)
    for rm, (rows, cols, vals) in zip((rA, rB, rC), mats):
        for r, c, v in zip(rows, cols, vals):
            if c < 2 * num_vars:
                t[c] = (t[c] + rm * ex[r] % R * v) % R
    return t


def evaluate(num_cons, num_vars, mats, rx, ry):
    ex, ey = eq_evals(rx), eq_evals(ry)
    assert len(ex) == num_cons and len(ey) == 2 * num_vars
    out = []
    for rows, cols, vals in mats:
        s = 0
        for r, c, v in zip(rows, cols, vals):
            if c < 2 * num_vars:
                s = (s + v * ex[r] % R * ey[c]) % R
        out.append(s)
    return tuple(out)


def ark_mont(v):
    """ark-ff's in-memory Montgomery form (R = 2^256) of a canonical value"""
    return (v << 256) % R


# ---- the synthetic keyless-shaped instance -------------------------------------------------------------------------------------
KEYLESS_LOG = 20
KEYLESS_REAL_ROWS = 1_040_083
KEYLESS_NNZ = (3_151_183, 1_040_083, 2_940_867)
KEYLESS_LONG_ROW = (0, 1 << 16)          # matrix A, row 0: 2^16 entries


def random_vals(rng, n):
    """n values as an (n, 32) uint8 array: about 1/4 equal to 1, 1/4 equal to r - 1, the rest uniform below 2^253"""
    limbs = rng.integers(0, 2**64, size=(n, 4), dtype=np.uint64)
    limbs[:, 3] &= np.uint64((1 << 61) - 1)
    kind = rng.integers(0, 4, size=n)
    one = np.array([1, 0, 0, 0], dtype=np.uint64)
    rm1 = np.array([(R - 1) >> (64 * k) & (2**64 - 1) for k in range(4)], dtype=np.uint64)
    limbs[kind == 0] = one
    limbs[kind == 1] = rm1
    return limbs.view(np.uint8).reshape(n, 32)


def keyless_instance(seed=1):
    """num_cons = num_vars = 2^20; nnz A / B / C = 3,151,183 / 1,040,083 / 2,940,867; rows from 1,040,083 on empty; about half of A's
    real rows hold an entry in the constant column (z[num_vars]); row 0 of A has 2^16 entries.  Triplets in random order.
    Returns (num_cons, num_vars, [(rows, cols, vals) x 3]) with uint32 rows / cols and (nnz, 32) uint8 values."""
    rng = np.random.default_rng(seed)
    n = 1 << KEYLESS_LOG
    real, nz = KEYLESS_REAL_ROWS, 2 * n
    # A: the long row, the constant column in half of the real rows, the rest spread over the real rows
    long_r, long_n = KEYLESS_LONG_ROW
    const_rows = rng.choice(real, size=real // 2, replace=False).astype(np.uint32)
    rest = KEYLESS_NNZ[0] - long_n - len(const_rows)
    a_rows = np.concatenate([np.full(long_n, long_r, np.uint32), const_rows, rng.integers(0, real, rest, dtype=np.uint32)])
    a_cols = np.concatenate([rng.integers(0, nz, long_n, dtype=np.uint32), np.full(len(const_rows), n, np.uint32),
                             rng.integers(0, nz, rest, dtype=np.uint32)])
    # B: one entry per real row; C: spread over the real rows
    b_rows = np.arange(real, dtype=np.uint32)
    b_cols = rng.integers(0, nz, real, dtype=np.uint32)
    c_rows = rng.integers(0, real, KEYLESS_NNZ[2], dtype=np.uint32)
    c_cols = rng.integers(0, nz, KEYLESS_NNZ[2], dtype=np.uint32)
    mats = []
    for rows, cols in ((a_rows, a_cols), (b_rows, b_cols), (c_rows, c_cols)):
        perm = rng.permutation(len(rows))
        mats.append((np.ascontiguousarray(rows[perm]), np.ascontiguousarray(cols[perm]), random_vals(rng, len(rows))))
    return n, n, mats


def vals_as_ints(vals):
    """(n, 32) uint8 -> list of ints"""
    w = vals.view(np.uint64).reshape(-1, 4)
    return [int(a) | int(b) << 64 | int(c) << 128 | int(d) << 192 for a, b, c, d in w]
