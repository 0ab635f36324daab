"""Pure-int model of MultiSparseMatPolynomialAsDense, the sequential loops of the reference line for line:
  sparse_to_dense_vecs         zeros of length N, then entry i of the matrix at index i                       (sparse_mlpoly_full.rs:89-101)
  AddrTimestamps::new          one audit_ts over the batch; per op: read_ts = audit_ts[addr], audit_ts[addr] += 1   (sparse_mlpoly_full.rs:211-243)
  multi_sparse_to_dense_rep    comb_ops = merge(row addr, row read_ts, col addr, col read_ts, val), comb_mem = row audit ++ col audit
                                                                                                              (sparse_mlpoly_full.rs:120-174, hyrax.rs:237-251)
  deref / hash layer / products the memory-checking sets of Layers::build_hash_layer                         (sparse_mlpoly_full.rs:245-257, 745-796)
A matrix is a triplet (rows, cols, vals) of equally long sequences of ints, in the caller's entry order.
N is the largest next_power_of_two of the entry counts (Rust: next_power_of_two(0) = 1), as the device call defines it."""
R = 0x30644e72e131a029b85045b68181585d2833e84879b9709143e1f593f0000001


def next_power_of_two(n):
    p = 1
    while p < n:
        p *= 2
    return p


def num_ops(mats):
    return max(next_power_of_two(len(rows)) for rows, _, _ in mats)


def num_cells(num_vars_x, num_vars_y):
    return 2 ** num_vars_x if num_vars_x > num_vars_y else 2 ** num_vars_y


def sparse_to_dense_vecs(mat, N):
    rows, cols, vals = mat
    assert N >= len(rows)
    ops_row, ops_col, val = [0] * N, [0] * N, [0] * N
    for i in range(len(rows)):
        ops_row[i] = rows[i]
        ops_col[i] = cols[i]
        val[i] = vals[i] % R
    return ops_row, ops_col, val


def addr_timestamps(cells, N, ops_addr):
    """-> (read_ts per instance, audit_ts)"""
    for item in ops_addr:
        assert len(item) == N
    audit_ts = [0] * cells
    read_ts_vec = []
    for ops_addr_inst in ops_addr:
        read_ts = [0] * N
        for i in range(N):
            addr = ops_addr_inst[i]
            assert addr < cells
            r_ts = audit_ts[addr]
            read_ts[i] = r_ts
            audit_ts[addr] = r_ts + 1
        read_ts_vec.append(read_ts)
    return read_ts_vec, audit_ts


def merge(polys):
    """DensePolynomial::merge: the polynomials end to end, zero-padded to the next power of two"""
    z = []
    for p in polys:
        z += list(p)
    return z + [0] * (next_power_of_two(len(z)) - len(z))


class Dense:
    def __init__(self, num_vars_x, num_vars_y, mats):
        assert len(mats) >= 1
        self.batch = len(mats)
        self.N = num_ops(mats)
        self.cells = num_cells(num_vars_x, num_vars_y)
        vecs = [sparse_to_dense_vecs(m, self.N) for m in mats]
        self.addr = ([v[0] for v in vecs], [v[1] for v in vecs])                    # [side][k][i]
        self.val = [v[2] for v in vecs]
        row = addr_timestamps(self.cells, self.N, self.addr[0])
        col = addr_timestamps(self.cells, self.N, self.addr[1])
        self.read_ts = (row[0], col[0])                                             # [side][k][i]
        self.audit_ts = (row[1], col[1])                                            # [side][a]
        self.comb_ops = merge(self.addr[0] + self.read_ts[0] + self.addr[1] + self.read_ts[1] + self.val)
        self.comb_mem = self.audit_ts[0] + self.audit_ts[1]

    def ops_start(self, group, j):
        """where polynomial j of group 0..4 (row addr, row read_ts, col addr, col read_ts, val) starts in comb_ops"""
        return (group * self.batch + j) * self.N


def deref(addr, mem):
    return [mem[a] for a in addr]


def hash_set(addr, val, ts, r_hash, r_multiset):
    """Layers::build_hash_layer: (ts * r_hash^2 + val * r_hash + addr) - r_multiset per element"""
    return [(t * r_hash % R * r_hash + v * r_hash + a - r_multiset) % R for a, v, t in zip(addr, val, ts)]


def product(v):
    p = 1
    for x in v:
        p = p * x % R
    return p


def memory_products(d, side, mem, r_hash, r_multiset):
    """-> (prod init, [prod read_k], [prod write_k], prod audit) of one side over the memory `mem` (cells entries)"""
    cells = list(range(d.cells))
    init = product(hash_set(cells, mem, [0] * d.cells, r_hash, r_multiset))
    audit = product(hash_set(cells, mem, d.audit_ts[side], r_hash, r_multiset))
    reads, writes = [], []
    for k in range(d.batch):
        a, ts = d.addr[side][k], d.read_ts[side][k]
        v = deref(a, mem)
        reads.append(product(hash_set(a, v, ts, r_hash, r_multiset)))
        writes.append(product(hash_set(a, v, [t + 1 for t in ts], r_hash, r_multiset)))
    return init, reads, writes, audit


def eq_evals(r):
    ev = [1]
    for rj in r:
        nxt = []
        for e in ev:
            hi = e * rj % R
            nxt += [(e - hi) % R, hi]
        ev = nxt
    return ev


def evaluate(z, r):
    """DensePolynomial::evaluate: <z, eq(r)>"""
    return sum(a * b for a, b in zip(z, eq_evals(r))) % R


def numpy_expectation(num_vars_x, num_vars_y, mats):
    """The same arrays with numpy, for shapes the loops above are too slow for: a stable argsort of the batch * N addresses of a side gives
    the ranks inside each run of equal addresses, bincount the audit counts.
    -> (N, cells, addr[side] (batch, N) uint32, read_ts[side] (batch, N) uint32, audit_ts[side] (cells,) uint32)"""
    import numpy as np
    N = max(next_power_of_two(len(m[0])) for m in mats)
    cells = num_cells(num_vars_x, num_vars_y)
    addr, read_ts, audit = [], [], []
    for side in (0, 1):
        a = np.zeros((len(mats), N), np.uint32)
        for k, m in enumerate(mats):
            a[k, :len(m[side])] = np.asarray(m[side], np.uint32)
        flat = a.reshape(-1)
        order = np.argsort(flat, kind="stable")
        s = flat[order]
        pos = np.arange(len(s), dtype=np.int64)
        head = np.ones(len(s), bool); head[1:] = s[1:] != s[:-1]
        start = np.maximum.accumulate(np.where(head, pos, 0))
        ts = np.empty(len(s), np.uint32); ts[order] = (pos - start).astype(np.uint32)
        addr.append(a); read_ts.append(ts.reshape(len(mats), N)); audit.append(np.bincount(flat, minlength=cells).astype(np.uint32))
    return N, cells, addr, read_ts, audit
