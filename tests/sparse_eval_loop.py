"""SparseMatPolyEvalProof::prove (sparse_mlpoly_full.rs:1700-1755) assembled by the caller from the entry points that existed before
sbn_sparse_eval_prove: the "loop" leg of tools/bench_sparse_eval.py and of tests/test_gpu_sparse_eval.py.  The caller runs the transcript
(sbn_transcript_*) between the calls, does equalize, the framing lines, the claim appends and the subset / split checks itself, and lays the
proof out as include/sbn254.h describes.

DotProductCircuit::evaluate of a split half has no entry point of its own in the earlier interface: the left half's sum is the e0 of
sbn_sc_eval_cubic on the three whole tables (the round-0 value at 0 sums the low half), the right half's the same on copies rotated by half
their length, which sbn_gather_merge makes from an index array uploaded once."""
import numpy as np

R_MOD = 0x30644e72e131a029b85045b68181585d2833e84879b9709143e1f593f0000001


def sb(x):
    return int(x % R_MOD).to_bytes(32, "little")


def ib(b):
    return int.from_bytes(b, "little")


def npo2(n):
    p = 1
    while p < n:
        p *= 2
    return p


def random_mats(nx, ny, N, batch, seed):
    """`batch` matrices of N entries with numpy: uint32 rows / cols, (N, 32) uint8 canonical values, as Context.dense_build takes them"""
    import r1cs_model as rm
    rng = np.random.default_rng(seed)
    return [(rng.integers(0, 1 << nx, N, dtype=np.uint32), rng.integers(0, 1 << ny, N, dtype=np.uint32), rm.random_vals(rng, N)) for _ in range(batch)]


def evals_of(sbn, ctx, dense, rx, ry):
    """the true evaluations M_k(rx, ry), through the device: <val_k, eq(rx)[row_k] * eq(ry)[col_k]> as the sum of both halves' e0"""
    lg = LoopGens(ctx, None, 0, dense.num_ops)
    try:
        return b"".join(sb(ib(l) + ib(r)) for l, r in _dotp_halves(ctx, dense, lg, *_derefs(ctx, dense, rx, ry), free=True))
    finally:
        lg.free()


class LoopGens:
    """what the loop leg holds beside the three generator handles: gens_derefs' first R generators with h (sbn_bases_split_at) for the
    derefs commitment, and the device index array of the rotation by N / 2"""

    def __init__(self, ctx, gens_derefs, R_derefs, N):
        self.ctx = ctx
        self.gens_n = self.rest = None
        if gens_derefs is not None:
            self.gens_n, self.rest = ctx.bases_split_at(gens_derefs, R_derefs)
        rot = ((np.arange(N, dtype=np.uint32) + N // 2) % N).astype(np.uint32)
        self.rot = ctx.dev_alloc(4 * N)
        ctx.dev_upload(self.rot, rot.tobytes())

    def free(self):
        for h in (self.gens_n, self.rest):
            if h is not None:
                h.free()
        self.ctx.dev_free(self.rot)


def _equalize(rx, ry):
    nx, ny = len(rx) // 32, len(ry) // 32
    m = max(nx, ny)
    return bytes(32 * (m - nx)) + rx, bytes(32 * (m - ny)) + ry


def _derefs(ctx, dense, rx, ry):
    """-> (mem_rx, mem_ry, derefs): the two eq tables and the gathered, merged table"""
    b, N = dense.batch, dense.num_ops
    rx_ext, ry_ext = _equalize(rx, ry)
    mem_rx, mem_ry = ctx.eq_evals(rx_ext), ctx.eq_evals(ry_ext)
    derefs = ctx.gather_merge([mem_rx] * b + [mem_ry] * b, [dense.addr_dev(0, k) for k in range(b)] + [dense.addr_dev(1, k) for k in range(b)], N)
    return mem_rx, mem_ry, derefs


def _dotp_halves(ctx, dense, lg, mem_rx, mem_ry, derefs, free=False):
    """[(eval_dotp_left, eval_dotp_right)] per matrix"""
    b, N = dense.batch, dense.num_ops
    out = []
    for k in range(b):
        tabs = [ctx.table_slice(derefs, k * N, N), ctx.table_slice(derefs, (b + k) * N, N), dense.ops_slice(4, k)]
        left = ctx.sc_eval_cubic(*tabs)[:32]
        rot = [ctx.gather_merge([t], [lg.rot], N) for t in tabs]
        right = ctx.sc_eval_cubic(*rot)[:32]
        for t in tabs + rot:
            t.free()
        out.append((left, right))
    if free:
        for t in (derefs, mem_rx, mem_ry):
            t.free()
    return out


def prove_loop(sbn, ctx, dense, rx, ry, evals, gens_ops, gens_mem, gens_derefs, lg, rnd, tr):
    """-> proof bytes in sbn_sparse_eval_prove's layout; rx, ry, evals, rnd: bytes in its layouts; `tr` (sbn.Transcript) moves on"""
    b, N, cells = dense.batch, dense.num_ops, dense.num_cells
    n, m = N.bit_length() - 1, cells.bit_length() - 1
    ell_d, ell_o, ell_m = n + npo2(2 * b).bit_length() - 1, n + npo2(5 * b).bit_length() - 1, m + 1
    lgs = {k: e - e // 2 for k, e in (("derefs", ell_d), ("ops", ell_o), ("mem", ell_m))}
    Ld, Rd = 1 << (ell_d // 2), 1 << lgs["derefs"]
    pos = [0]

    def take(k):
        out = rnd[32 * pos[0]:32 * (pos[0] + k)]
        pos[0] += k
        return out
    rnds = {k: take(3 + 2 * lgs[k]) for k in ("derefs", "ops", "mem")}
    name = lambda s: tr.append_message(b"protocol-name", s)
    held = []
    try:
        name(b"Sparse polynomial evaluation proof")
        mem_rx, mem_ry, derefs = _derefs(ctx, dense, rx, ry)
        held += [mem_rx, mem_ry, derefs]
        xy, _ = ctx.commit_table(lg.gens_n, derefs, None, Ld, Rd)
        comm = sbn.g1_compress(xy)
        tr.append_message(b"derefs_commitment", b"begin_derefs_commitment")
        tr.append_message(b"comm_poly_row_col_ops_val", b"poly_commitment_begin")
        for i in range(Ld):
            tr.append_message(b"poly_commitment_share", comm[32 * i:32 * i + 32])
        tr.append_message(b"comm_poly_row_col_ops_val", b"poly_commitment_end")
        tr.append_message(b"derefs_commitment", b"end_derefs_commitment")
        r_hash, r_multiset = tr.challenge_scalar(b"challenge_r_hash"), tr.challenge_scalar(b"challenge_r_hash")

        # PolyEvalNetwork::new
        val = [[ctx.table_slice(derefs, (side * b + k) * N, N) for k in range(b)] for side in (0, 1)]
        held += val[0] + val[1]
        sets = {}
        for side, mem in ((0, mem_rx), (1, mem_ry)):
            sets[side, "init"], sets[side, "audit"] = ctx.hash_layer_pair(None, mem, None, 0, dense.audit_ts_dev(side), 0, r_hash, r_multiset)
            rw = [ctx.hash_layer_pair(dense.addr_dev(side, k), val[side][k], dense.read_ts_dev(side, k), 0, dense.read_ts_dev(side, k), 1, r_hash, r_multiset)
                  for k in range(b)]
            sets[side, "read"], sets[side, "write"] = [p[0] for p in rw], [p[1] for p in rw]
        ops_in = sets[0, "read"] + sets[0, "write"] + sets[1, "read"] + sets[1, "write"]
        mem_in = [sets[0, "init"], sets[0, "audit"], sets[1, "init"], sets[1, "audit"]]
        held += ops_in + mem_in
        ops_layers = ctx.product_circuit_many(ops_in)
        mem_layers = ctx.product_circuit_many(mem_in)
        held += [t for c in ops_layers + mem_layers for t in c]

        # PolyEvalNetworkProof::prove (the same protocol name again, :1555), ProductLayerProof::prove
        name(b"Sparse polynomial evaluation proof")
        name(b"Sparse polynomial product layer proof")
        tops = ctx.table_read0_many([c[-1] for c in ops_layers + mem_layers])
        o_tops, m_tops = tops[:4 * b], tops[4 * b:]

        def prod(xs):
            p = 1
            for x in xs:
                p = p * ib(x) % R_MOD
            return p
        rows = []
        for side, nm in ((0, b"row"), (1, b"col")):
            init, audit = m_tops[2 * side], m_tops[2 * side + 1]
            read, write = o_tops[2 * b * side:2 * b * side + b], o_tops[2 * b * side + b:2 * b * side + 2 * b]
            if ib(init) * prod(write) % R_MOD != prod(read) * ib(audit) % R_MOD:
                raise AssertionError("subset check (sparse_mlpoly_full.rs:1324 / :1339)")
            tr.append_scalar(b"claim_" + nm + b"_eval_init", init)
            for x in read:
                tr.append_scalar(b"claim_" + nm + b"_eval_read", x)
            for x in write:
                tr.append_scalar(b"claim_" + nm + b"_eval_write", x)
            tr.append_scalar(b"claim_" + nm + b"_eval_audit", audit)
            rows.append(init + b"".join(read) + b"".join(write) + audit)
        halves = _dotp_halves(ctx, dense, lg, mem_rx, mem_ry, derefs)
        for k, (l, r) in enumerate(halves):
            tr.append_scalar(b"claim_eval_dotp_left", l); tr.append_scalar(b"claim_eval_dotp_right", r)
            if (ib(l) + ib(r)) % R_MOD != ib(evals[32 * k:32 * k + 32]):
                raise AssertionError("eval_dotp_left + eval_dotp_right != evals[%d] (sparse_mlpoly_full.rs:1366)" % k)
        eval_val = b"".join(l for l, _ in halves) + b"".join(r for _, r in halves)
        wgt = [dense.ops_slice(4, k) for k in range(b)]
        held += wgt
        dotps = []
        for k in range(b):
            hl, hr, hw = ctx.table_halves(val[0][k]), ctx.table_halves(val[1][k]), ctx.table_halves(wgt[k])
            held += list(hl) + list(hr) + list(hw)
            dotps += [(hl[0], hr[0], hw[0]), (hl[1], hr[1], hw[1])]
        layers_of = lambda ins, circ: [[ins[i]] + circ[i][:-1] for i in range(len(ins))]
        p_ops = ctx.product_proof_prove(layers_of(ops_in, ops_layers), dotps, tr)
        p_mem = ctx.product_proof_prove(layers_of(mem_in, mem_layers), [], tr)
        rand_ops, rand_mem = p_ops[2], p_mem[2]

        # HashLayerProof::prove
        name(b"Sparse polynomial hash layer proof")
        e_der = ctx.table_evaluate_many(val[0] + val[1], rand_ops)
        name(b"Derefs evaluation proof")
        pad = lambda e: e + bytes(32 * (npo2(len(e) // 32) - len(e) // 32))
        o_der = ctx.joint_opening_prove(gens_derefs, derefs, pad(e_der), (b"evals_ops_val", b"challenge_combine_n_to_one", b"joint_claim_eval"), rand_ops, rnds["derefs"], tr)[2]
        grp = [[dense.ops_slice(g, k) for k in range(b)] for g in range(5)]
        held += [t for g in grp for t in g]
        e_ops = ctx.table_evaluate_many([t for g in grp for t in g], rand_ops)
        mem_views = [ctx.table_slice(dense.comb_mem, 0, cells), ctx.table_slice(dense.comb_mem, cells, cells)]
        held += mem_views
        e_mem = ctx.table_evaluate_many(mem_views, rand_mem)
        o_ops = ctx.joint_opening_prove(gens_ops, dense.comb_ops, pad(e_ops), (b"claim_evals_ops", b"challenge_combine_n_to_one", b"joint_claim_eval_ops"), rand_ops, rnds["ops"], tr)[2]
        o_mem = ctx.joint_opening_prove(gens_mem, dense.comb_mem, e_mem, (b"claim_evals_mem", b"challenge_combine_two_to_one", b"joint_claim_eval_mem"), rand_mem, rnds["mem"], tr)[2]
        B = 32 * b
        hl_row = e_ops[:2 * B] + e_mem[:32]
        hl_col = e_ops[2 * B:4 * B] + e_mem[32:]
        return (comm + rows[0] + rows[1] + eval_val + p_mem[0] + p_mem[1] + p_ops[0] + p_ops[1] + hl_row + hl_col + e_ops[4 * B:] + e_der + o_ops + o_mem + o_der)
    finally:
        for t in reversed(held):                                # views before what they look into
            t.free()
