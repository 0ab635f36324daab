"""SparseMatPolyEvalProof::prove of the KZG build (sparse_mlpoly_full.rs:1757-1813) assembled by the caller from the entry points that existed
before sbn_sparse_eval_prove_kzg: the "loop" leg of tools/bench_sparse_eval_kzg.py and of tests/test_gpu_sparse_eval_kzg.py.  As
tests/sparse_eval_loop.py (whose helpers it shares), with the two places the KZG build differs in: the derefs commitment is sbn_kzg_commit of
the gathered, merged table and the derefs opening is sbn_kzg_open at kzg_eval_point — both on the FULL padded length n_d = npo2(2 b) N, which
is what pins the one call's stop at the non-zero prefix."""
from sparse_eval_loop import R_MOD, LoopGens, _derefs, _dotp_halves, evals_of, ib, npo2, random_mats, sb  # noqa: F401


def prove_loop(sbn, ctx, dense, rx, ry, evals, gens_ops, gens_mem, srs, lg, rnd, tr):
    """-> proof bytes in sbn_sparse_eval_prove_kzg's layout; rx, ry, evals, rnd: bytes in its layouts; lg: LoopGens(ctx, None, 0, N); `tr` moves on"""
    b, N, cells = dense.batch, dense.num_ops, dense.num_cells
    n, m = N.bit_length() - 1, cells.bit_length() - 1
    ell_d, ell_o, ell_m = n + npo2(2 * b).bit_length() - 1, n + npo2(5 * b).bit_length() - 1, m + 1
    lgs = {k: e - e // 2 for k, e in (("derefs", ell_d), ("ops", ell_o), ("mem", ell_m))}
    n_d = 1 << ell_d
    pos = [0]

    def take(k):
        out = rnd[32 * pos[0]:32 * (pos[0] + k)]
        pos[0] += k
        return out
    rnds = {k: take(3 + 2 * lgs[k]) for k in ("ops", "mem")}
    name = lambda s: tr.append_message(b"protocol-name", s)
    held = []
    try:
        name(b"Sparse polynomial evaluation proof")
        mem_rx, mem_ry, derefs = _derefs(ctx, dense, rx, ry)
        held += [mem_rx, mem_ry, derefs]
        xy, inf = ctx.kzg_commit(srs, derefs, n_d)                # KZGPolyCommitment::commit on all n_d coefficients (kzg.rs:386-397)
        comm = sbn.g1_compress(bytes(64) if inf else xy)
        tr.append_message(b"derefs_commitment", b"begin_derefs_commitment")
        tr.append_message(b"comm_poly_row_col_ops_val", comm)
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
        name(b"Derefs evaluation proof (KZG)")                    # DerefsEvalProof::prove (:503-550)
        pad = lambda e: e + bytes(32 * (npo2(len(e) // 32) - len(e) // 32))
        pe = [ib(pad(e_der)[32 * i:32 * i + 32]) for i in range(len(pad(e_der)) // 32)]
        for x in pe:
            tr.append_scalar(b"evals_ops_val", sb(x))
        ch = [ib(tr.challenge_scalar(b"challenge_combine_n_to_one")) for _ in range(len(pe).bit_length() - 1)]
        for i in range(len(ch) - 1, -1, -1):                       # bound_poly_var_bot from the last challenge down
            pe = [(pe[2 * k] + ch[i] * (pe[2 * k + 1] - pe[2 * k])) % R_MOD for k in range(len(pe) // 2)]
        tr.append_scalar(b"joint_claim_eval", sb(pe[0]))
        z = tr.challenge_scalar(b"kzg_eval_point")
        ev, pxy, pinf = ctx.kzg_open(srs, derefs, n_d, z)         # KZGProof::prove on all n_d coefficients (kzg.rs:174-192)
        o_der = sbn.g1_compress(bytes(64) if pinf else pxy) + ev
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
