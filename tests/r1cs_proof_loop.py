"""R1CSProof::prove (r1csproof.rs:241-459) assembled by the caller from the entry points that existed before sbn_r1cs_proof_prove: the "loop" leg
of tools/bench_r1cs_proof.py and of tests/test_gpu_r1cs_proof.py.  The caller runs the transcript (sbn_transcript_*), builds z on the host and
uploads it, does the Fr arithmetic of the Σ-protocols itself and fetches each of their 14 group elements with a one-row sbn_commit_rows over
a gens_1 handle that carries a lookup table."""
import numpy as np

R_MOD = 0x30644e72e131a029b85045b68181585d2833e84879b9709143e1f593f0000001


def sb(x):
    return int(x % R_MOD).to_bytes(32, "little")


def ib(b):
    return int.from_bytes(b, "little")


def random_instance(nc, nv, seed, per_row=3):
    """three sparse matrices with numpy, not satisfiable: `per_row` entries per row and matrix over the 2 num_vars columns
    -> [(rows, cols, vals)] with uint32 rows / cols and (nnz, 32) uint8 values, as Context.r1cs_upload takes them"""
    import r1cs_model as rm
    rng = np.random.default_rng(seed)
    mats = []
    for _ in range(3):
        rows = np.repeat(np.arange(nc, dtype=np.uint32), per_row)
        cols = rng.integers(0, 2 * nv, len(rows), dtype=np.uint32)
        mats.append((rows, cols, rm.random_vals(rng, len(rows))))
    return mats


class LoopGens:
    """the handles the loop leg needs beside gens_pc: gens_n and gens_1 from sbn_bases_split_at, gens_1 with a lookup table"""

    def __init__(self, ctx, gens_pc, R):
        self.ctx = ctx
        self.gens_n, self.gens_1 = ctx.bases_split_at(gens_pc, R)
        ctx.bases_precompute(self.gens_1, 64 << 20)

    def free(self):
        self.gens_n.free(); self.gens_1.free()


def prove_loop(sbn, ctx, inst, vars_t, vars_bytes, input_bytes, gens_pc, lg_, gens_3, gens_4, rnd, tr):
    """-> (proof bytes, rx, ry) in sbn_r1cs_proof_prove's layout; rnd: bytes in its layout; vars_bytes: the witness as canonical bytes"""
    nc, nv = inst.num_cons, inst.num_vars
    nx, ell = nc.bit_length() - 1, nv.bit_length() - 1
    ny, ml = ell + 1, ell // 2
    lg = ell - ml
    L, R = 1 << ml, 1 << lg
    g1 = lg_.gens_1
    pos = [0]

    def take(k):
        out = rnd[32 * pos[0]:32 * (pos[0] + k)]
        pos[0] += k
        return out

    def point(label, p32):
        tr.append_message(label, p32)

    def com1(v, b):
        return sbn.g1_compress(ctx.commit_rows(g1, sb(v), sb(b), 1, 1)[0])

    tr.append_message(b"protocol-name", b"R1CS proof")
    for i in range(len(input_bytes) // 32):
        tr.append_message(b"input", input_bytes[32 * i:32 * i + 32])
    poly_blinds = take(L)
    comm_vars = sbn.g1_compress(ctx.commit_table(lg_.gens_n, vars_t, poly_blinds, L, R)[0])
    tr.append_message(b"poly_commitment", b"poly_commitment_begin")
    for i in range(L):
        point(b"poly_commitment_share", comm_vars[32 * i:32 * i + 32])
    tr.append_message(b"poly_commitment", b"poly_commitment_end")
    tau = b"".join(tr.challenge_scalar(b"challenge_tau") for _ in range(nx))
    z_host = bytes(vars_bytes) + sb(1) + bytes(input_bytes) + bytes(32 * (nv - 1 - len(input_bytes) // 32))
    tabs = []
    try:
        eq = ctx.eq_evals(tau); tabs.append(eq)
        z = ctx.table_upload(z_host); tabs.append(z)
        Az, Bz, Cz = ctx.r1cs_multiply(inst, z); tabs += [Az, Bz, Cz]
        sc1, rx, fin1, blind_post1 = ctx.zk_sumcheck_prove_r1cs(eq, Az, Bz, Cz, g1, gens_4, sb(0), sb(0), take(8 * nx), tr)
        tau_c, Az_c, Bz_c, Cz_c = (ib(fin1[32 * i:32 * i + 32]) for i in range(4))
        Az_b, Bz_b, Cz_b, prod_b = (ib(x) for x in (take(1), take(1), take(1), take(1)))
        t1, t2 = ib(take(1)), ib(take(1))
        tr.append_message(b"protocol-name", b"knowledge proof")
        comm_Cz, k_alpha = com1(Cz_c, Cz_b), com1(t1, t2)
        point(b"C", comm_Cz); point(b"alpha", k_alpha)
        c = ib(tr.challenge_scalar(b"c"))
        pok = k_alpha + sb(Cz_c * c + t1) + sb(Cz_b * c + t2)
        b1, b2, b3, b4, b5 = (ib(take(1)) for _ in range(5))
        prod = Az_c * Bz_c % R_MOD
        tr.append_message(b"protocol-name", b"product proof")
        X, Y, Z = com1(Az_c, Az_b), com1(Bz_c, Bz_b), com1(prod, prod_b)
        p_alpha, p_beta, p_delta = com1(b1, b2), com1(b3, b4), com1(b3 * Az_c, b3 * Az_b + b5)
        for label, p in ((b"X", X), (b"Y", Y), (b"Z", Z), (b"alpha", p_alpha), (b"beta", p_beta), (b"delta", p_delta)):
            point(label, p)
        c = ib(tr.challenge_scalar(b"c"))
        pok += p_alpha + p_beta + p_delta + sb(b1 + c * Az_c) + sb(b2 + c * Az_b) + sb(b3 + c * Bz_c) + sb(b4 + c * Bz_b) + sb(b5 + c * (prod_b - Az_b * Bz_c))
        for label, p in ((b"comm_Az_claim", X), (b"comm_Bz_claim", Y), (b"comm_Cz_claim", comm_Cz), (b"comm_prod_Az_Bz_claims", Z)):
            point(label, p)
        blind_expected1 = tau_c * (prod_b - Cz_b) % R_MOD
        claim_post1 = (prod - Cz_c) * tau_c % R_MOD
        r1 = ib(take(1))
        tr.append_message(b"protocol-name", b"equality proof")
        C1, C2, e_alpha = com1(claim_post1, blind_expected1), com1(claim_post1, ib(blind_post1)), com1(0, r1)
        point(b"C1", C1); point(b"C2", C2); point(b"alpha", e_alpha)
        c = ib(tr.challenge_scalar(b"c"))
        eq1 = e_alpha + sb(c * (blind_expected1 - ib(blind_post1)) + r1)
        rA, rB, rC = (tr.challenge_scalar(l) for l in (b"challenge_Az", b"challenge_Bz", b"challenge_Cz"))
        claim2 = ib(rA) * Az_c + ib(rB) * Bz_c + ib(rC) * Cz_c
        blind2 = ib(rA) * Az_b + ib(rB) * Bz_b + ib(rC) * Cz_b
        abc = ctx.r1cs_eval_table(inst, rx, rA, rB, rC); tabs.append(abc)
        sc2, ry, fin2, blind_post2 = ctx.zk_sumcheck_prove_quad(z, abc, g1, gens_3, sb(claim2), sb(blind2), take(7 * ny), tr)
        eval_vars = ctx.table_evaluate(vars_t, ry[32:])
        blind_eval = take(1)
        opening, _, cy = ctx.polyeval_prove(gens_pc, vars_t, ry[32:], eval_vars, take(3 + 2 * lg), tr, blinds=poly_blinds, blind_Zr=blind_eval)
        z_c, abc_c = ib(fin2[:32]), ib(fin2[32:])
        blind_expected2 = abc_c * ((1 - ib(ry[:32])) * ib(blind_eval) % R_MOD) % R_MOD
        claim_post2 = z_c * abc_c % R_MOD
        r2 = ib(take(1))
        tr.append_message(b"protocol-name", b"equality proof")
        C1, C2, e_alpha = com1(claim_post2, blind_expected2), com1(claim_post2, ib(blind_post2)), com1(0, r2)
        point(b"C1", C1); point(b"C2", C2); point(b"alpha", e_alpha)
        c = ib(tr.challenge_scalar(b"c"))
        eq2 = e_alpha + sb(c * (blind_expected2 - ib(blind_post2)) + r2)
    finally:
        for t in tabs:
            t.free()
    assert 32 * pos[0] == len(rnd)
    return comm_vars + sc1 + X + Y + comm_Cz + Z + pok + eq1 + sc2 + sbn.g1_compress(cy) + opening + eq2, rx, ry
