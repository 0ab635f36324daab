// abi_sparse_eval.inc — C ABI: SparseMatPolyEvalProof::prove in ONE call: sbn_sparse_eval_prove (sparse_mlpoly_full.rs:1700-1755, the Hyrax build) and
// sbn_sparse_eval_prove_kzg (:1757-1813, --features kzg).  The two builds share sparse_eval_locked; where the KZG build differs is listed below.
// sbn_sparse_eval_prove composes, on one working copy of the caller's Merlin transcript, the bodies of the calls that already hold its parts:
//   equalize, eq(rx), eq(ry)          eq_evals_locked on the zero-padded points                       (:1681-1697, :1713-1718)
//   dense.deref + Derefs::new         gather_merge_locked: ONE gathered, merged table                  (:275-279, :293-297)
//   derefs.commit                     ONE L x R commit_rows_device over the first R generators         (:301-304, :341-347)
//   PolyEvalNetwork::new              hash_layer_pair_product_locked (2 batch read/write pairs, 2 init/audit pairs: the hashed sets AND their first product
//                                     layer in one pass), product_circuit_many_locked from layer 1 up   (:745-866)
//   ProductLayerProof::prove          k_pp_dotp + k_se_claims: every claim in one wait; product_proof_locked twice (ops, then mem), the first one on
//                                     the dot-product partial sums k_pp_dotp has just left (the pass runs once per proof)   (:1306-1428)
//   HashLayerProof::prove             table_evaluate_many_locked (7 batch at rand_ops, 2 at rand_mem), joint_opening_locked three times   (:922-1046)
// The host does the transcript lines between them, the subset and split checks on the claims, and the proof's byte layout (include/sbn254.h).
// The dense representation and its two tables are only read.  Included by sbn254.hip.
// The KZG build (an SRS instead of gens_derefs) differs in two places:
//   derefs.commit_kzg                 ONE point: with a key, sum_a eq[a] S_a over the cells read at least once (abi_derefs_key.inc); without, the MSM of
//                                     the first min(n', srs->n) entries of the gathered table, n' = 2 b N its non-zero prefix   (:307-312, :349-356, kzg.rs:386-404)
//   DerefsEvalProof::prove (KZG)      joint_reduce, kzg_eval_point, kzg_div_enqueue over n' coefficients and the MSM of the n' - 1 quotient
//                                     coefficients: q_i = 0 for i >= n' - 1, the padding contributes nothing   (:503-550, kzg.rs:174-192)

struct SparseEvalShape {
  size_t batch, N, ell_m, cells, L_ops;                 // L_ops = log2 N = the layers of an ops circuit; ell_m = log2 cells = the layers of a mem circuit
  size_t cnt_d, cnt_o, lc_d, lc_o;                      // evals of the derefs / ops joint openings, padded, and their log2
  size_t ell_d, ell_o, ell_mm;                          // variables of the three opened polynomials
  size_t Ld, Rd, lg_d, lg_o, lg_m;
  size_t pp_mem_polys, pp_mem_claims, pp_ops_polys, pp_ops_claims;   // bytes of the two product proofs' out_polys / out_claims
  size_t rnd_scalars, proof_bytes;
  size_t n_d, n_prefix;                                 // the derefs polynomial's length cnt_d * N and its non-zero prefix 2 b N
  size_t rnd_scalars_kzg, proof_bytes_kzg;              // the KZG build: no derefs draws, comm_derefs one point, proof_derefs [proof | eval]
};
static bool sparse_eval_shape(size_t nx, size_t ny, size_t N, size_t batch, SparseEvalShape* s) {
  if (batch < 1 || batch > (size_t)SE_BATCH_MAX || N < 2 || (N & (N - 1)) || nx > 31 || ny > 31 || std::max(nx, ny) < 1) return false;
  s->batch = batch; s->N = N; s->ell_m = std::max(nx, ny); s->cells = (size_t)1 << s->ell_m; s->L_ops = r1cs_log2(N);
  s->cnt_d = 1; while (s->cnt_d < 2 * batch) s->cnt_d <<= 1;
  s->cnt_o = 1; while (s->cnt_o < 5 * batch) s->cnt_o <<= 1;
  s->lc_d = r1cs_log2(s->cnt_d); s->lc_o = r1cs_log2(s->cnt_o);
  s->ell_d = s->L_ops + s->lc_d; s->ell_o = s->L_ops + s->lc_o; s->ell_mm = s->ell_m + 1;             // sparse_mlpoly_full.rs:619-623
  if (s->ell_o > 2 * (size_t)PE_SIDE_MAX || s->ell_mm > 2 * (size_t)PE_SIDE_MAX || s->L_ops > (size_t)EQ_MAX_VARS || s->ell_m > (size_t)EQ_MAX_VARS) return false;
  s->Ld = (size_t)1 << (s->ell_d / 2); s->lg_d = s->ell_d - s->ell_d / 2; s->Rd = (size_t)1 << s->lg_d;
  s->lg_o = s->ell_o - s->ell_o / 2; s->lg_m = s->ell_mm - s->ell_mm / 2;
  auto polys = [](size_t L) { return 128 * (L * (L - 1) / 2); };
  s->pp_mem_polys = polys(s->ell_m); s->pp_mem_claims = 32 * (2 * 4 * s->ell_m);
  s->pp_ops_polys = polys(s->L_ops); s->pp_ops_claims = 32 * (2 * 4 * batch * s->L_ops + 3 * 2 * batch);
  s->rnd_scalars = 9 + 2 * (s->lg_d + s->lg_o + s->lg_m);
  s->proof_bytes = 32 * s->Ld + 32 * (4 + 6 * batch) + s->pp_mem_polys + s->pp_mem_claims + s->pp_ops_polys + s->pp_ops_claims + 32 * (7 * batch + 2)
                 + 64 * (s->lg_d + s->lg_o + s->lg_m) + 3 * 128;
  s->n_d = s->cnt_d * N; s->n_prefix = 2 * batch * N;
  s->rnd_scalars_kzg = 6 + 2 * (s->lg_o + s->lg_m);
  s->proof_bytes_kzg = 32 + 32 * (4 + 6 * batch) + s->pp_mem_polys + s->pp_mem_claims + s->pp_ops_polys + s->pp_ops_claims + 32 * (7 * batch + 2)
                     + 64 * (s->lg_o + s->lg_m) + 2 * 128 + 64;
  return true;
}

// DensePolynomial::commit of a device table with no blinds (hyrax.rs:283-308), as sbn_commit_table's launches; the caller holds the mutex
static int sparse_eval_commit(sbn_ctx* c, const sbn_bases* gn, const sbn_table* t, size_t L, size_t R, uint8_t* out_xy) {
  const uint32_t* dZ = (const uint32_t*)t->d;
  if (gn->uniq) { RowInfo ri; ri.mont_scalars = true; return commit_rows_device(c, gn, dZ, nullptr, L, R, out_xy, nullptr, ri); }
  int rc;
  if ((rc = ensure(c, c->scal_canon, (L * R + L) * 32))) return rc;
  uint32_t* o = (uint32_t*)c->scal_canon.p;
  LAUNCH(c, "k_scalars_from_mont", k_scalars_from_internal, (unsigned)((L * R + 255) / 256), 256, dZ, o, L * R);
  return commit_rows_device(c, gn, o, nullptr, L, R, out_xy, nullptr);
}

// the proof on the transcript `t` (a copy of the caller's); arguments already checked.  srs != null: the KZG build (gens_derefs is null, key may be)
static int sparse_eval_locked(sbn_ctx* c, const sbn_dense* dn, const uint8_t* rx, size_t nx, const uint8_t* ry, size_t ny, const uint8_t* evals,
                              const sbn_bases* gens_ops, const sbn_bases* gens_mem, const sbn_bases* gens_derefs, const sbn_bases* srs, const sbn_derefs_key* key,
                              const SparseEvalShape& s, const uint8_t* rnd, sbn_host::MerlinTranscript& t, uint8_t* out_proof) {
  using namespace sbn_host::fr;
  // every intermediate of the call: the two eq tables, the derefs table, the 4 batch + 4 hashed sets and their layers, and the views (slices of
  // derefs, comb_ops, comb_mem), which own nothing
  TableScope T(c);
  sbn_host::Script ts{t};
  int rc;
  const size_t b = s.batch, N = s.N;
  // rnd: the three openings' draws in the reference's order (HashLayerProof::prove: derefs, ops, mem)
  const bool kzg = srs != nullptr;
  const uint8_t* rnd_d = rnd;                                      // (the KZG build's derefs opening draws nothing: ops | mem)
  const uint8_t* rnd_o = kzg ? rnd : rnd_d + 32 * (3 + 2 * s.lg_d);
  const uint8_t* rnd_m = rnd_o + 32 * (3 + 2 * s.lg_o);
  // out_proof: the fields of SparseMatPolyEvalProof in declaration order, nested structs likewise (:1659-1662, :1529-1532, :1293-1299, :874-882)
  uint8_t* o_comm = out_proof;
  uint8_t* o_pl_row = o_comm + 32 * (kzg ? 1 : s.Ld);             // init, read[b], write[b], audit
  uint8_t* o_pl_col = o_pl_row + 32 * (2 + 2 * b);
  uint8_t* o_pl_val = o_pl_col + 32 * (2 + 2 * b);                // eval_dotp_left[b], eval_dotp_right[b]
  uint8_t* o_pp_mem = o_pl_val + 32 * (2 * b);                    // proof_mem is declared before proof_ops
  uint8_t* o_pp_ops = o_pp_mem + s.pp_mem_polys + s.pp_mem_claims;
  uint8_t* o_hl_row = o_pp_ops + s.pp_ops_polys + s.pp_ops_claims;   // addr[b], read_ts[b], audit_ts
  uint8_t* o_hl_col = o_hl_row + 32 * (2 * b + 1);
  uint8_t* o_hl_val = o_hl_col + 32 * (2 * b + 1);
  uint8_t* o_hl_der = o_hl_val + 32 * b;                          // row[b], col[b]
  uint8_t* o_open_o = o_hl_der + 32 * (2 * b);
  uint8_t* o_open_m = o_open_o + 64 * s.lg_o + 128;
  uint8_t* o_open_d = o_open_m + 64 * s.lg_m + 128;

  ts.protocol("Sparse polynomial evaluation proof");               // :1709

  // ---- 1. equalize, the two eq tables, derefs (:1713-1720) ----
  sbn_table *mem_rx = nullptr, *mem_ry = nullptr, *derefs = nullptr;
  {
    std::vector<uint8_t> ext(32 * s.ell_m, 0);                     // the shorter point is padded with zeros at the front (:1681-1697)
    memcpy(&ext[32 * (s.ell_m - nx)], rx, 32 * nx);
    if ((rc = eq_evals_locked(c, ext.data(), s.ell_m, &mem_rx))) return rc;
    T.keep(mem_rx);
    std::fill(ext.begin(), ext.end(), 0);
    memcpy(&ext[32 * (s.ell_m - ny)], ry, 32 * ny);
    if ((rc = eq_evals_locked(c, ext.data(), s.ell_m, &mem_ry))) return rc;
    T.keep(mem_ry);
    const sbn_table* mem[2 * SE_BATCH_MAX]; const void* addr[2 * SE_BATCH_MAX];
    for (size_t k = 0; k < b; k++) { mem[k] = mem_rx; addr[k] = dense_addr(dn, 0) + k * N; mem[b + k] = mem_ry; addr[b + k] = dense_addr(dn, 1) + k * N; }
    if ((rc = gather_merge_locked(c, mem, addr, 2 * b, N, -1, 0, 1, 0, &derefs))) return rc;
    T.keep(derefs);
  }

  // ---- 2. the derefs commitment (:1723-1727, :341-347; PolyCommitment's lines hyrax.rs:44-51) ----
  ts.message("derefs_commitment", "begin_derefs_commitment", 23);
  if (kzg) {                                                       // :1781-1785, :349-356, kzg.rs:386-404
    uint8_t xy[64]; int inf = 0;
    const size_t m = std::min(s.n_prefix, srs->n);                 // KZGPolyCommitment::commit truncates to the SRS (kzg.rs:388); the padding behind n' is zero
    if (key) rc = derefs_key_commit_locked(c, key, mem_rx, mem_ry, xy, &inf);
    else rc = kzg_msm_internal(c, srs, (const uint32_t*)derefs->d, m, xy, &inf);
    if (rc) return rc;
    if (inf) memset(xy, 0, 64);
    sbn_g1_compress(xy, 1, o_comm);                                // the identity as serialize_compressed writes it
    ts.point("comm_poly_row_col_ops_val", o_comm);
  } else {
    const sbn_bases *gn = nullptr, *g1 = nullptr;
    if ((rc = r1cs_proof_gens(c, gens_derefs, s.Rd, &gn, &g1))) return rc;
    std::vector<uint8_t> xy(64 * s.Ld);
    if ((rc = sparse_eval_commit(c, gn, derefs, s.Ld, s.Rd, xy.data()))) return rc;
    sbn_g1_compress(xy.data(), s.Ld, o_comm);
    ts.message("comm_poly_row_col_ops_val", "poly_commitment_begin", 21);
    for (size_t i = 0; i < s.Ld; i++) ts.point("poly_commitment_share", o_comm + 32 * i);
    ts.message("comm_poly_row_col_ops_val", "poly_commitment_end", 19);
  }
  ts.message("derefs_commitment", "end_derefs_commitment", 21);
  uint8_t r_hm[64]; const uint8_t* r_hash = r_hm; const uint8_t* r_multiset = r_hm + 32;
  ts.challenges("challenge_r_hash", r_hm, 2);                                                                    // :1730

  // ---- 3. PolyEvalNetwork::new (:853-866): the hashed sets and their product circuits ----
  // ops circuits in proof_ops' order: row read, row write, col read, col write (:1380-1392); mem circuits: row init, row audit, col init, col audit (:1404-1409)
  const size_t n_ops = 4 * b, L_ops = s.L_ops, L_mem = s.ell_m;
  std::vector<const sbn_table*> row_val(b), col_val(b), wgt(b);
  std::vector<const sbn_table*> hs_ops(n_ops), hs_mem(4);
  for (size_t k = 0; k < b; k++) {
    row_val[k] = T.view(derefs, k * N, N); col_val[k] = T.view(derefs, (b + k) * N, N);
    wgt[k] = T.view(&dn->ops, (4 * b + k) * N, N);
  }
  // the first product layer comes out of the hashing pass (k_hash_pair_prod); the layers above it from product_circuit_many_locked, started one layer up
  std::vector<sbn_table*> pc_ops(n_ops * L_ops + 1, nullptr), pc_mem(4 * L_mem + 1, nullptr);
  for (int side = 0; side < 2; side++) {
    const sbn_table* mem = side ? mem_ry : mem_rx;
    sbn_table *ta = nullptr, *tb = nullptr, *pa = nullptr, *pb = nullptr;
    if ((rc = hash_layer_pair_product_locked(c, nullptr, mem, nullptr, 0, dense_audit(dn, side), 0, r_hash, r_multiset, &ta, &tb, &pa, &pb))) return rc;
    hs_mem[2 * side] = T.keep(ta); hs_mem[2 * side + 1] = T.keep(tb);
    pc_mem[(2 * side) * L_mem] = T.keep(pa); pc_mem[(2 * side + 1) * L_mem] = T.keep(pb);
    for (size_t k = 0; k < b; k++) {
      const uint32_t* rts = dense_read_ts(dn, side) + k * N;
      if ((rc = hash_layer_pair_product_locked(c, dense_addr(dn, side) + k * N, side ? col_val[k] : row_val[k], rts, 0, rts, 1, r_hash, r_multiset, &ta, &tb, &pa, &pb))) return rc;
      const size_t ir = 2 * b * side + k, iw = ir + b;
      hs_ops[ir] = T.keep(ta); hs_ops[iw] = T.keep(tb);
      pc_ops[ir * L_ops] = T.keep(pa); pc_ops[iw * L_ops] = T.keep(pb);
    }
  }
  if (L_ops > 1) {
    std::vector<const sbn_table*> l0(n_ops);
    for (size_t i = 0; i < n_ops; i++) l0[i] = pc_ops[i * L_ops];
    if ((rc = product_circuit_many_locked(c, l0.data(), n_ops, pc_ops.data() + 1, L_ops, N / 2, L_ops - 1))) return rc;
    for (size_t i = 0; i < n_ops; i++) for (size_t j = 1; j < L_ops; j++) T.keep(pc_ops[i * L_ops + j]);
  }
  if (L_mem > 1) {
    std::vector<const sbn_table*> l0(4);
    for (size_t i = 0; i < 4; i++) l0[i] = pc_mem[i * L_mem];
    if ((rc = product_circuit_many_locked(c, l0.data(), 4, pc_mem.data() + 1, L_mem, s.cells / 2, L_mem - 1))) return rc;
    for (size_t i = 0; i < 4; i++) for (size_t j = 1; j < L_mem; j++) T.keep(pc_mem[i * L_mem + j]);
  }

  // ---- 4. PolyEvalNetworkProof::prove opens with the same protocol name again (:1555); ProductLayerProof::prove: every claim in one wait (:1314-1373) ----
  ts.protocol("Sparse polynomial evaluation proof");
  ts.protocol("Sparse polynomial product layer proof");
  // the split dot-product circuits, interleaved left_i, right_i (:1354-1373; DotProductCircuit::split, product_tree.rs:87-105)
  const size_t n_dotp = 2 * b, half = N / 2;
  std::vector<const sbn_table*> dl(n_dotp), dr(n_dotp), dw(n_dotp);
  for (size_t k = 0; k < b; k++)
    for (size_t h = 0; h < 2; h++) { dl[2 * k + h] = T.view(row_val[k], h * half, half); dr[2 * k + h] = T.view(col_val[k], h * half, half); dw[2 * k + h] = T.view(wgt[k], h * half, half); }
  El claim[SE_TOPS_MAX + SE_DOTP_MAX];
  {
    if ((rc = sc_tickets(c))) return rc;                            // (for the host mailbox it allocates on first use: k_se_claims writes there; no ticket is taken)
    const size_t gx_dot = pp_dotp_grid(half);                       // the grid product_proof_run uses: proof_ops takes these partial sums as they lie
    if ((rc = ensure(c, c->sc_partial, std::max(SC_PARTIAL_BYTES, (size_t)SC_PACK_MAX * gx_dot * 32)))) return rc;
    ScArgsPack pack; memset(&pack, 0, sizeof pack);
    for (size_t k = 0; k < n_dotp; k++) { pack.a[k].t[0] = (const uint32_t*)dl[k]->d; pack.a[k].t[1] = (const uint32_t*)dr[k]->d; pack.a[k].t[2] = (const uint32_t*)dw[k]->d; }
    LAUNCH(c, "k_pp_dotp", k_pp_dotp, dim3((unsigned)gx_dot, (unsigned)n_dotp), 256, pack, half, (uint32_t*)c->sc_partial.p);
    SeTops tops; memset(&tops, 0, sizeof tops);
    // slot order: row init, row read[b], row write[b], row audit, then the column side: the order of the appends
    for (int side = 0; side < 2; side++) {
      const size_t o = (size_t)side * (2 * b + 2);
      tops.p[o] = (const uint32_t*)pc_mem[(2 * side) * L_mem + L_mem - 1]->d;
      tops.p[o + 2 * b + 1] = (const uint32_t*)pc_mem[(2 * side + 1) * L_mem + L_mem - 1]->d;
      for (size_t k = 0; k < b; k++) {
        tops.p[o + 1 + k] = (const uint32_t*)pc_ops[(2 * b * side + k) * L_ops + L_ops - 1]->d;
        tops.p[o + 1 + b + k] = (const uint32_t*)pc_ops[(2 * b * side + b + k) * L_ops + L_ops - 1]->d;
      }
    }
    const uint32_t n_tops = (uint32_t)(4 * b + 4), seq = ++c->mbox_seq;
    LAUNCH(c, "k_se_claims", k_se_claims, 1, 256, tops, n_tops, (const uint32_t*)c->sc_partial.p, (uint32_t)gx_dot, (uint32_t)n_dotp, zk_slot(c, 0), zk_flag(c, 0), seq);
    LAUNCHCHK(c);
    if ((rc = sc_flag_wait(c, zk_flag(c, 0), seq))) return rc;
    memcpy(claim, zk_slot(c, 0), 32 * (n_tops + n_dotp));
  }
  for (int side = 0; side < 2; side++) {
    const El* cl = claim + (size_t)side * (2 * b + 2);
    El ws = from_u64(1), rs = from_u64(1);
    for (size_t k = 0; k < b; k++) { rs = fmul(rs, cl[1 + k]); ws = fmul(ws, cl[1 + b + k]); }
    if (memcmp(fmul(cl[0], ws).v, fmul(rs, cl[2 * b + 1]).v, 32))   // :1324, :1339 — cannot fail on a handle sbn_dense_build made
      return fail(c, SBN_EHIP, "sparse eval: the %s memory's subset check init * writes == reads * audit failed  [sparse_mlpoly_full.rs:%d assert_eq]", side ? "column" : "row", side ? 1339 : 1324);
    uint8_t* o = side ? o_pl_col : o_pl_row;
    memcpy(o, cl, 32 * (2 * b + 2));
    ts.scalar(side ? "claim_col_eval_init" : "claim_row_eval_init", o);
    ts.scalars(side ? "claim_col_eval_read" : "claim_row_eval_read", o + 32, b);
    ts.scalars(side ? "claim_col_eval_write" : "claim_row_eval_write", o + 32 * (1 + b), b);
    ts.scalar(side ? "claim_col_eval_audit" : "claim_row_eval_audit", o + 32 * (2 * b + 1));
  }
  for (size_t k = 0; k < b; k++) {
    const El& l = claim[4 * b + 4 + 2 * k]; const El& r = claim[4 * b + 4 + 2 * k + 1];
    memcpy(o_pl_val + 32 * k, l.v, 32); memcpy(o_pl_val + 32 * (b + k), r.v, 32);
    ts.scalar("claim_eval_dotp_left", o_pl_val + 32 * k);
    ts.scalar("claim_eval_dotp_right", o_pl_val + 32 * (b + k));
    if (memcmp(add(l, r).v, evals + 32 * k, 32))
      return fail(c, SBN_EINVAL, "sparse eval: eval_dotp_left + eval_dotp_right != evals[%zu]  [sparse_mlpoly_full.rs:1366 assert_eq]", k);
  }

  // ---- 5. proof_ops, then proof_mem (:1397-1415) ----
  std::vector<uint8_t> rand_ops(32 * L_ops), rand_mem(32 * L_mem);
  {
    sbn_transcript w; w.t = t;
    std::vector<const sbn_table*> lay(n_ops * L_ops);
    for (size_t i = 0; i < n_ops; i++) { lay[i * L_ops] = hs_ops[i]; for (size_t j = 1; j < L_ops; j++) lay[i * L_ops + j] = pc_ops[i * L_ops + j - 1]; }
    uint8_t fin[32 * SC_PACK_MAX];
    if ((rc = product_proof_locked(c, lay.data(), n_ops, L_ops, dl.data(), dr.data(), dw.data(), n_dotp, &w, o_pp_ops, o_pp_ops + s.pp_ops_polys, rand_ops.data(), fin,
                                   true /* k_pp_dotp ran for the claims above; nothing has written c->sc_partial since */))) return rc;
    lay.assign(4 * L_mem, nullptr);
    for (size_t i = 0; i < 4; i++) { lay[i * L_mem] = hs_mem[i]; for (size_t j = 1; j < L_mem; j++) lay[i * L_mem + j] = pc_mem[i * L_mem + j - 1]; }
    if ((rc = product_proof_locked(c, lay.data(), 4, L_mem, nullptr, nullptr, nullptr, 0, &w, o_pp_mem, o_pp_mem + s.pp_mem_polys, rand_mem.data(), fin))) return rc;
    t = w.t;
  }

  // ---- 6. HashLayerProof::prove (:922-1046) ----
  ts.protocol("Sparse polynomial hash layer proof");
  {
    // 2 batch derefs polynomials and the 5 batch of comb_ops (row addr, row read_ts, col addr, col read_ts, val: its own order) at rand_ops, ONE eq table
    std::vector<const sbn_table*> Z(7 * b);
    for (size_t k = 0; k < b; k++) { Z[k] = row_val[k]; Z[b + k] = col_val[k]; }
    for (size_t j = 0; j < 5 * b; j++) Z[2 * b + j] = T.view(&dn->ops, j * N, N);
    std::vector<uint8_t> ev(32 * 7 * b);
    if ((rc = table_evaluate_many_locked(c, Z.data(), 7 * b, rand_ops.data(), L_ops, ev.data()))) return rc;
    const sbn_table* Zm[2] = {T.view(&dn->mem, 0, s.cells), T.view(&dn->mem, s.cells, s.cells)};
    uint8_t evm[64];
    if ((rc = table_evaluate_many_locked(c, Zm, 2, rand_mem.data(), L_mem, evm))) return rc;
    const uint8_t* e_ops = &ev[32 * 2 * b];
    memcpy(o_hl_der, ev.data(), 32 * 2 * b);
    memcpy(o_hl_row, e_ops, 32 * 2 * b); memcpy(o_hl_row + 32 * 2 * b, evm, 32);
    memcpy(o_hl_col, e_ops + 32 * 2 * b, 32 * 2 * b); memcpy(o_hl_col + 32 * 2 * b, evm + 32, 32);
    memcpy(o_hl_val, e_ops + 32 * 4 * b, 32 * b);
    uint8_t cx[64], cy[64], jc[32]; int xi = 0, yi = 0;
    std::vector<uint8_t> pad(32 * std::max(s.cnt_d, s.cnt_o), 0);
    memcpy(pad.data(), ev.data(), 32 * 2 * b);
    if (kzg) {
      // DerefsEvalProof::prove, KZG (:503-550): the reduction's claim is absorbed, then KZGProof::prove on the derefs table at kzg_eval_point
      ts.protocol("Derefs evaluation proof (KZG)");
      std::vector<uint8_t> rj;
      joint_reduce(pad.data(), s.cnt_d, s.lc_d, "evals_ops_val", "challenge_combine_n_to_one", "joint_claim_eval", rand_ops.data(), L_ops, t, rj, jc);
      uint8_t z[32], pxy[64]; int pinf = 0;
      ts.challenge("kzg_eval_point", z);
      const size_t n = s.n_prefix;                                 // >= 4
      if ((rc = ensure(c, c->kzg_ws, 64 + kzg_levels_bytes(n)))) return rc;
      uint32_t* evd = (uint32_t*)c->kzg_ws.p;
      ScScalar p2[64]; kzg_pow2_table(z, p2);
      void* qd = nullptr; size_t qbytes = 0;
      if ((rc = kzg_qbuf(c, n - 1, &qd, &qbytes))) return rc;
      rc = kzg_div_enqueue(c, (const uint32_t*)derefs->d, n, p2, (uint32_t*)qd, n - 1, evd, evd + 16);
      if (rc == SBN_OK) rc = kzg_fetch(c, evd, 1, o_open_d + 32);
      if (rc == SBN_OK) rc = kzg_msm_internal(c, srs, (const uint32_t*)qd, n - 1, pxy, &pinf);
      hipStreamSynchronize(c->stream); pool_put(c, qd, qbytes);
      if (rc) return rc;
      if (pinf) memset(pxy, 0, 64);
      sbn_g1_compress(pxy, 1, o_open_d);
    } else {
    // DerefsEvalProof::prove (:412-432)
    ts.protocol("Derefs evaluation proof");
    if ((rc = joint_opening_locked(c, gens_derefs, derefs, pad.data(), s.cnt_d, s.lc_d, "evals_ops_val", "challenge_combine_n_to_one", "joint_claim_eval",
                                   rand_ops.data(), L_ops, rnd_d, t, nullptr, jc, o_open_d, cx, &xi, cy, &yi))) return rc;
    }
    // comb_ops (:978-1009)
    std::fill(pad.begin(), pad.end(), 0);
    memcpy(pad.data(), e_ops, 32 * 5 * b);
    if ((rc = joint_opening_locked(c, gens_ops, &dn->ops, pad.data(), s.cnt_o, s.lc_o, "claim_evals_ops", "challenge_combine_n_to_one", "joint_claim_eval_ops",
                                   rand_ops.data(), L_ops, rnd_o, t, nullptr, jc, o_open_o, cx, &xi, cy, &yi))) return rc;
    // comb_mem (:1011-1035)
    if ((rc = joint_opening_locked(c, gens_mem, &dn->mem, evm, 2, 1, "claim_evals_mem", "challenge_combine_two_to_one", "joint_claim_eval_mem",
                                   rand_mem.data(), L_mem, rnd_m, t, nullptr, jc, o_open_m, cx, &xi, cy, &yi))) return rc;
  }
  if (c->prof) { HIPCHK(c, hipStreamSynchronize(c->stream)); prof_drain(c); }
  return T.done();
}

// the shape, generator and canonicity checks of both builds, under the build's name `pfx`.  srs != null: the KZG build (gens_derefs is null, key may be)
static int sparse_eval_check(sbn_ctx* c, const char* pfx, const sbn_dense* dn, const uint8_t* rx, size_t nx, const uint8_t* ry, size_t ny, const uint8_t* evals,
                             const sbn_bases* gens_ops, const sbn_bases* gens_mem, const sbn_bases* gens_derefs, const sbn_bases* srs, const sbn_derefs_key* key,
                             const uint8_t* rnd, SparseEvalShape* sp) {
  SparseEvalShape& s = *sp;
  if (dn->batch > (size_t)SE_BATCH_MAX) return fail(c, SBN_EINVAL, "%s: batch = %zu: proof_ops would hold %zu instances, at most %d fit one product proof", pfx, dn->batch, 6 * dn->batch, SC_PACK_MAX);
  if (dn->N < 2) return fail(c, SBN_EINVAL, "%s: N = %zu: the dot-product circuits cannot be split  [product_tree.rs:89 assert_eq]", pfx, dn->N);
  if (nx > 31 || ny > 31 || ((size_t)1 << std::max(nx, ny)) != dn->cells)
    return fail(c, SBN_EINVAL, "%s: rx has %zu and ry %zu variables, the memories have %zu cells  [sparse_mlpoly_full.rs:226 assert, hyrax.rs:218 assert_eq]", pfx, nx, ny, dn->cells);
  if (!sparse_eval_shape(nx, ny, dn->N, dn->batch, &s)) return fail(c, SBN_EINVAL, "%s: shape (%zu, %zu, N = %zu, batch = %zu) is outside what the openings take", pfx, nx, ny, dn->N, dn->batch);
  const struct { const sbn_bases* g; size_t lg; const char* name; } gs[3] = {{gens_ops, s.lg_o, "gens_ops"}, {gens_mem, s.lg_m, "gens_mem"}, {gens_derefs, s.lg_d, "gens_derefs"}};
  for (const auto& x : gs)
    if (x.g && (x.g->n != ((size_t)1 << x.lg) + 1 || !x.g->has_h))
      return fail(c, SBN_EINVAL, "%s: %s has %zu points%s, the opening needs %zu + 1 with h  [nizk/mod.rs:412-415, :455]", pfx, x.name, x.g->n, x.g->has_h ? "" : " and no h", (size_t)1 << x.lg);
  if (srs) {
    if (srs->has_h) return fail(c, SBN_EINVAL, "%s: the SRS handle has an h; an SRS is sbn_kzg_srs_upload's or sbn_kzg_srs_from_tau's", pfx);
    if (srs->n < s.n_d - 1)
      return fail(c, SBN_EINVAL, "%s: the derefs quotient has %zu coefficients, the SRS %zu points  [kzg.rs:186 slices past its end]", pfx, s.n_d - 1, srs->n);
    if (key && (key->dense != dn || key->srs != srs || key->srs_n != srs->n || key->batch != dn->batch || key->N != dn->N || key->cells != dn->cells))
      return fail(c, SBN_EINVAL, "%s: the derefs key was built for another dense handle or another SRS", pfx);
  }
  const struct { const uint8_t* p; size_t n; const char* name; } sc[4] = {{rx, nx, "rx"}, {ry, ny, "ry"}, {evals, s.batch, "evals"}, {rnd, srs ? s.rnd_scalars_kzg : s.rnd_scalars, "rnd"}};
  for (const auto& x : sc)
    for (size_t i = 0; i < x.n; i++) if (!fr_canonical(x.p + 32 * i)) return fail(c, SBN_EINVAL, "%s: %s[%zu] is not canonical  [scalar.rs:87-95]", pfx, x.name, i);
  return SBN_OK;
}

// both builds' entry: the checks under the build's name `pfx`, then the proof on a copy of the transcript, into a buffer of the call's own
static int sparse_eval_entry(sbn_ctx* c, const char* pfx, const sbn_dense* dn, const uint8_t* rx, size_t nx, const uint8_t* ry, size_t ny, const uint8_t* evals,
                             const sbn_bases* gens_ops, const sbn_bases* gens_mem, const sbn_bases* gens_derefs, const sbn_bases* srs, const sbn_derefs_key* key,
                             const uint8_t* rnd, sbn_transcript* tr, uint8_t* out_proof) {
  std::lock_guard<std::mutex> g(c->mu); hipSetDevice(c->device);
  SparseEvalShape s;
  int rc;
  if ((rc = sparse_eval_check(c, pfx, dn, rx, nx, ry, ny, evals, gens_ops, gens_mem, gens_derefs, srs, key, rnd, &s))) return rc;
  std::vector<uint8_t> proof(srs ? s.proof_bytes_kzg : s.proof_bytes);      // the caller's buffer is written only by a call that succeeded
  if ((rc = prove_on_copy(c, tr, [&](sbn_host::MerlinTranscript& t) { return sparse_eval_locked(c, dn, rx, nx, ry, ny, evals, gens_ops, gens_mem, gens_derefs, srs, key, s, rnd, t, proof.data()); }))) return rc;
  memcpy(out_proof, proof.data(), proof.size());
  return SBN_OK;
}

extern "C" {

int sbn_sparse_eval_sizes(size_t num_vars_x, size_t num_vars_y, size_t num_ops, size_t batch, size_t* rnd_scalars, size_t* proof_bytes) {
  SparseEvalShape s;
  if (!sparse_eval_shape(num_vars_x, num_vars_y, num_ops, batch, &s)) return SBN_EINVAL;
  if (rnd_scalars) *rnd_scalars = s.rnd_scalars;
  if (proof_bytes) *proof_bytes = s.proof_bytes;
  return SBN_OK;
}

int sbn_sparse_eval_prove(sbn_ctx* c, const sbn_dense* dn, const uint8_t* rx, size_t nx, const uint8_t* ry, size_t ny, const uint8_t* evals,
                          const sbn_bases* gens_ops, const sbn_bases* gens_mem, const sbn_bases* gens_derefs, const uint8_t* rnd, sbn_transcript* tr, uint8_t* out_proof) {
  if (!c || !dn || (!rx && nx) || (!ry && ny) || !evals || !gens_ops || !gens_mem || !gens_derefs || !rnd || !tr || !out_proof) return SBN_EINVAL;
  return sparse_eval_entry(c, "sparse eval", dn, rx, nx, ry, ny, evals, gens_ops, gens_mem, gens_derefs, nullptr, nullptr, rnd, tr, out_proof);
}

int sbn_sparse_eval_kzg_sizes(size_t num_vars_x, size_t num_vars_y, size_t num_ops, size_t batch, size_t* rnd_scalars, size_t* proof_bytes) {
  SparseEvalShape s;
  if (!sparse_eval_shape(num_vars_x, num_vars_y, num_ops, batch, &s)) return SBN_EINVAL;
  if (rnd_scalars) *rnd_scalars = s.rnd_scalars_kzg;
  if (proof_bytes) *proof_bytes = s.proof_bytes_kzg;
  return SBN_OK;
}

int sbn_sparse_eval_prove_kzg(sbn_ctx* c, const sbn_dense* dn, const uint8_t* rx, size_t nx, const uint8_t* ry, size_t ny, const uint8_t* evals,
                              const sbn_bases* gens_ops, const sbn_bases* gens_mem, const sbn_bases* srs, const sbn_derefs_key* key,
                              const uint8_t* rnd, sbn_transcript* tr, uint8_t* out_proof) {
  if (!c || !dn || (!rx && nx) || (!ry && ny) || !evals || !gens_ops || !gens_mem || !srs || !rnd || !tr || !out_proof) return SBN_EINVAL;
  return sparse_eval_entry(c, "sparse eval (KZG)", dn, rx, nx, ry, ny, evals, gens_ops, gens_mem, nullptr, srs, key, rnd, tr, out_proof);
}

}  // extern "C"
