// abi_sparse_verify.inc — C ABI: SparseMatPolyEvalProof::verify (sparse_mlpoly_full.rs:1815-1845; wrapped by R1CSEvalProof::verify, r1cs.rs:465-490) in
// ONE call, the Hyrax build: PolyEvalNetworkProof::verify (:1581-1650) with ProductLayerProof::verify, both ProductCircuitEvalProofBatched::verify and
// HashLayerProof::verify inside, the three joint openings and the Merlin transcript included.
//
// The field and transcript half is sparse_verify_host.hpp, host only.  The group half is three openings (derefs, ops, mem: the reference's order), each
// the two stages of polyeval_verify_locked (abi_polyeval_verify.inc; opening_eq_launch and opening_row_commit of abi_verify_common.inc), rearranged so that the call waits for the device four times instead of six:
//   before any hashing   ONE k_g1_decompress over every point of the proof: comm_derefs (written in table layout, where the first MSM reads it: no handle
//                        is built) and the 2 lg + 2 points of each opening.  It runs under the host's product-layer work.
//   per opening          joint_reduce on the host; k_polyeval_eq, C_LZ by msm_single_launch over the commitment's device points, C_Zr = Zr * G as a
//                        one-term k_window_sums launch over the derived set (polyeval_ext) in place of a one-row commit; ONE hand-over and ONE wait (the
//                        first brings the decompression flags); then the transcript lines of the opening (polyeval_verify_script).
//   final equations      they feed no transcript, so none has a wait of its own: opening k's row commit of -z1 s ‖ -z1 a r ‖ -z2 is enqueued behind the
//                        hand-over of opening k + 1 and runs while the host hashes; behind the mem opening's transcript ONE k_window_sums launch takes
//                        the three sums over 2 lg + 4 points each (the proof's points, Cx, Cy), ONE hand-over brings them and the three commit sums,
//                        and the host folds and tests each equation for the identity on its own: the group equations of the reference, no batching.
// The KZG build (sbn_sparse_eval_verify_kzg) runs the same function with `kz` set: comm_derefs is one compressed point absorbed as :349-356 does, derefs_reduce
// (:561-584) replaces the derefs opening (the joint claim is absorbed, not compared, and kzg_eval_point is drawn), the two Hyrax openings of comb_ops and
// comb_mem and their final equations are what they are above, and the pairing check of (comm_derefs, kzg_eval_point, eval, pi) follows behind the mutex'
// release through sbn_g1_decompress and the KZG check of abi_pairing.inc.
// Included by sbn254.hip; needs abi_verify_common.inc (the envelope, both hand-overs, the opening stages), abi_polyeval.inc (polyeval_ext), abi_sparse_eval.inc
// (sparse_eval_shape) and, for the KZG build, abi_pairing.inc (kzg_check_run).

static const int SV_OPENINGS = 3;                    // derefs, ops, mem
struct SvKzg { uint8_t comm[32], pi[32], y[32], z[32]; };      // out: the KZG opening to check: the two points normalised compressed, eval, kzg_eval_point
static const size_t SV_STAGE_POINTS = 64 + SS_WINDOWS;      // the window sums of C_LZ (at most 64: checked) and of C_Zr

struct SvOpening {
  const sbn_bases* gens; const sbn_bases* ext; const sbn_bases* comm;      // comm null: comm_derefs, decompressed by this call
  const uint32_t* comm_pts;
  OpeningShape sh; size_t pt0;                        // pt0: its first point among the call's decompressed points
  const uint8_t* proof;                               // its bytes: L[lg], R[lg], delta, beta, z1, z2
  std::vector<uint8_t> rj, hs;                        // the opening's point; the scalars of the final equation's np + 2 points
  uint8_t claim[32], Cxy[128];
  std::vector<sbn_host::fr::El> u, ui;
  PolyevalFinal fin;
};

// the check on the transcript `t` (a copy of the caller's); arguments already checked.  SBN_OK with *accepted = 0: the proof is refused
static int sparse_verify_locked(sbn_ctx* c, const SparseEvalShape& s, const sbn_host::spv::Layout& L, const sbn_bases* comm_ops, const sbn_bases* comm_mem,
                                const uint8_t* rx, size_t nx, const uint8_t* ry, size_t ny, const uint8_t* evals,
                                const sbn_bases* gens_ops, const sbn_bases* gens_mem, const sbn_bases* gens_derefs, const uint8_t* proof,
                                sbn_host::MerlinTranscript& t, int* accepted, SvKzg* kz = nullptr) {
  using namespace sbn_host::fr;
  namespace spv = sbn_host::spv;
  *accepted = 0;
  if (!spv::proof_scalars_canonical(L, proof)) return SBN_OK;      // Scalar::from_bytes fails (scalar.rs:87-95): nothing has been launched
  int rc;
  SvOpening op[SV_OPENINGS];
  const int k0 = kz ? 1 : 0;                                           // the KZG build has no derefs opening
  {
    const sbn_bases* gs[SV_OPENINGS] = {gens_derefs, gens_ops, gens_mem};
    const sbn_bases* cm[SV_OPENINGS] = {nullptr, comm_ops, comm_mem};
    const size_t ells[SV_OPENINGS] = {s.ell_d, s.ell_o, s.ell_mm};
    const spv::Field fl[SV_OPENINGS] = {spv::HASH_PROOF_DEREFS, spv::HASH_PROOF_OPS, spv::HASH_PROOF_MEM};
    size_t pt = kz ? 0 : s.Ld;
    for (int k = 0; k < SV_OPENINGS; k++) {
      SvOpening& o = op[k];
      if (k < k0) { o.gens = o.ext = o.comm = nullptr; o.comm_pts = nullptr; o.sh = OpeningShape(); o.pt0 = 0; o.proof = nullptr; continue; }      // (all sizes zero)
      o.gens = gs[k]; o.comm = cm[k]; o.sh = opening_shape(ells[k]); o.pt0 = pt; pt += o.sh.np; o.proof = proof + L.off[fl[k]];
      o.comm_pts = cm[k] ? (const uint32_t*)cm[k]->d_pts : nullptr;
      if ((rc = polyeval_ext(c, o.gens, &o.ext))) return rc;
    }
  }
  const size_t NP = op[2].pt0 + op[2].sh.np;                            // comm_derefs, then the points of the derefs, ops and mem openings
  size_t nmax = 0, Lmax = 0;
  for (const SvOpening& o : op) { nmax = std::max(nmax, o.sh.n); Lmax = std::max(Lmax, o.sh.L_size); }
  const size_t okp = (NP + 127) / 128;                               // the decompression flags as whole 128-byte entries of the first hand-over
  const size_t desc_bytes = 4 * (size_t)SS_DESC_WORDS;
  auto up = [](size_t x) { return (x + 255) / 256 * 256; };

  // pinned staging: every block is written once and read by one copy, so nothing is overwritten under a copy in flight
  const size_t h_comp = 0, h_d1 = up(32 * NP), h_df = h_d1 + SV_OPENINGS * desc_bytes, h_cxy = h_df + SV_OPENINGS * desc_bytes, h_total = h_cxy + SV_OPENINGS * 128;
  if ((rc = ensure_pin(c, std::max<size_t>(8192, h_total)))) return rc;
  if ((rc = ensure(c, c->wsum, 4096))) return rc;
  uint8_t* pin = (uint8_t*)c->pin;

  // device state: the proof's points (compressed, table layout with room for Cx, Cy of each opening, flags), eq(r) of one opening at a time, the row,
  // the descriptors, the staged sums of a first stage, the sums of the final equations
  const size_t o_comp = 0, o_mont = up(32 * NP), o_ok = up(o_mont + 64 * (NP + 2 * SV_OPENINGS)), o_L = up(o_ok + 128 * okp), o_Lc = o_L + up(32 * Lmax), o_R = o_Lc + up(32 * Lmax),
               o_s = o_R + up(32 * nmax), o_row = o_s + up(32 * nmax), o_d1 = o_row + up(32 * (nmax + 2)), o_df = o_d1 + up(SV_OPENINGS * desc_bytes),
               o_stage = o_df + up(SV_OPENINGS * desc_bytes), o_fin = o_stage + up(128 * (SV_STAGE_POINTS + okp)), total = o_fin + up(128 * (SV_OPENINGS * SS_WINDOWS + SV_OPENINGS));
  SlabLease slab(c);                                                 // behind a refusal nothing stays queued
  if ((rc = slab.get(total, "sparse verify state"))) return rc;
  uint8_t* p0 = (uint8_t*)slab.p;
  uint32_t* d_mont = (uint32_t*)(p0 + o_mont); uint8_t* d_ok = p0 + o_ok; uint32_t* d_L = (uint32_t*)(p0 + o_L); uint32_t* d_Lc = (uint32_t*)(p0 + o_Lc);
  uint32_t* d_row = (uint32_t*)(p0 + o_row); uint32_t* d_stage = (uint32_t*)(p0 + o_stage); uint32_t* d_fin = (uint32_t*)(p0 + o_fin);
  op[0].comm_pts = d_mont;
  // opening k's row of the final equation and its commit, launches only; the sum lands in d_fin[3 * 64 + k]
  auto row_commit = [&](int k) { return opening_row_commit(c, op[k].sh, op[k].ext, op[k].u, op[k].ui, op[k].fin, d_row, d_fin + 32 * (size_t)(SV_OPENINGS * SS_WINDOWS + k)); };

  // ---- before any hashing: every point of the proof, one launch ----
  uint8_t* comp = pin + h_comp;                                       // normalised: the identity in the form sbn_g1_compress writes it
  if (!kz) for (size_t i = 0; i < s.Ld; i++) g1_compressed_normalise(proof + 32 * i, comp + 32 * i);
  else { g1_compressed_normalise(proof, kz->comm); g1_compressed_normalise(proof + L.off[spv::HASH_PROOF_DEREFS], kz->pi); memcpy(kz->y, proof + L.off[spv::HASH_PROOF_DEREFS] + 32, 32); }
  for (const SvOpening& o : op) for (size_t i = 0; i < o.sh.np; i++) g1_compressed_normalise(o.proof + 32 * i, comp + 32 * (o.pt0 + i));
  HIPCHK(c, hipMemsetAsync(d_ok, 0, 128 * okp, c->stream));
  HIPCHK(c, hipMemcpyAsync(p0 + o_comp, comp, 32 * NP, hipMemcpyHostToDevice, c->stream));
  LAUNCH(c, "k_g1_decompress", k_g1_decompress, (unsigned)((NP + 63) / 64), 64, (const uint32_t*)(p0 + o_comp), NP, (uint32_t*)nullptr, d_mont, d_ok);
  LAUNCHCHK(c);

  // ---- host: the transcript up to the product layer, ProductLayerProof::verify, the field part of HashLayerProof::verify ----
  sbn_host::Script ts{t};
  static const char NAME[] = "Sparse polynomial evaluation proof";
  ts.protocol(NAME);                                                  // sparse_mlpoly_full.rs:1824
  ts.message("derefs_commitment", "begin_derefs_commitment", 23);     // :341-347
  if (kz) ts.point("comm_poly_row_col_ops_val", kz->comm);           // :349-356 with kzg.rs:399-403: the 32 compressed bytes
  else {
    ts.message("comm_poly_row_col_ops_val", "poly_commitment_begin", 21);      // hyrax.rs:44-51
    for (size_t i = 0; i < s.Ld; i++) ts.point("poly_commitment_share", comp + 32 * i);
    ts.message("comm_poly_row_col_ops_val", "poly_commitment_end", 19);
  }
  ts.message("derefs_commitment", "end_derefs_commitment", 21);
  uint8_t rhb[64];
  ts.challenges("challenge_r_hash", rhb, 2);
  ts.protocol(NAME);                                                  // PolyEvalNetworkProof::verify
  spv::ProductFields pf{spv::field(L, proof, spv::PROD_EVAL_ROW), spv::field(L, proof, spv::PROD_EVAL_COL), spv::field(L, proof, spv::PROD_EVAL_VAL),
                        spv::field(L, proof, spv::PROD_PROOF_MEM), spv::field(L, proof, spv::PROD_PROOF_OPS)};
  spv::ProductClaims pc;
  if (!spv::product_layer_verify(ts, pf, s.N, s.cells, evals, s.batch, &pc)) return SBN_OK;
  const size_t m = s.ell_m;
  std::vector<El> rxe(m, from_u64(0)), rye(m, from_u64(0));           // equalize (:1681-1697): the shorter point gets zeros in front
  for (size_t j = 0; j < nx; j++) rxe[m - nx + j] = el_from(rx + 32 * j);
  for (size_t j = 0; j < ny; j++) rye[m - ny + j] = el_from(ry + 32 * j);
  spv::HashFields hf{spv::field(L, proof, spv::HASH_EVAL_ROW), spv::field(L, proof, spv::HASH_EVAL_COL), spv::field(L, proof, spv::HASH_EVAL_VAL), spv::field(L, proof, spv::HASH_EVAL_DEREFS)};
  spv::JointEvals je;
  if (pc.rand_mem.size() != m || pc.rand_ops.size() != s.L_ops) return SBN_OK;
  if (!spv::hash_layer_field(hf, s.batch, pc, rxe.data(), rye.data(), el_from(rhb), el_from(rhb + 32), &je)) return SBN_OK;
  ts.protocol("Sparse polynomial hash layer proof");                  // :1135
  ts.protocol(kz ? "Derefs evaluation proof (KZG)" : "Derefs evaluation proof");      // :467 / :512
  if (kz) {                                                           // derefs_reduce (:561-584): the claim is absorbed and not compared; then the opening's point
    joint_reduce(je.derefs.data(), s.cnt_d, s.lc_d, "evals_ops_val", "challenge_combine_n_to_one", "joint_claim_eval", (const uint8_t*)pc.rand_ops.data(), s.L_ops, t, op[0].rj, op[0].claim);
    ts.challenges("kzg_eval_point", kz->z, 1);
  }

  // ---- the three openings ----
  std::vector<uint8_t> Rv, Rv_right;                                  // R = eq(r_right) and the coordinates it was made of
  int pending = -1;                                                   // the opening whose row commit waits for the next hand-over to be in front of it
  for (int k = k0; k < SV_OPENINGS; k++) {
    SvOpening& o = op[k];
    if (k == 0) joint_reduce(je.derefs.data(), s.cnt_d, s.lc_d, "evals_ops_val", "challenge_combine_n_to_one", "joint_claim_eval", (const uint8_t*)pc.rand_ops.data(), s.L_ops, t, o.rj, o.claim);
    else if (k == 1) joint_reduce(je.ops.data(), s.cnt_o, s.lc_o, "claim_evals_ops", "challenge_combine_n_to_one", "joint_claim_eval_ops", (const uint8_t*)pc.rand_ops.data(), s.L_ops, t, o.rj, o.claim);
    else joint_reduce(je.mem.data(), 2, 1, "claim_evals_mem", "challenge_combine_two_to_one", "joint_claim_eval_mem", (const uint8_t*)pc.rand_mem.data(), m, t, o.rj, o.claim);
    // first stage: eq(r), C_LZ over the commitment's device points, C_Zr = Zr * gens_1.G[0] (column n of the derived set)
    if ((rc = opening_eq_launch(c, o.sh, o.rj.data(), d_L, (uint32_t*)(p0 + o_R), (uint32_t*)(p0 + o_s), d_Lc))) return rc;
    MsmShape s1;
    if ((rc = msm_single_launch(c, d_Lc, o.comm_pts, o.sh.L_size, o.comm, &s1))) return rc;
    if (s1.W < 1 || (size_t)s1.W > SV_STAGE_POINTS - SS_WINDOWS) return fail(c, SBN_EINVAL, "sparse verify: %d windows", s1.W);
    const size_t W = (size_t)s1.W, npts = W + SS_WINDOWS + (k == k0 ? okp : 0);
    HIPCHK(c, hipMemcpyAsync(d_stage, c->wsum.p, W * 128, hipMemcpyDeviceToDevice, c->stream));
    {
      uint32_t* d = (uint32_t*)(pin + h_d1 + desc_bytes * k);
      memset(d, 0, desc_bytes);
      d[0] = 1; d[SS_DESC_IDX] = (uint32_t)o.sh.n;                       // (the derived set holds n + 2 points: checked with the handle's size)
      memcpy(d + SS_DESC_SCAL, o.claim, 32);
      HIPCHK(c, hipMemcpyAsync(p0 + o_d1 + desc_bytes * k, d, desc_bytes, hipMemcpyHostToDevice, c->stream));
      LAUNCH(c, "k_window_sums", k_window_sums, (unsigned)SS_WINDOWS, 256, (const uint32_t*)(p0 + o_d1 + desc_bytes * k), (const uint32_t*)o.ext->d_pts, d_stage + 32 * W);
    }
    if (k == k0) HIPCHK(c, hipMemcpyAsync(d_stage + 32 * (W + SS_WINDOWS), d_ok, 128 * okp, hipMemcpyDeviceToDevice, c->stream));
    uint32_t seq = 0;
    if ((rc = sums_handover_begin(c, d_stage, npts, &seq))) return rc;
    // behind the hand-over: the previous opening's row commit, which the device works on while the host hashes
    if (pending >= 0) { if ((rc = row_commit(pending))) return rc; pending = -1; }
    // beside the device: a_vec = R on the host (the transcript needs its canonical bytes); once for two openings with the same right half
    if (Rv_right.size() != 32 * o.sh.mr || memcmp(Rv_right.data(), &o.rj[32 * o.sh.ml], 32 * o.sh.mr) != 0) {
      Rv_right.assign(o.rj.begin() + 32 * o.sh.ml, o.rj.end());
      polyeval_host_eq(Rv_right.data(), o.sh.mr, Rv);
    }
    const sbn_host::Pt* S = nullptr;
    if ((rc = sums_handover_wait(c, npts, seq, &S))) return rc;
    if (k == k0) {
      const uint8_t* ok = (const uint8_t*)(S + W + SS_WINDOWS);
      for (size_t i = 0; i < NP; i++) if (!ok[i]) return SBN_OK;      // a point of the proof does not decompress
    }
    sbn_host::to_affine_bytes(fold_windows(S, s1.W, s1.c), o.Cxy, nullptr);
    sbn_host::to_affine_bytes(fold_windows(S + W, SS_WINDOWS, SS_WINDOW_BITS), o.Cxy + 64, nullptr);
    // the opening's transcript lines and the scalars of its final equation
    uint8_t rq[32], cc[32];
    if (!polyeval_verify_script(ts, o.Cxy, Rv.data(), o.sh.n, comp + 32 * o.pt0, o.sh.lg, rq, cc, o.u, o.ui)) return SBN_OK;      // a challenge u = 0
    o.hs.assign(32 * (o.sh.np + 2), 0);
    o.fin = polyeval_verify_scalars(&o.rj[32 * o.sh.ml], o.sh.lg, o.u, o.ui, rq, cc, o.proof + 32 * o.sh.np, o.proof + 32 * o.sh.np + 32, o.hs.data());
    pending = k;
  }
  if ((rc = row_commit(pending))) return rc;

  // ---- the three final equations: one launch over the proof's points, Cx and Cy; one hand-over with the three commit sums ----
  memset(pin + h_df, 0, (h_total - h_df));                            // (an opening the KZG build does not have: a sum of no terms, not read)
  for (int k = k0; k < SV_OPENINGS; k++) {
    const SvOpening& o = op[k];
    uint32_t* d = (uint32_t*)(pin + h_df + desc_bytes * k);
    const size_t np = o.sh.np;
    d[0] = (uint32_t)(np + 2);                                        // at most 2 * 20 + 4 terms (the shape's check of ell)
    for (size_t i = 0; i < np; i++) d[SS_DESC_IDX + i] = (uint32_t)(o.pt0 + i);
    d[SS_DESC_IDX + np] = (uint32_t)(NP + 2 * k); d[SS_DESC_IDX + np + 1] = (uint32_t)(NP + 2 * k + 1);      // (d_mont holds NP + 6 points)
    memcpy(d + SS_DESC_SCAL, o.hs.data(), 32 * (np + 2));
    for (int q = 0; q < 4; q++) { const sbn_host::Fq v = fq_to_dev_mont(o.Cxy + 32 * q); memcpy(pin + h_cxy + 128 * k + 32 * q, v.v, 32); }
  }
  HIPCHK(c, hipMemcpyAsync(p0 + o_df, pin + h_df, SV_OPENINGS * desc_bytes, hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemcpyAsync(d_mont + 16 * NP, pin + h_cxy, SV_OPENINGS * 128, hipMemcpyHostToDevice, c->stream));
  LAUNCH(c, "k_window_sums", k_window_sums, (unsigned)(SV_OPENINGS * SS_WINDOWS), 256, (const uint32_t*)(p0 + o_df), (const uint32_t*)d_mont, d_fin);
  const sbn_host::Pt* S = nullptr;
  if ((rc = sums_handover(c, d_fin, SV_OPENINGS * SS_WINDOWS + SV_OPENINGS, &S))) return rc;
  bool all = true;
  for (int k = k0; k < SV_OPENINGS; k++)
    if (!sbn_host::is_inf(sbn_host::padd(fold_windows(S + (size_t)SS_WINDOWS * k, SS_WINDOWS, SS_WINDOW_BITS), sbn_host::pt_from_device(S[SV_OPENINGS * SS_WINDOWS + k])))) all = false;
  *accepted = all ? 1 : 0;
  return SBN_OK;
}

// what is misuse of either build's entry point (SBN_EINVAL before any launch), from the batch on; the pointers are the caller's to check.  `kzg`: the
// KZG build has no gens_derefs (gens: ops, mem, derefs or null), its layout and its proof size.  Out: the shape and the proof's layout
static int sparse_verify_args(sbn_ctx* c, const char* pfx, bool kzg, size_t num_vars_x, size_t num_vars_y, size_t num_ops, size_t num_cells, size_t batch,
                              const sbn_bases* comm_ops, const sbn_bases* comm_mem, const uint8_t* rx, const uint8_t* ry, const uint8_t* evals,
                              const sbn_bases* const gens[SV_OPENINGS], SparseEvalShape* sp, sbn_host::spv::Layout* Lp) {
  if (batch < 1 || batch > (size_t)SE_BATCH_MAX) return fail(c, SBN_EINVAL, "%s: batch = %zu is outside 1 .. %d", pfx, batch, SE_BATCH_MAX);
  if (num_ops < 2 || (num_ops & (num_ops - 1))) return fail(c, SBN_EINVAL, "%s: N = %zu (a power of two from 2 on)  [product_tree.rs:89 assert_eq]", pfx, num_ops);
  SparseEvalShape& s = *sp;
  sbn_host::spv::Layout& L = *Lp;
  if (!sparse_eval_shape(num_vars_x, num_vars_y, num_ops, batch, &s) || !sbn_host::spv::layout_make(num_vars_x, num_vars_y, num_ops, batch, &L, kzg) ||
      L.off[sbn_host::spv::NFIELDS] != (kzg ? s.proof_bytes_kzg : s.proof_bytes))
    return fail(c, SBN_EINVAL, "%s: shape (%zu, %zu, N = %zu, batch = %zu) is outside what the openings take", pfx, num_vars_x, num_vars_y, num_ops, batch);
  if (num_cells != s.cells) return fail(c, SBN_EINVAL, "%s: %zu memory cells, rx and ry have %zu and %zu variables  [sparse_mlpoly_full.rs:1828 assert_eq]", pfx, num_cells, num_vars_x, num_vars_y);
  const size_t rows_o = opening_shape(s.ell_o).L_size, rows_m = opening_shape(s.ell_mm).L_size;
  if (comm_ops->n != rows_o || comm_mem->n != rows_m)
    return fail(c, SBN_EINVAL, "%s: comm_ops has %zu and comm_mem %zu row commitments, the shape has %zu and %zu", pfx, comm_ops->n, comm_mem->n, rows_o, rows_m);
  const struct { size_t lg; const char* name; } gs[SV_OPENINGS] = {{s.lg_o, "gens_ops"}, {s.lg_m, "gens_mem"}, {s.lg_d, "gens_derefs"}};
  for (int k = 0; k < (kzg ? 2 : SV_OPENINGS); k++)
    if (gens[k]->n != ((size_t)1 << gs[k].lg) + 1 || !gens[k]->has_h)
      return fail(c, SBN_EINVAL, "%s: %s has %zu points%s, the opening needs %zu + 1 with h  [nizk/mod.rs:412-415]", pfx, gs[k].name, gens[k]->n, gens[k]->has_h ? "" : " and no h", (size_t)1 << gs[k].lg);
  const struct { const uint8_t* p; size_t n; const char* name; } sc[3] = {{rx, num_vars_x, "rx"}, {ry, num_vars_y, "ry"}, {evals, batch, "evals"}};
  for (const auto& x : sc)
    for (size_t i = 0; i < x.n; i++) if (!fr_canonical(x.p + 32 * i)) return fail(c, SBN_EINVAL, "%s: %s[%zu] is not canonical  [scalar.rs:87-95]", pfx, x.name, i);
  return SBN_OK;
}

extern "C" {

int sbn_sparse_eval_verify(sbn_ctx* c, size_t num_vars_x, size_t num_vars_y, size_t num_ops, size_t num_cells, size_t batch,
                           const sbn_bases* comm_ops, const sbn_bases* comm_mem, const uint8_t* rx, const uint8_t* ry, const uint8_t* evals,
                           const sbn_bases* gens_ops, const sbn_bases* gens_mem, const sbn_bases* gens_derefs, const uint8_t* proof, sbn_transcript* tr, int* accepted) {
  if (!c || !comm_ops || !comm_mem || (!rx && num_vars_x) || (!ry && num_vars_y) || !evals || !gens_ops || !gens_mem || !gens_derefs || !proof || !tr || !accepted) return SBN_EINVAL;
  SparseEvalShape s;
  sbn_host::spv::Layout L;
  const sbn_bases* const gens[SV_OPENINGS] = {gens_ops, gens_mem, gens_derefs};
  int rc;
  if ((rc = sparse_verify_args(c, "sparse verify", false, num_vars_x, num_vars_y, num_ops, num_cells, batch, comm_ops, comm_mem, rx, ry, evals, gens, &s, &L))) return rc;
  std::lock_guard<std::mutex> g(c->mu); hipSetDevice(c->device);
  return verify_on_copy(c, tr, accepted, [&](sbn_host::MerlinTranscript& t) {
    return sparse_verify_locked(c, s, L, comm_ops, comm_mem, rx, num_vars_x, ry, num_vars_y, evals, gens_ops, gens_mem, gens_derefs, proof, t, accepted);
  });
}

int sbn_sparse_eval_verify_kzg(sbn_ctx* c, size_t num_vars_x, size_t num_vars_y, size_t num_ops, size_t num_cells, size_t batch,
                               const sbn_bases* comm_ops, const sbn_bases* comm_mem, const uint8_t* rx, const uint8_t* ry, const uint8_t* evals,
                               const sbn_bases* gens_ops, const sbn_bases* gens_mem, const sbn_g2_lines* g2, const sbn_g2_lines* tau_g2,
                               const uint8_t* proof, sbn_transcript* tr, int* accepted) {
  if (!c || !comm_ops || !comm_mem || (!rx && num_vars_x) || (!ry && num_vars_y) || !evals || !gens_ops || !gens_mem || !g2 || !tau_g2 || !proof || !tr || !accepted) return SBN_EINVAL;
  if (g2->ctx != c || tau_g2->ctx != c) return fail(c, SBN_EINVAL, "sparse verify (KZG): a G2 handle of another context");
  SparseEvalShape s;
  sbn_host::spv::Layout L;
  const sbn_bases* const gens[SV_OPENINGS] = {gens_ops, gens_mem, nullptr};
  int rc;
  if ((rc = sparse_verify_args(c, "sparse verify (KZG)", true, num_vars_x, num_vars_y, num_ops, num_cells, batch, comm_ops, comm_mem, rx, ry, evals, gens, &s, &L))) return rc;
  // the field half, the transcript and the two Hyrax openings on a copy of the transcript, under the context's mutex.  Not verify_on_copy: its body
  // would hold the mutex through the pairing check, which takes it itself; what follows rc != SBN_OK and a refusal is what verify_on_copy does
  sbn_host::MerlinTranscript t = tr->t;
  SvKzg kz;
  int acc = 0;
  {
    std::lock_guard<std::mutex> g(c->mu); hipSetDevice(c->device);
    rc = sparse_verify_locked(c, s, L, comm_ops, comm_mem, rx, num_vars_x, ry, num_vars_y, evals, gens_ops, gens_mem, nullptr, proof, t, &acc, &kz);
    if (rc != SBN_OK) { hipStreamSynchronize(c->stream); return rc; }
  }
  if (!acc) { *accepted = 0; return SBN_OK; }
  // DerefsEvalProof::verify's KZGProof::verify (:586-594): the opening of comm_derefs at kzg_eval_point against the proof's own eval
  uint8_t comp[64], xy[128], ok[2] = {0, 0};
  memcpy(comp, kz.comm, 32); memcpy(comp + 32, kz.pi, 32);
  if ((rc = sbn_g1_decompress(c, comp, 2, xy, ok))) return rc;
  if (!ok[0] || !ok[1]) { *accepted = 0; return SBN_OK; }                // a point of the proof does not decompress
  static const uint8_t ONE[32] = {1};
  std::vector<uint8_t> pts(xy, xy + 64), scal(ONE, ONE + 32);
  int paired = 0;
  if ((rc = kzg_check_run(c, g2, tau_g2, pts, scal, kz.y, kz.z, xy + 64, &paired))) return rc;
  *accepted = paired;
  if (paired) tr->t = t;
  return SBN_OK;
}

}  // extern "C"
