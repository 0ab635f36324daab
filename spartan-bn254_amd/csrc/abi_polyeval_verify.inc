// abi_polyeval_verify.inc — C ABI: batched point decompression and the Hyrax opening CHECK in one call.  sbn_polyeval_verify is
// PolyEvalProof::verify / verify_plain (hyrax.rs:118-151) with DotProductProofLog::verify (nizk/mod.rs:525-567) and BulletReductionProof::verify
// (nizk/bullet.rs:130-173) inside, the Merlin transcript included; sbn_joint_opening_verify puts the n-to-1 reduction of the HashLayerProof openings
// (sparse_mlpoly_full.rs:434-457 and its siblings) in front of it.
//
// Two host waits.  Behind the first: C_LZ = sum L_i C_i (the MSM over the commitment's device points), C_Zr = Zr * gens_1.G[0] for verify_plain (a
// one-row commit over the derived set of the prover, polyeval_ext) and the flags of the proof's decompressed points.  The host then runs the
// transcript and the O(lg n) field work: b_hat = <s, R> = prod_k (u_k^-1 (1 - r_k) + u_k r_k) over the right-hand coordinates of r, both vectors
// being tensor products.  Behind the second: the reference's final equation (nizk/mod.rs:560-565) moved to one side,
//   a c (sum u_i^2 L_i + sum u_i^-2 R_i + Cx + r Cy) + a beta + delta - z1 sum_j s_j G_j - z1 a r G1 - z2 h = 0       (a = b_hat)
// as an MSM over the 2 lg n + 4 device points of the proof and ONE one-row commit of [-z1 s ‖ -z1 a r] with blind -z2 over the derived set
// (lookup table when the handle has one).  The window sums of the MSMs and the commits' sums go to the host together (k_points_to_host, one launch per wait);
// the host folds the windows (the 254-doubling chain) and tests for the identity.  No scalar multiplication runs on the CPU.
// The host half (the transcript lines, b_hat and the scalars: polyeval_verify_script, polyeval_verify_scalars, OpeningShape) is verify_host.hpp; the
// envelope, the hand-over, the MSM launches and the two device stages shared with the sparse check are abi_verify_common.inc and msm_host.hpp.
// Included by sbn254.hip; needs abi_verify_common.inc and abi_polyeval.inc (polyeval_ext).

// what is misuse (SBN_EINVAL before any launch); the pointers are the caller's to check
static int polyeval_verify_check(sbn_ctx* c, const sbn_bases* gens, const sbn_bases* comm, const uint8_t* r, size_t ell, const uint8_t* C_Zr_xy, const uint8_t* Zr) {
  if (ell == 0 || ell > 2 * (size_t)PE_SIDE_MAX) return fail(c, SBN_EINVAL, "polyeval verify: ell = %zu is outside 1 .. %d", ell, 2 * PE_SIDE_MAX);
  const OpeningShape sh = opening_shape(ell);
  const size_t L_size = sh.L_size, n = sh.n;
  if (comm->n != L_size) return fail(c, SBN_EINVAL, "polyeval verify: the commitment has %zu points, r has %zu variables (%zu rows)", comm->n, ell, L_size);
  if (gens->n != n + 1 || !gens->has_h) return fail(c, SBN_EINVAL, "polyeval verify: the generator set has %zu points%s, the opening needs %zu + 1 with h  [nizk/mod.rs:412-415]", gens->n, gens->has_h ? "" : " and no h", n);
  if ((C_Zr_xy != nullptr) == (Zr != nullptr)) return fail(c, SBN_EINVAL, "polyeval verify: exactly one of C_Zr_xy (verify) and Zr (verify_plain) is given");
  for (size_t j = 0; j < ell; j++) if (!fr_canonical(r + 32 * j)) return fail(c, SBN_EINVAL, "polyeval verify: r[%zu] is not canonical", j);
  if (Zr && !fr_canonical(Zr)) return fail(c, SBN_EINVAL, "polyeval verify: Zr is not canonical");
  if (C_Zr_xy && !g1_xy_valid(C_Zr_xy)) return fail(c, SBN_EINVAL, "polyeval verify: C_Zr is not a canonical point of the curve");
  return SBN_OK;
}

// the check on the transcript `t` (a copy of the caller's); arguments already checked.  SBN_OK with *accepted = 0: the proof is refused
static int polyeval_verify_locked(sbn_ctx* c, const sbn_bases* gens, const sbn_bases* comm, const uint8_t* r, size_t ell, const uint8_t* C_Zr_xy, const uint8_t* Zr,
                                  const uint8_t* proof, sbn_host::MerlinTranscript& t, int* accepted) {
  using namespace sbn_host::fr;
  *accepted = 0;
  const OpeningShape sh = opening_shape(ell);
  const size_t ml = sh.ml, mr = sh.mr, L_size = sh.L_size, n = sh.n, lg = sh.lg, np = sh.np;      // np: the proof's points L, R, delta, beta; Cx and Cy follow them on the device
  const uint8_t* z1b = proof + 64 * lg + 64; const uint8_t* z2b = z1b + 32;
  if (!fr_canonical(z1b) || !fr_canonical(z2b)) return SBN_OK;    // Scalar::from_bytes fails (scalar.rs:87-95)
  sbn_host::Script ts{t};
  int rc;
  const sbn_bases* ext = nullptr;
  if ((rc = polyeval_ext(c, gens, &ext))) return rc;
  if ((rc = ensure_pin(c, 8192))) return rc;
  if ((rc = ensure(c, c->wsum, 4096))) return rc;

  // device state: L (table form), L (canonical), R and s of k_polyeval_eq, the commit row with its blind, the staged sums, the proof's points
  const size_t o_L = 0, o_Lc = o_L + 32 * L_size, o_R = o_Lc + 32 * L_size, o_s = o_R + 32 * n, o_row = o_s + 32 * n, o_stage = o_row + 32 * (n + 2),
               o_comp = o_stage + 128 * VERIFY_STAGE_POINTS, o_pts = o_comp + 32 * np, o_scal = o_pts + 64 * (np + 2), o_ok = o_scal + 32 * (np + 2), total = o_ok + 64;
  SlabLease slab(c);
  if ((rc = slab.get(total, "polyeval verify state"))) return rc;
  uint8_t* p0 = (uint8_t*)slab.p;
  uint32_t* d_L = (uint32_t*)(p0 + o_L); uint32_t* d_Lc = (uint32_t*)(p0 + o_Lc); uint32_t* d_row = (uint32_t*)(p0 + o_row); uint32_t* d_stage = (uint32_t*)(p0 + o_stage);
  uint32_t* d_comp = (uint32_t*)(p0 + o_comp); uint32_t* d_pts = (uint32_t*)(p0 + o_pts); uint32_t* d_scal = (uint32_t*)(p0 + o_scal); uint8_t* d_ok = p0 + o_ok;
  uint8_t* pin = (uint8_t*)c->pin;

  // ---- first launch: the proof's points, eq(r_left), C_LZ, C_Zr ----
  uint8_t comp[44 * 32];                                          // np <= 42; the identity in the form sbn_g1_compress writes it
  for (size_t i = 0; i < np; i++) g1_compressed_normalise(proof + 32 * i, comp + 32 * i);
  memcpy(pin, comp, 32 * np);
  HIPCHK(c, hipMemsetAsync(d_ok, 0, 64, c->stream));
  HIPCHK(c, hipMemcpyAsync(d_comp, pin, 32 * np, hipMemcpyHostToDevice, c->stream));
  LAUNCH(c, "k_g1_decompress", k_g1_decompress, (unsigned)((np + 63) / 64), 64, (const uint32_t*)d_comp, np, (uint32_t*)nullptr, d_pts, d_ok);
  if ((rc = opening_eq_launch(c, sh, r, d_L, (uint32_t*)(p0 + o_R), (uint32_t*)(p0 + o_s), d_Lc))) return rc;
  MsmShape s1;
  if ((rc = msm_single_launch(c, d_Lc, (const uint32_t*)comm->d_pts, L_size, comm, &s1))) return rc;
  if (s1.W + 2 > VERIFY_STAGE_POINTS) return fail(c, SBN_EINVAL, "polyeval verify: %d windows", s1.W);
  HIPCHK(c, hipMemcpyAsync(d_stage, c->wsum.p, (size_t)s1.W * 128, hipMemcpyDeviceToDevice, c->stream));
  size_t npts1 = (size_t)s1.W;
  if (Zr) {                                                       // C_Zr = Zr.commit(0, gens_1) (hyrax.rs:147): the row [0 ... 0 ‖ Zr], blind 0
    memcpy(pin + 2048, Zr, 32);
    HIPCHK(c, hipMemsetAsync(d_row, 0, 32 * (n + 2), c->stream));
    HIPCHK(c, hipMemcpyAsync(d_row + 8 * n, pin + 2048, 32, hipMemcpyHostToDevice, c->stream));
    RowInfo ri; ri.internal_rows = true;
    if ((rc = commit_rows_launch(c, ext, d_row, d_row + 8 * (n + 1), 1, n + 1, nullptr, nullptr, ri))) return rc;
    HIPCHK(c, hipMemcpyAsync(d_stage + 32 * npts1, c->wsum.p, 128, hipMemcpyDeviceToDevice, c->stream));
    npts1++;
  }
  sbn_host::Pt S[VERIFY_STAGE_POINTS]; uint32_t okw[16];
  // beside the device: a_vec = R on the host (the transcript needs its canonical bytes)
  std::vector<uint8_t> Rv;
  polyeval_host_eq(r + 32 * ml, mr, Rv);
  if ((rc = verify_handover(c, d_stage, npts1, (const uint32_t*)d_ok, (uint32_t)((np + 3) / 4), S, okw))) return rc;
  for (size_t i = 0; i < np; i++) if (!((const uint8_t*)okw)[i]) return SBN_OK;      // a point of the proof does not decompress
  uint8_t Cxy[128];                                               // Cx ‖ Cy
  sbn_host::to_affine_bytes(fold_windows(S, s1.W, s1.c), Cxy, nullptr);
  if (Zr) sbn_host::to_affine_bytes(sbn_host::pt_from_device(S[s1.W]), Cxy + 64, nullptr); else memcpy(Cxy + 64, C_Zr_xy, 64);

  // ---- the transcript, as the reference's verifier writes it ----
  uint8_t rq[32], cc[32];
  std::vector<El> u, ui;
  if (!polyeval_verify_script(ts, Cxy, Rv.data(), n, comp, lg, rq, cc, u, ui)) return SBN_OK;      // a challenge u = 0

  // ---- O(lg n) field work: b_hat in closed form, the scalars of the proof's points, the row's constants ----
  uint8_t* hs = pin + 4096;                                       // (np + 2) scalars, then Cx ‖ Cy
  const PolyevalFinal fin = polyeval_verify_scalars(r + 32 * ml, lg, u, ui, rq, cc, z1b, z2b, hs);
  memcpy(hs + 32 * (np + 2), Cxy, 128);

  // ---- second launch: the folded equation ----
  HIPCHK(c, hipMemcpyAsync(d_scal, hs, 32 * (np + 2), hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemcpyAsync(d_pts + 16 * np, hs + 32 * (np + 2), 128, hipMemcpyHostToDevice, c->stream));
  LAUNCH(c, "k_points_to_mont", k_points_to_mont, 1, 256, (const uint32_t*)(d_pts + 16 * np), d_pts + 16 * np, (size_t)2);
  MsmShape s2;
  if ((rc = msm_single_launch(c, d_scal, d_pts, np + 2, nullptr, &s2))) return rc;
  if (s2.W + 2 > VERIFY_STAGE_POINTS) return fail(c, SBN_EINVAL, "polyeval verify: %d windows", s2.W);
  HIPCHK(c, hipMemcpyAsync(d_stage, c->wsum.p, (size_t)s2.W * 128, hipMemcpyDeviceToDevice, c->stream));
  if ((rc = opening_row_commit(c, sh, ext, u, ui, fin, d_row, d_stage + 32 * (size_t)s2.W))) return rc;
  if ((rc = verify_handover(c, d_stage, (size_t)s2.W + 1, nullptr, 0, S, nullptr))) return rc;
  const sbn_host::Pt sum = sbn_host::padd(fold_windows(S, s2.W, s2.c), sbn_host::pt_from_device(S[s2.W]));
  *accepted = sbn_host::is_inf(sum) ? 1 : 0;
  return SBN_OK;
}

extern "C" {

int sbn_g1_decompress(sbn_ctx* c, const uint8_t* in32, size_t n, uint8_t* out_xy, uint8_t* out_ok) {
  if (!c || ((!in32 || !out_xy || !out_ok) && n)) return SBN_EINVAL;
  if (n == 0) return SBN_OK;
  std::lock_guard<std::mutex> g(c->mu); hipSetDevice(c->device);
  int rc;
  if ((rc = ensure(c, c->stage_pts, g1_decompress_stage_bytes(n)))) return rc;
  return g1_decompress_run(c, in32, n, nullptr, out_xy, out_ok);
}

int sbn_bases_from_compressed(sbn_ctx* c, const uint8_t* in32, size_t n, sbn_bases** out, size_t* bad_index) {
  if (!c || !out || (!in32 && n)) return SBN_EINVAL;
  *out = nullptr;
  std::lock_guard<std::mutex> g(c->mu); hipSetDevice(c->device);
  return bases_from_compressed_locked(c, in32, n, out, bad_index);
}

int sbn_polyeval_verify(sbn_ctx* c, const sbn_bases* gens, const sbn_bases* comm, const uint8_t* r, size_t ell, const uint8_t* C_Zr_xy, const uint8_t* Zr,
                        const uint8_t* proof, sbn_transcript* tr, int* accepted) {
  if (!c || !gens || !comm || !r || !proof || !tr || !accepted) return SBN_EINVAL;
  int rc;
  if ((rc = polyeval_verify_check(c, gens, comm, r, ell, C_Zr_xy, Zr))) return rc;
  std::lock_guard<std::mutex> g(c->mu); hipSetDevice(c->device);
  return verify_on_copy(c, tr, accepted, [&](sbn_host::MerlinTranscript& t) { return polyeval_verify_locked(c, gens, comm, r, ell, C_Zr_xy, Zr, proof, t, accepted); });
}

int sbn_joint_opening_verify(sbn_ctx* c, const sbn_bases* gens, const sbn_bases* comm, const uint8_t* evals, size_t count,
                             const uint8_t* label_evals, size_t label_evals_len, const uint8_t* label_chal, size_t label_chal_len,
                             const uint8_t* label_claim, size_t label_claim_len, const uint8_t* r, size_t ell_r,
                             const uint8_t* proof, sbn_transcript* tr, uint8_t* out_challenges, int* accepted) {
  if (!c || !gens || !comm || !evals || !label_evals || !label_chal || !label_claim || (!r && ell_r) || !proof || !tr || !accepted) return SBN_EINVAL;
  if (count == 0 || (count & (count - 1)) || count > ((size_t)1 << 20)) return fail(c, SBN_EINVAL, "joint opening: %zu evals (a power of two is needed: the caller pads)", count);
  size_t lc = 0; while (((size_t)1 << lc) < count) lc++;
  for (size_t i = 0; i < count; i++) if (!fr_canonical(evals + 32 * i)) return fail(c, SBN_EINVAL, "joint opening: evals[%zu] is not canonical", i);
  const size_t ell = lc + ell_r;
  if (ell == 0 || ell > 2 * (size_t)PE_SIDE_MAX) return fail(c, SBN_EINVAL, "joint opening: %zu variables", ell);
  for (size_t j = 0; j < ell_r; j++) if (!fr_canonical(r + 32 * j)) return fail(c, SBN_EINVAL, "joint opening: r[%zu] is not canonical", j);
  std::lock_guard<std::mutex> g(c->mu); hipSetDevice(c->device);
  using sbn_host::Label;
  std::vector<uint8_t> rj;
  const int rc = verify_on_copy(c, tr, accepted, [&](sbn_host::MerlinTranscript& t) -> int {
    uint8_t claim[32];
    joint_reduce(evals, count, lc, Label(label_evals, label_evals_len), Label(label_chal, label_chal_len), Label(label_claim, label_claim_len), r, ell_r, t, rj, claim);
    int rc2;
    if ((rc2 = polyeval_verify_check(c, gens, comm, rj.data(), ell, nullptr, claim))) return rc2;      // (sizes: before any launch; the challenges are canonical)
    return polyeval_verify_locked(c, gens, comm, rj.data(), ell, nullptr, claim, proof, t, accepted);
  });
  if (rc == SBN_OK && lc && out_challenges) memcpy(out_challenges, rj.data(), 32 * lc);
  return rc;
}

}  // extern "C"
