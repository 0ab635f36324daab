// abi_verify_common.inc — what the one-call verifiers share on the device side, the counterpart of abi_proof_common.inc (DESIGN §4.16a).  Their host
// arithmetic is verify_host.hpp; their single MSM and its fold are msm_single_launch and fold_windows (msm_host.hpp), their device state a SlabLease
// (ctx.hpp).  What belongs here: code with a launch or a wait in it that more than one verifier runs —
//   verify_on_copy                     the envelope of a check: a copy of the transcript, stored back only behind accepted = 1
//   vbox_ensure, verify_handover       sums to the host, the small area        sbox_ensure, sums_handover[_begin / _wait]      the large one
//   g1_decompress_run, bases_from_compressed_locked      compressed points through the staging buffer
//   opening_point, opening_eq_launch, opening_row_commit  the two device stages every Hyrax opening check has
// Included by sbn254.hip right after abi_proof_common.inc; needs abi_msm.inc (commit_rows_launch, bases_build_dedupe) and abi_tables.inc (scs_from).

// the check runs on a copy of the caller's transcript, which moves on only behind an accepted proof; behind a failure nothing stays queued
template <class Body>
static int verify_on_copy(sbn_ctx* c, sbn_transcript* tr, int* accepted, Body body) {
  sbn_host::MerlinTranscript t = tr->t;
  *accepted = 0;
  const int rc = body(t);
  if (rc != SBN_OK) { hipStreamSynchronize(c->stream); *accepted = 0; return rc; }
  if (*accepted) tr->t = t;
  return SBN_OK;
}

// ---- sums to the host.  Two areas and two kernels, on purpose: k_points_to_host runs ONE block, takes up to 64 points and carries extra words
// (decompression flags, a proof point) behind them to one flag word — the shape of an opening check's wait; k_sums_to_host is many-block with a flag
// per block and no extra words — the shape of up to 256 x 64 window sums.  Neither does the other's job at the other's cost ----
static const int VERIFY_STAGE_POINTS = 64;      // window sums of one MSM (<= 37 at c = 7, the narrowest window) and two commit sums
static const uint32_t VBOX_EXTRA_WORDS = 16, VBOX_FLAG_WORD = 32 * VERIFY_STAGE_POINTS + VBOX_EXTRA_WORDS, VBOX_WORDS = VBOX_FLAG_WORD + 16;
// the hand-over area, allocated on first use
static int vbox_ensure(sbn_ctx* c) {
  if (!c->vbox) {
    uint32_t* vb = nullptr;
    HIPCHK(c, hipHostMalloc((void**)&vb, VBOX_WORDS * 4, hipHostMallocMapped | hipHostMallocCoherent));
    memset(vb, 0, VBOX_WORDS * 4);
    c->vbox = vb;
  }
  return sc_tickets(c);                                                 // (the mailbox whose sequence numbers the flag takes)
}
// `npoints` XYZZ sums at d_pts and the `nextra` words at d_extra to the host in ONE launch and ONE wait: the hand-over of a bullet round
// (k_points_to_host, sc_flag_wait) into an area of its own — the window sums of an MSM do not fit the mailbox's final-claims words
static int verify_handover(sbn_ctx* c, const uint32_t* d_pts, size_t npoints, const uint32_t* d_extra, uint32_t nextra, sbn_host::Pt* out, uint32_t* extra_out) {
  int rc;
  if (npoints > (size_t)VERIFY_STAGE_POINTS || nextra > VBOX_EXTRA_WORDS) return fail(c, SBN_EINVAL, "polyeval verify: %zu points and %u words do not fit the hand-over area", npoints, nextra);
  if ((rc = vbox_ensure(c))) return rc;
  const uint32_t seq = ++c->mbox_seq;
  LAUNCH(c, "k_points_to_host", k_points_to_host, 1, 256, d_pts, (uint32_t)npoints, d_extra, nextra, c->vbox, c->vbox + VBOX_FLAG_WORD, seq);
  LAUNCHCHK(c);
  if ((rc = sc_flag_wait(c, c->vbox + VBOX_FLAG_WORD, seq))) return rc;
  memcpy(out, c->vbox, npoints * 128);
  if (nextra) memcpy(extra_out, c->vbox + 32 * npoints, nextra * 4);
  return SBN_OK;
}

static const uint32_t SBOX_FLAG_WORDS = 256;      // one flag per block of k_sums_to_host, in front of the sums
// the hand-over area of the window sums, sized on first use and grown when a call brings more: vbox holds 64 points, a call here up to 256 x 64
static int sbox_ensure(sbn_ctx* c, size_t npoints) {
  const size_t words = SBOX_FLAG_WORDS + 32 * npoints;
  if (words <= c->sbox_words) return SBN_OK;
  if (c->sbox) { HIPCHK(c, hipStreamSynchronize(c->stream)); HIPCHK(c, hipHostFree(c->sbox)); c->sbox = nullptr; c->sbox_words = 0; }
  uint32_t* sb = nullptr;
  HIPCHK(c, hipHostMalloc((void**)&sb, words * 4, hipHostMallocMapped | hipHostMallocCoherent));
  memset(sb, 0, words * 4);
  c->sbox = sb; c->sbox_words = words;
  return SBN_OK;
}
// `npoints` XYZZ sums at d_sums to the host in ONE launch (sums_handover_begin) and ONE wait (sums_handover_wait); *out: the sums as the device left
// them, valid until the next hand-over.  Between the two a caller may enqueue work that the host does not wait for
static int sums_handover_begin(sbn_ctx* c, const uint32_t* d_sums, size_t npoints, uint32_t* seq_out) {
  int rc;
  const size_t nblk = (npoints + SS_HANDOVER_POINTS - 1) / SS_HANDOVER_POINTS;
  if (npoints == 0 || nblk > (size_t)SBOX_FLAG_WORDS) return fail(c, SBN_EINVAL, "small sums: %zu points do not fit the hand-over area", npoints);
  if ((rc = sbox_ensure(c, npoints))) return rc;
  const uint32_t seq = ++c->mbox_seq;
  LAUNCH(c, "k_sums_to_host", k_sums_to_host, (unsigned)nblk, 256, (const uint4*)d_sums, (uint32_t)(8 * npoints), (uint4*)(c->sbox + SBOX_FLAG_WORDS), c->sbox, seq);
  LAUNCHCHK(c);
  *seq_out = seq;
  return SBN_OK;
}
static int sums_handover_wait(sbn_ctx* c, size_t npoints, uint32_t seq, const sbn_host::Pt** out) {
  const size_t nblk = (npoints + SS_HANDOVER_POINTS - 1) / SS_HANDOVER_POINTS;
  // a short spin on the flags (a count of polls, not a time: enough for a call of a few sums, whose kernel is tens of microseconds), then the
  // ordinary stream synchronisation, which is the normal path of a large call (256 sums: 2.3 ms of kernel) and of every call with profiling on
  volatile uint32_t* fl = c->sbox;
  bool seen = false;
  if (!c->prof) {
    for (int spin = 0; spin < 200000 && !seen; spin++) {
      size_t done = 0; while (done < nblk && fl[done] == seq) done++;
      if (done == nblk) { std::atomic_thread_fence(std::memory_order_acquire); seen = true; }
    }
  }
  if (!seen) {
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (c->prof) prof_drain(c);
    for (size_t i = 0; i < nblk; i++) if (fl[i] != seq) return fail(c, SBN_EHIP, "small sums: result flag %zu missing after synchronisation", i);
  }
  *out = (const sbn_host::Pt*)(c->sbox + SBOX_FLAG_WORDS);
  return SBN_OK;
}
static int sums_handover(sbn_ctx* c, const uint32_t* d_sums, size_t npoints, const sbn_host::Pt** out) {
  int rc; uint32_t seq = 0;
  if ((rc = sums_handover_begin(c, d_sums, npoints, &seq))) return rc;
  return sums_handover_wait(c, npoints, seq, out);
}

// ---- compressed points through the context's staging buffer ----
static inline size_t g1_decompress_stage_bytes(size_t n) { return 32 * n + 64 * n + n; }      // the compressed bytes, canonical x ‖ y, the flags
// n >= 1 compressed points at in32 (c->stage_pts holds g1_decompress_stage_bytes(n)): the upload, ONE k_g1_decompress (d_mont: the points in table
// layout as well, or null), canonical x ‖ y and one flag per point to the host, ONE wait
static int g1_decompress_run(sbn_ctx* c, const uint8_t* in32, size_t n, uint32_t* d_mont, uint8_t* out_xy, uint8_t* out_ok) {
  uint8_t* p = (uint8_t*)c->stage_pts.p;
  const size_t o_xy = 32 * n, o_ok = o_xy + 64 * n;
  HIPCHK(c, hipMemcpyAsync(p, in32, 32 * n, hipMemcpyHostToDevice, c->stream));
  LAUNCH(c, "k_g1_decompress", k_g1_decompress, (unsigned)((n + 63) / 64), 64, (const uint32_t*)p, n, (uint32_t*)(p + o_xy), d_mont, p + o_ok);
  LAUNCHCHK(c);
  HIPCHK(c, hipMemcpyAsync(out_xy, p + o_xy, 64 * n, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipMemcpyAsync(out_ok, p + o_ok, n, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  if (c->prof) prof_drain(c);
  return SBN_OK;
}
// sbn_bases_from_compressed with the context's mutex held: a handle over n decompressed points.  A point that does not decompress is SBN_EINVAL
// with its index in *bad_index (which the caller set to SIZE_MAX to tell it from other misuse)
static int bases_from_compressed_locked(sbn_ctx* c, const uint8_t* in32, size_t n, sbn_bases** out, size_t* bad_index) {
  int rc;
  if ((rc = ensure(c, c->stage_pts, g1_decompress_stage_bytes(n) + 64))) return rc;
  sbn_bases* b = new sbn_bases(); b->n = n; b->has_h = false;
  hipError_t e = hipMalloc(&b->d_pts, (n ? n : 1) * 64);
  if (e != hipSuccess) { delete b; return fail(c, SBN_ENOMEM, "hipMalloc bases: %s", hipGetErrorString(e)); }
  std::vector<uint8_t> xy(64 * n), ok(n);
  if (n && (rc = g1_decompress_run(c, in32, n, (uint32_t*)b->d_pts, xy.data(), ok.data()))) { hipStreamSynchronize(c->stream); sbn_bases_free(c, b); return rc; }
  for (size_t i = 0; i < n; i++)
    if (!ok[i]) {
      if (bad_index) *bad_index = i;
      sbn_bases_free(c, b);
      return fail(c, SBN_EINVAL, "bases_from_compressed: point %zu does not decompress  [group.rs:323-329]", i);
    }
  std::vector<std::string> keys(n);
  for (size_t j = 0; j < n; j++) keys[j].assign((const char*)&xy[64 * j], 64);
  if (n && (rc = bases_build_dedupe(c, b, keys))) { sbn_bases_free(c, b); return rc; }
  *out = b;
  return SBN_OK;
}

// ---- the device stages of a Hyrax opening check (polyeval_verify_locked, sparse_verify_locked) ----
// the opening's point r (sh.ell canonical scalars) as k_polyeval_eq takes it: left and right coordinates in the device's Montgomery form
static PolyEvalPoint opening_point(const OpeningShape& sh, const uint8_t* r) {
  using namespace sbn_host::fr;
  PolyEvalPoint pt; memset(&pt, 0, sizeof pt);
  for (size_t j = 0; j < sh.ml; j++) { const El x = to_dev_mont(el_from(r + 32 * j)); memcpy(pt.l[j], x.v, 32); }
  for (size_t j = 0; j < sh.mr; j++) { const El x = to_dev_mont(el_from(r + 32 * (sh.ml + j))); memcpy(pt.r[j], x.v, 32); }
  return pt;
}
// first stage, launches only: L = eq(r_left) (table form, d_L), R = eq(r_right) and s (d_R, d_s), L as canonical scalars for the MSM (d_Lc)
static int opening_eq_launch(sbn_ctx* c, const OpeningShape& sh, const uint8_t* r, uint32_t* d_L, uint32_t* d_R, uint32_t* d_s, uint32_t* d_Lc) {
  LAUNCH(c, "k_polyeval_eq", k_polyeval_eq, (unsigned)((std::max(sh.n, sh.L_size) + 255) / 256), 256, opening_point(sh, r), (int)sh.ml, (int)sh.mr, d_L, d_R, d_s);
  LAUNCH(c, "k_scalars_from_mont", k_scalars_from_internal, (unsigned)((sh.L_size + 255) / 256), 256, (const uint32_t*)d_L, d_Lc, sh.L_size);
  return SBN_OK;
}
// second stage, launches only: the row -z1 s ‖ -z1 a r with blind -z2 of the final equation (d_row: n + 2 scalars) and its ONE one-row commit over
// the derived set `ext`; the sum (XYZZ, 128 bytes) lands at d_dst
static int opening_row_commit(sbn_ctx* c, const OpeningShape& sh, const sbn_bases* ext, const std::vector<sbn_host::fr::El>& u, const std::vector<sbn_host::fr::El>& ui,
                              const PolyevalFinal& fin, uint32_t* d_row, uint32_t* d_dst) {
  using namespace sbn_host::fr;
  int rc;
  PolyEvalPoint U; memset(&U, 0, sizeof U);
  for (size_t k = 0; k < sh.lg; k++) { const El a = to_dev_mont(u[k]), b = to_dev_mont(ui[k]); memcpy(U.l[k], a.v, 32); memcpy(U.r[k], b.v, 32); }
  LAUNCH(c, "k_polyeval_verify_row", k_polyeval_verify_row, (unsigned)((sh.n + 255) / 256), 256, U, (int)sh.lg, scs_from(to_dev_mont(fin.nz1)), scs_from(fin.tail), scs_from(fin.nz2), d_row, d_row + 8 * (sh.n + 1));
  RowInfo ri; ri.internal_rows = true;
  if ((rc = commit_rows_launch(c, ext, d_row, d_row + 8 * (sh.n + 1), 1, sh.n + 1, nullptr, nullptr, ri))) return rc;
  HIPCHK(c, hipMemcpyAsync(d_dst, c->wsum.p, 128, hipMemcpyDeviceToDevice, c->stream));
  return SBN_OK;
}
