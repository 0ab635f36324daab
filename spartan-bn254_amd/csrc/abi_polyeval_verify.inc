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
// Included by sbn254.hip.

// the bucket pipeline of msm_device (msm_host.hpp) without its hand-over: the window sums stay in c->wsum (shape->W x XYZZ) — launches only
static int msm_windows_launch(sbn_ctx* c, const uint32_t* d_scal, const uint32_t* d_bases, size_t n, const sbn_bases* b, MsmShape* shape) {
  if (n == 0 || n > 0x7fffffffull) return fail(c, SBN_EINVAL, "msm: n=%zu is outside 1 .. 2^31-1", n);
  BucketJob J; memset(&J, 0, sizeof J);
  J.mode = MODE_SINGLE;
  const MsmOverrides o = msm_overrides_read();
  {
    int cm = 1; while ((1 << cm) < c->sort_rs_max) cm++;
    const bool s2 = sort2_applies(c, MODE_SINGLE, n, S2_C_MIN);
    J.s = choose_shape(o, n, false, s2 ? S2_C_MAX : cm + 1, 1, s2 ? S2_C_MAX : MSM_C_MAX);
  }
  J.P = (size_t)J.s.W; J.threads = n; J.points = d_bases;
  J.da.scalars = d_scal; J.da.n = n; J.da.estride = n; J.da.bad = c->d_bad;
  int rc;
  if (glv_applies(c, o, b, n, J.s)) {
    const uint32_t* tab;
    if ((rc = bases_glv_table(c, b, &tab))) return rc;
    if ((rc = ensure(c, c->glv_scal, 2 * n * 16))) return rc;
    J.s = glv_shape(o, n); J.P = (size_t)J.s.W; J.threads = 2 * n; J.points = tab;
    J.da.scalars = (const uint32_t*)c->glv_scal.p; J.da.n = 2 * n; J.da.estride = 2 * n;
    J.glv = true; J.glv_gap = b->n + (b->has_h ? 1 : 0) - n;
    LAUNCH(c, "k_glv_split", k_glv_split, (unsigned)((n + 255) / 256), 256, d_scal, n, (uint32_t*)c->glv_scal.p, c->d_bad);
  }
  if ((rc = run_bucket_job(c, J, o))) return rc;
  *shape = J.s;
  return SBN_OK;
}

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
// sum_w 2^(c w) S_w of window sums as the device left them
static sbn_host::Pt verify_fold_windows(const sbn_host::Pt* S, const MsmShape& s) {
  std::vector<sbn_host::Pt> W((size_t)s.W);
  for (int w = 0; w < s.W; w++) W[(size_t)w] = sbn_host::pt_from_device(S[w]);
  return sbn_host::combine_windows(W.data(), s.W, s.c);
}

// canonical affine x || y on the curve y^2 = x^3 + 3, or the all-zero identity
static bool g1_xy_valid(const uint8_t xy[64]) {
  bool inf = true; for (int k = 0; k < 64; k++) if (xy[k]) { inf = false; break; }
  if (inf) return true;
  sbn_host::Fq x, y; memcpy(x.v, xy, 32); memcpy(y.v, xy + 32, 32);
  if (sbn_host::geq_p(x.v) || sbn_host::geq_p(y.v)) return false;
  const sbn_host::Fq three = {{3, 0, 0, 0}};
  const sbn_host::Fq xm = sbn_host::to_mont(x), ym = sbn_host::to_mont(y);
  const sbn_host::Fq rhs = sbn_host::add(sbn_host::mul(sbn_host::sqr(xm), xm), sbn_host::to_mont(three)), lhs = sbn_host::sqr(ym);
  return memcmp(lhs.v, rhs.v, 32) == 0;
}

// what is misuse (SBN_EINVAL before any launch); the pointers are the caller's to check
static int polyeval_verify_check(sbn_ctx* c, const sbn_bases* gens, const sbn_bases* comm, const uint8_t* r, size_t ell, const uint8_t* C_Zr_xy, const uint8_t* Zr) {
  if (ell == 0 || ell > 2 * (size_t)PE_SIDE_MAX) return fail(c, SBN_EINVAL, "polyeval verify: ell = %zu is outside 1 .. %d", ell, 2 * PE_SIDE_MAX);
  const size_t ml = ell / 2, mr = ell - ml, L_size = (size_t)1 << ml, n = (size_t)1 << mr;
  if (comm->n != L_size) return fail(c, SBN_EINVAL, "polyeval verify: the commitment has %zu points, r has %zu variables (%zu rows)", comm->n, ell, L_size);
  if (gens->n != n + 1 || !gens->has_h) return fail(c, SBN_EINVAL, "polyeval verify: the generator set has %zu points%s, the opening needs %zu + 1 with h  [nizk/mod.rs:412-415]", gens->n, gens->has_h ? "" : " and no h", n);
  if ((C_Zr_xy != nullptr) == (Zr != nullptr)) return fail(c, SBN_EINVAL, "polyeval verify: exactly one of C_Zr_xy (verify) and Zr (verify_plain) is given");
  for (size_t j = 0; j < ell; j++) if (!fr_canonical(r + 32 * j)) return fail(c, SBN_EINVAL, "polyeval verify: r[%zu] is not canonical", j);
  if (Zr && !fr_canonical(Zr)) return fail(c, SBN_EINVAL, "polyeval verify: Zr is not canonical");
  if (C_Zr_xy && !g1_xy_valid(C_Zr_xy)) return fail(c, SBN_EINVAL, "polyeval verify: C_Zr is not a canonical point of the curve");
  return SBN_OK;
}

// the transcript lines of PolyEvalProof::verify_plain / verify with DotProductProofLog::verify and BulletReductionProof::verify inside (hyrax.rs:127,
// nizk/mod.rs:538-556, bullet.rs:147-153), as every opening check writes them.  Cxy: Cx ‖ Cy; Rv: a_vec = R, n scalars; comp: the proof's 2 lg + 2
// normalised points.  Out: the challenges r and c, u and their inverses.  false: a challenge u = 0 has no inverse (bullet.rs:161-165)
static bool polyeval_verify_script(sbn_host::Script& ts, const uint8_t Cxy[128], const uint8_t* Rv, size_t n, const uint8_t* comp, size_t lg,
                                   uint8_t rq[32], uint8_t cc[32], std::vector<sbn_host::fr::El>& u, std::vector<sbn_host::fr::El>& ui) {
  using namespace sbn_host::fr;
  uint8_t c32[32];
  ts.protocol("polynomial evaluation proof");                     // hyrax.rs:127
  ts.protocol("dot product proof (log)");                         // nizk/mod.rs:538
  ts.point_xy("Cx", Cxy, c32);                                    // :543-545
  ts.point_xy("Cy", Cxy + 64, c32);
  ts.scalars("a", Rv, n);
  ts.challenge("r", rq);                                          // :548
  u.assign(lg, from_u64(0)); ui.assign(lg, from_u64(0));
  for (size_t j = 0; j < lg; j++) {                               // bullet.rs:147-153
    ts.point("L", comp + 32 * j);
    ts.point("R", comp + 32 * (lg + j));
    uint8_t ub[32];
    ts.challenge("u", ub);
    u[j] = el_from(ub);
    if (is_zero(u[j])) return false;                              // no inverse (bullet.rs:161-165)
    ui[j] = inv(u[j]);
  }
  ts.point("delta", comp + 64 * lg);                              // nizk/mod.rs:555-556
  ts.point("beta", comp + 64 * lg + 32);
  ts.challenge("c", cc);
  return true;
}
// b_hat = <s, R> in closed form over the right-hand coordinates r_right, the scalars of the final equation's 2 lg + 4 points (L, R, delta, beta, Cx,
// Cy) into hs, and the constants of the row -z1 s ‖ -z1 a r with blind -z2
struct PolyevalFinal { sbn_host::fr::El a_hat, nz1, nz2, tail; };
static PolyevalFinal polyeval_verify_scalars(const uint8_t* r_right, size_t lg, const std::vector<sbn_host::fr::El>& u, const std::vector<sbn_host::fr::El>& ui,
                                             const uint8_t rq[32], const uint8_t cc[32], const uint8_t* z1b, const uint8_t* z2b, uint8_t* hs) {
  using namespace sbn_host::fr;
  const El one = from_u64(1), zero = from_u64(0);
  El a_hat = one;
  for (size_t k = 0; k < lg; k++) {
    const El rk = el_from(r_right + 32 * k);
    a_hat = fmul(a_hat, add(fmul(ui[k], sub(one, rk)), fmul(u[k], rk)));
  }
  const El ec = el_from(cc), er = el_from(rq), ac = fmul(a_hat, ec), z1 = el_from(z1b), z2 = el_from(z2b);
  for (size_t j = 0; j < lg; j++) {
    const El sl = fmul(ac, fmul(u[j], u[j])), sr = fmul(ac, fmul(ui[j], ui[j]));
    memcpy(hs + 32 * j, sl.v, 32); memcpy(hs + 32 * (lg + j), sr.v, 32);
  }
  memcpy(hs + 64 * lg, one.v, 32); memcpy(hs + 64 * lg + 32, a_hat.v, 32);               // delta, beta
  { const El sy = fmul(ac, er); memcpy(hs + 64 * lg + 64, ac.v, 32); memcpy(hs + 64 * lg + 96, sy.v, 32); }   // Cx, Cy
  PolyevalFinal f; f.a_hat = a_hat; f.nz1 = sub(zero, z1); f.nz2 = sub(zero, z2); f.tail = fmul(f.nz1, fmul(a_hat, er));
  return f;
}

// the check on the transcript `t` (a copy of the caller's); arguments already checked.  SBN_OK with *accepted = 0: the proof is refused
static int polyeval_verify_locked(sbn_ctx* c, const sbn_bases* gens, const sbn_bases* comm, const uint8_t* r, size_t ell, const uint8_t* C_Zr_xy, const uint8_t* Zr,
                                  const uint8_t* proof, sbn_host::MerlinTranscript& t, int* accepted) {
  using namespace sbn_host::fr;
  *accepted = 0;
  const size_t ml = ell / 2, mr = ell - ml, L_size = (size_t)1 << ml, n = (size_t)1 << mr, lg = mr;
  const size_t np = 2 * lg + 2;                                   // the proof's points: L, R, delta, beta; Cx and Cy follow them on the device
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
  void* slab = nullptr; size_t slab_bytes = 0;
  hipError_t e = pool_get(c, total, &slab, &slab_bytes);
  if (e != hipSuccess) return fail(c, SBN_ENOMEM, "hipMalloc polyeval verify state: %s", hipGetErrorString(e));
  struct Drop { sbn_ctx* c; void* p; size_t b; ~Drop() { hipStreamSynchronize(c->stream); pool_put(c, p, b); } } drop{c, slab, slab_bytes};
  uint8_t* p0 = (uint8_t*)slab;
  uint32_t* d_L = (uint32_t*)(p0 + o_L); uint32_t* d_Lc = (uint32_t*)(p0 + o_Lc); uint32_t* d_row = (uint32_t*)(p0 + o_row); uint32_t* d_stage = (uint32_t*)(p0 + o_stage);
  uint32_t* d_comp = (uint32_t*)(p0 + o_comp); uint32_t* d_pts = (uint32_t*)(p0 + o_pts); uint32_t* d_scal = (uint32_t*)(p0 + o_scal); uint8_t* d_ok = p0 + o_ok;
  uint8_t* pin = (uint8_t*)c->pin;

  // ---- first launch: the proof's points, eq(r_left), C_LZ, C_Zr ----
  uint8_t comp[44 * 32];                                          // np <= 42; the identity in the form sbn_g1_compress writes it
  for (size_t i = 0; i < np; i++) {
    memcpy(comp + 32 * i, proof + 32 * i, 32);
    if (comp[32 * i + 31] & 0x40) { memset(comp + 32 * i, 0, 32); comp[32 * i + 31] = 0x40; }
  }
  memcpy(pin, comp, 32 * np);
  HIPCHK(c, hipMemsetAsync(d_ok, 0, 64, c->stream));
  HIPCHK(c, hipMemcpyAsync(d_comp, pin, 32 * np, hipMemcpyHostToDevice, c->stream));
  LAUNCH(c, "k_g1_decompress", k_g1_decompress, (unsigned)((np + 63) / 64), 64, (const uint32_t*)d_comp, np, (uint32_t*)nullptr, d_pts, d_ok);
  {
    PolyEvalPoint pt; memset(&pt, 0, sizeof pt);
    for (size_t j = 0; j < ml; j++) { const El x = to_dev_mont(el_from(r + 32 * j)); memcpy(pt.l[j], x.v, 32); }
    for (size_t j = 0; j < mr; j++) { const El x = to_dev_mont(el_from(r + 32 * (ml + j))); memcpy(pt.r[j], x.v, 32); }
    LAUNCH(c, "k_polyeval_eq", k_polyeval_eq, (unsigned)((std::max(n, L_size) + 255) / 256), 256, pt, (int)ml, (int)mr, d_L, (uint32_t*)(p0 + o_R), (uint32_t*)(p0 + o_s));
    LAUNCH(c, "k_scalars_from_mont", k_scalars_from_internal, (unsigned)((L_size + 255) / 256), 256, (const uint32_t*)d_L, d_Lc, L_size);
  }
  MsmShape s1;
  if ((rc = msm_windows_launch(c, d_Lc, (const uint32_t*)comm->d_pts, L_size, comm, &s1))) return rc;
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
  sbn_host::to_affine_bytes(verify_fold_windows(S, s1), Cxy, nullptr);
  if (Zr) sbn_host::to_affine_bytes(sbn_host::pt_from_device(S[s1.W]), Cxy + 64, nullptr); else memcpy(Cxy + 64, C_Zr_xy, 64);

  // ---- the transcript, as the reference's verifier writes it ----
  uint8_t rq[32], cc[32];
  std::vector<El> u, ui;
  if (!polyeval_verify_script(ts, Cxy, Rv.data(), n, comp, lg, rq, cc, u, ui)) return SBN_OK;      // a challenge u = 0

  // ---- O(lg n) field work: b_hat in closed form, the scalars of the proof's points, the row's constants ----
  uint8_t* hs = pin + 4096;                                       // (np + 2) scalars, then Cx ‖ Cy
  const PolyevalFinal fin = polyeval_verify_scalars(r + 32 * ml, lg, u, ui, rq, cc, z1b, z2b, hs);
  memcpy(hs + 32 * (np + 2), Cxy, 128);
  const El nz1 = fin.nz1, nz2 = fin.nz2, tail = fin.tail;

  // ---- second launch: the folded equation ----
  HIPCHK(c, hipMemcpyAsync(d_scal, hs, 32 * (np + 2), hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemcpyAsync(d_pts + 16 * np, hs + 32 * (np + 2), 128, hipMemcpyHostToDevice, c->stream));
  LAUNCH(c, "k_points_to_mont", k_points_to_mont, 1, 256, (const uint32_t*)(d_pts + 16 * np), d_pts + 16 * np, (size_t)2);
  MsmShape s2;
  if ((rc = msm_windows_launch(c, d_scal, d_pts, np + 2, nullptr, &s2))) return rc;
  if (s2.W + 2 > VERIFY_STAGE_POINTS) return fail(c, SBN_EINVAL, "polyeval verify: %d windows", s2.W);
  HIPCHK(c, hipMemcpyAsync(d_stage, c->wsum.p, (size_t)s2.W * 128, hipMemcpyDeviceToDevice, c->stream));
  {
    PolyEvalPoint U; memset(&U, 0, sizeof U);
    for (size_t k = 0; k < lg; k++) { const El a = to_dev_mont(u[k]), b = to_dev_mont(ui[k]); memcpy(U.l[k], a.v, 32); memcpy(U.r[k], b.v, 32); }
    LAUNCH(c, "k_polyeval_verify_row", k_polyeval_verify_row, (unsigned)((n + 255) / 256), 256, U, (int)lg, scs_from(to_dev_mont(nz1)), scs_from(tail), scs_from(nz2), d_row, d_row + 8 * (n + 1));
    RowInfo ri; ri.internal_rows = true;
    if ((rc = commit_rows_launch(c, ext, d_row, d_row + 8 * (n + 1), 1, n + 1, nullptr, nullptr, ri))) return rc;
    HIPCHK(c, hipMemcpyAsync(d_stage + 32 * (size_t)s2.W, c->wsum.p, 128, hipMemcpyDeviceToDevice, c->stream));
  }
  if ((rc = verify_handover(c, d_stage, (size_t)s2.W + 1, nullptr, 0, S, nullptr))) return rc;
  const sbn_host::Pt sum = sbn_host::padd(verify_fold_windows(S, s2), sbn_host::pt_from_device(S[s2.W]));
  *accepted = sbn_host::is_inf(sum) ? 1 : 0;
  return SBN_OK;
}

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

// sbn_bases_from_compressed with the context's mutex held: a handle over n decompressed points.  A point that does not decompress is SBN_EINVAL
// with its index in *bad_index (which the caller set to SIZE_MAX to tell it from other misuse)
static int bases_from_compressed_locked(sbn_ctx* c, const uint8_t* in32, size_t n, sbn_bases** out, size_t* bad_index) {
  int rc;
  const size_t o_xy = 32 * n, o_ok = o_xy + 64 * n;
  if ((rc = ensure(c, c->stage_pts, o_ok + n + 64))) return rc;
  uint8_t* p = (uint8_t*)c->stage_pts.p;
  sbn_bases* b = new sbn_bases(); b->n = n; b->has_h = false;
  hipError_t e = hipMalloc(&b->d_pts, (n ? n : 1) * 64);
  if (e != hipSuccess) { delete b; return fail(c, SBN_ENOMEM, "hipMalloc bases: %s", hipGetErrorString(e)); }
  std::vector<uint8_t> xy(64 * n), ok(n);
  auto run = [&]() -> int {
    if (!n) return SBN_OK;
    HIPCHK(c, hipMemcpyAsync(p, in32, 32 * n, hipMemcpyHostToDevice, c->stream));
    LAUNCH(c, "k_g1_decompress", k_g1_decompress, (unsigned)((n + 63) / 64), 64, (const uint32_t*)p, n, (uint32_t*)(p + o_xy), (uint32_t*)b->d_pts, p + o_ok);
    LAUNCHCHK(c);
    HIPCHK(c, hipMemcpyAsync(xy.data(), p + o_xy, 64 * n, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(ok.data(), p + o_ok, n, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (c->prof) prof_drain(c);
    return SBN_OK;
  };
  if ((rc = run())) { hipStreamSynchronize(c->stream); sbn_bases_free(c, b); return rc; }
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

extern "C" {

int sbn_g1_decompress(sbn_ctx* c, const uint8_t* in32, size_t n, uint8_t* out_xy, uint8_t* out_ok) {
  if (!c || ((!in32 || !out_xy || !out_ok) && n)) return SBN_EINVAL;
  if (n == 0) return SBN_OK;
  std::lock_guard<std::mutex> g(c->mu); hipSetDevice(c->device);
  int rc;
  const size_t o_xy = 32 * n, o_ok = o_xy + 64 * n;
  if ((rc = ensure(c, c->stage_pts, o_ok + n))) return rc;
  uint8_t* p = (uint8_t*)c->stage_pts.p;
  HIPCHK(c, hipMemcpyAsync(p, in32, 32 * n, hipMemcpyHostToDevice, c->stream));
  LAUNCH(c, "k_g1_decompress", k_g1_decompress, (unsigned)((n + 63) / 64), 64, (const uint32_t*)p, n, (uint32_t*)(p + o_xy), (uint32_t*)nullptr, p + o_ok);
  LAUNCHCHK(c);
  HIPCHK(c, hipMemcpyAsync(out_xy, p + o_xy, 64 * n, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipMemcpyAsync(out_ok, p + o_ok, n, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  if (c->prof) prof_drain(c);
  return SBN_OK;
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
