// abi_polyeval.inc — C ABI: the Hyrax opening in ONE call.  sbn_polyeval_prove is PolyEvalProof::prove (hyrax.rs:65-116) with
// DotProductProofLog::prove (nizk/mod.rs:439-522) and BulletReductionProof::prove (nizk/bullet.rs:24-126) inside; sbn_joint_opening_prove
// puts the n-to-1 reduction of the HashLayerProof openings (sparse_mlpoly_full.rs:384-407, :986-1009, :1013-1035) in front of it.
//
// gens_n and gens_1 share h (commitments.rs:78-99), so EVERY group element of the proof is a commitment over the one fixed set
// G ‖ Q_base with h — the caller's generator handle itself, copied once per handle with its lookup table (the set of abi_bullet.inc):
//   Cx = [L*Z ‖ 0], blind <blinds, L>          Cy = [0 ... 0 ‖ Zr], blind blind_Zr           (one two-row commit)
//   L_j, R_j = the two rows of a bullet round                                                  (lg n two-row commits, bullet_round_locked)
//   delta = d * MSM(s, G) + r_delta * h = [d * s_t ‖ 0], blind r_delta     beta = d * (r * Q_base) + r_beta * h = [0 ... 0 ‖ d * r], blind r_beta
// lg n + 2 two-row commits on the lookup path, one host wait each; g_hat and Gamma (which the caller drops, nizk/mod.rs:484) are never formed
// and no scalar multiplication runs on the CPU.  Between the waits the host compresses the points, runs the Merlin transcript, inverts u and
// folds the blind (bullet.rs:104).  The transcript stays on the host: a_vec = R goes in as n separate 32-byte messages (transcript.rs:46-50,
// ~2 200 Keccak permutations at n = 8192), strictly sequential and BEHIND Cx and Cy in the byte stream, so what hides behind the first commit
// is the host's own computation of R, not the absorption (DESIGN.md 4.11).
// polyeval_host_eq, joint_reduce and OpeningShape are verify_host.hpp (the verifiers run them too); opening_point is abi_verify_common.inc.
// Included by sbn254.hip; needs abi_proof_common.inc, abi_verify_common.inc and abi_bullet.inc.

// the copy of the caller's R_size + 1 generators (+ h) that the commits run over, with its lookup table: built on the first opening, owned by `gens`
static int polyeval_ext(sbn_ctx* c, const sbn_bases* gens, const sbn_bases** out) {
  return derived_set(gens, DERIVED_POLYEVAL, std::string(), [&](sbn_bases** ext) -> int {
    const int rc = bases_from_device(c, gens->d_pts, gens->n, (const uint8_t*)gens->d_pts + 64 * gens->n, ext);
    if (rc != SBN_OK) return rc;
    if (bases_build_comb(c, (*ext)->uniq ? (*ext)->uniq : *ext, BULLET_COMB_BYTES) != SBN_OK) (void)hipGetLastError();     // best effort, as in bullet_begin_impl
    return SBN_OK;
  }, out);
}

static int polyeval_check(sbn_ctx* c, const sbn_bases* gens, const sbn_table* Z, const uint8_t* blinds, const uint8_t* r, size_t ell, const uint8_t* Zr,
                          const uint8_t* blind_Zr, const uint8_t* rnd) {
  if (ell == 0 || ell > 2 * (size_t)PE_SIDE_MAX) return fail(c, SBN_EINVAL, "polyeval: ell = %zu is outside 1 .. %d", ell, 2 * PE_SIDE_MAX);
  const OpeningShape sh = opening_shape(ell);
  const size_t mr = sh.mr, L_size = sh.L_size, n = sh.n;
  if (Z->len != ((size_t)1 << ell)) return fail(c, SBN_EINVAL, "polyeval: the table has %zu entries, r has %zu variables  [hyrax.rs:77 assert_eq]", Z->len, ell);
  if (gens->n != n + 1 || !gens->has_h) return fail(c, SBN_EINVAL, "polyeval: the generator set has %zu points%s, the opening needs %zu + 1 with h  [nizk/mod.rs:412-415, :455]", gens->n, gens->has_h ? "" : " and no h", n);
  for (size_t j = 0; j < ell; j++) if (!fr_canonical(r + 32 * j)) return fail(c, SBN_EINVAL, "polyeval: r[%zu] is not canonical", j);
  if (!fr_canonical(Zr) || (blind_Zr && !fr_canonical(blind_Zr))) return fail(c, SBN_EINVAL, "polyeval: Zr / blind_Zr is not canonical");
  if (blinds) for (size_t i = 0; i < L_size; i++) if (!fr_canonical(blinds + 32 * i)) return fail(c, SBN_EINVAL, "polyeval: blinds[%zu] is not canonical", i);
  for (size_t i = 0; i < 3 + 2 * mr; i++) if (!fr_canonical(rnd + 32 * i)) return fail(c, SBN_EINVAL, "polyeval: rnd[%zu] is not canonical", i);
  return SBN_OK;
}

// the opening on the transcript `t` (a copy of the caller's: the caller's moves on only when this returns SBN_OK); arguments already checked
static int polyeval_prove_locked(sbn_ctx* c, const sbn_bases* gens, const sbn_table* Z, const uint8_t* blinds, const uint8_t* r, size_t ell, const uint8_t* Zr,
                                 const uint8_t* blind_Zr, const uint8_t* rnd, sbn_host::MerlinTranscript& t, uint8_t* out_proof,
                                 uint8_t out_Cx_xy[64], int* Cx_is_inf, uint8_t out_Cy_xy[64], int* Cy_is_inf) {
  using namespace sbn_host::fr;
  typedef std::chrono::steady_clock clk;
  const OpeningShape sh = opening_shape(ell);
  const size_t ml = sh.ml, mr = sh.mr, L_size = sh.L_size, n = sh.n, lg = sh.lg;
  sbn_host::Script ts{t};
  int rc;
  sbn_bullet st; st.n = st.m = n; st.has_q = true; st.has_h = true; st.q_scaled = true; memset(&st.qs, 0, sizeof st.qs);
  if ((rc = polyeval_ext(c, gens, &st.ext))) return rc;
  if ((rc = ensure_pin(c, 4096 + (blinds ? L_size * 32 : 0)))) return rc;
  // the row slices of L*Z, as sbn_table_bound cuts them (~2048 blocks in flight)
  const size_t col_tiles = (n + 63) / 64;
  size_t nslices = (2048 + col_tiles - 1) / col_tiles; if (nslices > L_size) nslices = L_size; if (nslices < 1) nslices = 1;
  const size_t rows_per_slice = (L_size + nslices - 1) / nslices; nslices = (L_size + rows_per_slice - 1) / rows_per_slice;
  if (col_tiles > 0x7fffffff || nslices > 65535) return fail(c, SBN_EINVAL, "polyeval: bound grid too large");
  if ((rc = ensure(c, c->sc_partial, std::max<size_t>(4096, nslices * n * 32)))) return rc;
  SlabLease slab(c);
  if ((rc = slab.get((5 * n + 2 * (n + 2) + 2) * 32, "polyeval state"))) return rc;     // the bullet state's layout (bullet_begin_impl)
  st.slab = slab.p; st.slab_bytes = slab.bytes;
  uint8_t* p0 = (uint8_t*)st.slab; st.d_a = p0; st.d_b = p0 + 32 * n; st.d_s = p0 + 64 * n; st.d_a2 = p0 + 96 * n; st.d_b2 = p0 + 128 * n;
  st.d_w = p0 + 160 * n; st.d_dots = p0 + 160 * n + 64 * (n + 2);
  uint32_t* W0 = (uint32_t*)st.d_w; uint32_t* W1 = W0 + 8 * (n + 1); uint32_t* BL = W1 + 8 * (n + 1);
  uint32_t* d_L = (uint32_t*)st.d_a2; uint32_t* d_blinds = (uint32_t*)st.d_b2;       // free until the first fold writes the ping-pong halves

  ts.protocol("polynomial evaluation proof");                     // hyrax.rs:75
  ts.protocol("dot product proof (log)");                         // nizk/mod.rs:451
  const uint8_t* d = rnd; const uint8_t* r_delta = rnd + 32; const uint8_t* r_beta = rnd + 64; const uint8_t* blinds_vec = rnd + 96;

  // ---- front: L, R, L*Z, <blinds, L>, the Cx / Cy rows; one two-row commit ----
  {
    const PolyEvalPoint pt = opening_point(sh, r);
    if (blinds) {
      memcpy((uint8_t*)c->pin + 4096, blinds, L_size * 32);
      HIPCHK(c, hipMemcpyAsync(d_blinds, (uint8_t*)c->pin + 4096, L_size * 32, hipMemcpyHostToDevice, c->stream));
    }
    LAUNCH(c, "k_polyeval_eq", k_polyeval_eq, (unsigned)((n + 255) / 256), 256, pt, (int)ml, (int)mr, d_L, (uint32_t*)st.d_b, (uint32_t*)st.d_s);
    LAUNCH(c, "k_bound_partial", k_bound_partial, dim3((unsigned)col_tiles, (unsigned)nslices), 256, (const uint32_t*)Z->d, (const uint32_t*)d_L, L_size, n, rows_per_slice, (uint32_t*)c->sc_partial.p);
    PolyEvalFront A;
    A.partial = (const uint32_t*)c->sc_partial.p; A.Lv = d_L; A.blinds = blinds ? d_blinds : nullptr; A.a = (uint32_t*)st.d_a; A.w0 = W0; A.w1 = W1; A.bl = BL; A.dots = (uint32_t*)st.d_dots;
    ScScalar sz, sbz; memcpy(sz.v, Zr, 32); memset(&sbz, 0, sizeof sbz); if (blind_Zr) memcpy(sbz.v, blind_Zr, 32);
    LAUNCH(c, "k_polyeval_front", k_polyeval_front, (unsigned)((n + 255) / 256 + 1), 256, A, nslices, n, L_size, sz, sbz);
    LAUNCHCHK(c);
  }
  uint32_t seq = 0;
  if ((rc = bullet_rows_launch(c, &st, &seq))) return rc;
  // beside the device's front: a_vec = R on the host (the transcript needs its canonical bytes; n products)
  const clk::time_point h0 = clk::now();
  std::vector<uint8_t> Rv;
  polyeval_host_eq(r + 32 * ml, mr, Rv);
  const clk::time_point h1 = clk::now();
  uint8_t bx[32], zero32[32];
  if ((rc = bullet_rows_collect(c, seq, out_Cx_xy, Cx_is_inf, out_Cy_xy, Cy_is_inf, bx, zero32))) return rc;
  const clk::time_point h2 = clk::now();
  uint8_t comp[32];
  ts.point_xy("Cx", out_Cx_xy, comp);                             // nizk/mod.rs:470-474
  ts.point_xy("Cy", out_Cy_xy, comp);
  ts.scalars("a", Rv.data(), n);                                  // nizk/mod.rs:476
  const clk::time_point h3 = clk::now();
  c->polyeval_us[0] = std::chrono::duration<double, std::micro>(h1 - h0).count();
  c->polyeval_us[1] = std::chrono::duration<double, std::micro>(h2 - h1).count();
  c->polyeval_us[2] = std::chrono::duration<double, std::micro>(h3 - h2).count();
  uint8_t rq[32];
  ts.challenge("r", rq);                                          // nizk/mod.rs:480: Q = r * Q_base
  st.qs = scs_from(to_dev_mont(el_from(rq)));
  El blind_G = el_from(bx);                                       // blind_Gamma = blind_x + r * blind_y (nizk/mod.rs:483)
  if (blind_Zr) blind_G = add(blind_G, fmul(el_from(rq), el_from(blind_Zr)));

  // ---- the rounds (bullet.rs:63-108): one launch + one two-row commit + one wait each ----
  uint8_t u[32] = {0}, ui[32] = {0};
  for (size_t j = 0; j < lg; j++) {
    const uint8_t* bL = blinds_vec + 64 * j; const uint8_t* bR = bL + 32;
    uint8_t Lxy[64], Rxy[64], cl[32], cr[32]; int li = 0, ri = 0;
    if ((rc = bullet_round_locked(c, &st, j > 0, u, ui, bL, bR, Lxy, &li, Rxy, &ri, cl, cr))) return rc;
    ts.point_xy("L", Lxy, out_proof + 32 * j);
    ts.point_xy("R", Rxy, out_proof + 32 * (lg + j));
    ts.challenge("u", u);
    const El eu = el_from(u);
    if (is_zero(eu)) return fail(c, SBN_EINVAL, "polyeval: the challenge u of round %zu is zero  [bullet.rs:82 unwrap]", j);
    const El eui = inv(eu);
    memcpy(ui, eui.v, 32);
    blind_G = add(add(fmul(fmul(eu, eu), el_from(bL)), blind_G), fmul(fmul(eui, eui), el_from(bR)));     // bullet.rs:104
  }

  // ---- close: the last fold, the delta / beta rows; one two-row commit ----
  {
    const ScScalar su = scs_from(to_dev_mont(el_from(u))), si = scs_from(to_dev_mont(el_from(ui))), sd = scs_from(to_dev_mont(el_from(d)));
    const ScScalar sdr = scs_from(fmul(el_from(d), el_from(rq)));
    ScScalar s1, s2; memcpy(s1.v, r_delta, 32); memcpy(s2.v, r_beta, 32);
    LAUNCH(c, "k_polyeval_close", k_polyeval_close, (unsigned)((n + 255) / 256), 256, (const uint32_t*)st.d_a, (const uint32_t*)st.d_b, (const uint32_t*)st.d_s,
           W0, W1, BL, (uint32_t*)st.d_dots, n, su, si, sd, sdr, s1, s2);
    LAUNCHCHK(c);
  }
  if ((rc = bullet_rows_launch(c, &st, &seq))) return rc;
  uint8_t dxy[64], bxy[64], ah[32], bh[32]; int di = 0, bi = 0;
  if ((rc = bullet_rows_collect(c, seq, dxy, &di, bxy, &bi, ah, bh))) return rc;
  ts.point_xy("delta", dxy, out_proof + 64 * lg);     // nizk/mod.rs:501-504
  ts.point_xy("beta", bxy, out_proof + 64 * lg + 32);
  uint8_t cc[32];
  ts.challenge("c", cc);
  // x_hat = a_hat of the reduction (the fold of x_vec = L*Z), a_hat = its b_hat (the fold of a_vec = R)   (nizk/mod.rs:484, :495, :508-509)
  const El ec = el_from(cc), x_hat = el_from(ah), a_hat = el_from(bh);
  const El z1 = add(el_from(d), fmul(ec, fmul(x_hat, a_hat)));
  const El z2 = add(fmul(a_hat, add(fmul(ec, blind_G), el_from(r_beta))), el_from(r_delta));
  memcpy(out_proof + 64 * lg + 64, z1.v, 32); memcpy(out_proof + 64 * lg + 96, z2.v, 32);
  return SBN_OK;
}

extern "C" {

int sbn_polyeval_prove(sbn_ctx* c, const sbn_bases* gens, const sbn_table* Z, const uint8_t* blinds, const uint8_t* r, size_t ell, const uint8_t Zr[32],
                       const uint8_t* blind_Zr, const uint8_t* rnd, sbn_transcript* tr, uint8_t* out_proof,
                       uint8_t out_Cx_xy[64], int* Cx_is_inf, uint8_t out_Cy_xy[64], int* Cy_is_inf) {
  if (!c || !gens || !Z || !r || !Zr || !rnd || !tr || !out_proof || !out_Cx_xy || !out_Cy_xy) return SBN_EINVAL;
  int rc;
  if ((rc = polyeval_check(c, gens, Z, blinds, r, ell, Zr, blind_Zr, rnd))) return rc;
  std::lock_guard<std::mutex> g(c->mu); hipSetDevice(c->device);
  return prove_on_copy(c, tr, [&](sbn_host::MerlinTranscript& t) {
    return polyeval_prove_locked(c, gens, Z, blinds, r, ell, Zr, blind_Zr, rnd, t, out_proof, out_Cx_xy, Cx_is_inf, out_Cy_xy, Cy_is_inf);
  });
}

}  // extern "C"
// the reduction and the opening on the transcript `t` (a copy of the caller's); count = 2^lc evals, canonical as r is; the caller holds the
// context's mutex.  out_challenges: lc x 32 or NULL
static int joint_opening_locked(sbn_ctx* c, const sbn_bases* gens, const sbn_table* Z, const uint8_t* evals, size_t count, size_t lc,
                                sbn_host::Label label_evals, sbn_host::Label label_chal, sbn_host::Label label_claim,
                                const uint8_t* r, size_t ell_r, const uint8_t* rnd, sbn_host::MerlinTranscript& t,
                                uint8_t* out_challenges, uint8_t out_joint_claim[32], uint8_t* out_proof,
                                uint8_t out_Cx_xy[64], int* Cx_is_inf, uint8_t out_Cy_xy[64], int* Cy_is_inf) {
  const size_t ell = lc + ell_r;
  std::vector<uint8_t> rj; uint8_t claim[32];
  joint_reduce(evals, count, lc, label_evals, label_chal, label_claim, r, ell_r, t, rj, claim);
  int rc;
  if ((rc = polyeval_check(c, gens, Z, nullptr, rj.data(), ell, claim, nullptr, rnd))) return rc;
  if ((rc = polyeval_prove_locked(c, gens, Z, nullptr, rj.data(), ell, claim, nullptr, rnd, t, out_proof, out_Cx_xy, Cx_is_inf, out_Cy_xy, Cy_is_inf))) return rc;
  if (lc && out_challenges) memcpy(out_challenges, rj.data(), 32 * lc);
  memcpy(out_joint_claim, claim, 32);
  return SBN_OK;
}

extern "C" {

int sbn_joint_opening_prove(sbn_ctx* c, const sbn_bases* gens, const sbn_table* Z, const uint8_t* evals, size_t count,
                            const uint8_t* label_evals, size_t label_evals_len, const uint8_t* label_chal, size_t label_chal_len,
                            const uint8_t* label_claim, size_t label_claim_len, const uint8_t* r, size_t ell_r, const uint8_t* rnd, sbn_transcript* tr,
                            uint8_t* out_challenges, uint8_t out_joint_claim[32], uint8_t* out_proof,
                            uint8_t out_Cx_xy[64], int* Cx_is_inf, uint8_t out_Cy_xy[64], int* Cy_is_inf) {
  if (!c || !gens || !Z || !evals || !label_evals || !label_chal || !label_claim || (!r && ell_r) || !rnd || !tr || !out_joint_claim || !out_proof || !out_Cx_xy || !out_Cy_xy) return SBN_EINVAL;
  if (count == 0 || (count & (count - 1)) || count > ((size_t)1 << 20)) return fail(c, SBN_EINVAL, "joint opening: %zu evals (a power of two is needed: the caller pads)", count);
  size_t lc = 0; while (((size_t)1 << lc) < count) lc++;
  if (lc && !out_challenges) return SBN_EINVAL;
  for (size_t i = 0; i < count; i++) if (!fr_canonical(evals + 32 * i)) return fail(c, SBN_EINVAL, "joint opening: evals[%zu] is not canonical", i);
  const size_t ell = lc + ell_r;
  if (ell > 2 * (size_t)PE_SIDE_MAX) return fail(c, SBN_EINVAL, "joint opening: %zu variables", ell);
  for (size_t j = 0; j < ell_r; j++) if (!fr_canonical(r + 32 * j)) return fail(c, SBN_EINVAL, "joint opening: r[%zu] is not canonical", j);
  std::lock_guard<std::mutex> g(c->mu); hipSetDevice(c->device);
  using sbn_host::Label;
  return prove_on_copy(c, tr, [&](sbn_host::MerlinTranscript& t) {
    return joint_opening_locked(c, gens, Z, evals, count, lc, Label(label_evals, label_evals_len), Label(label_chal, label_chal_len), Label(label_claim, label_claim_len),
                                r, ell_r, rnd, t, out_challenges, out_joint_claim, out_proof, out_Cx_xy, Cx_is_inf, out_Cy_xy, Cy_is_inf);
  });
}

// host microseconds of the context's most recent opening: {R = a_vec computed on the host, the wait for the Cx / Cy commit behind it,
// Cx, Cy and the n a_vec messages absorbed into the transcript}
int sbn_prof_last_polyeval(sbn_ctx* c, double out_us[3]) {
  if (!c || !out_us) return SBN_EINVAL;
  std::lock_guard<std::mutex> g(c->mu);
  for (int i = 0; i < 3; i++) out_us[i] = c->polyeval_us[i];
  return SBN_OK;
}

}  // extern "C"
