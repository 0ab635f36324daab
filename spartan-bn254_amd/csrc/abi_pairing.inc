// abi_pairing.inc — C ABI: pairings and KZG verification (pairing_host.hpp, pairing_kernels.cuh).
//   sbn_g2_prepare / sbn_g2_lines_free    a fixed G2 point (srs.g2, srs.tau_g2): parsed, checked and its 88 lines tabulated on the host, once per SRS
//   sbn_pairing_products                  nchecks independent products of at most four pairings in ONE launch, one wave a check
//   sbn_kzg_verify / _batched             KZGProof::verify (kzg.rs:196-217) / KZGBatchProof::batch_verify (:315-352) as
//                                             e(C - y G + z pi, g2) * e(-pi, tau_g2) == 1
//                                         which holds by bilinearity alone: no G2 point is multiplied, both are fixed per SRS.  The G1 sum is one
//                                         sbn_g1_small_sums call (k_window_sums and the host fold), the product one k_pairing_products launch.
// The byte-level point and scalar helpers (g1_xy_valid, g1_neg_bytes, fr_neg_bytes, fq_to_dev_mont) are verify_host.hpp.
// Included by sbn254.hip; needs abi_small_sums.inc (sbn_g1_small_sums).

static const size_t PAIR_CHECKS_MAX = (size_t)1 << 16;      // a grid of 2^16 waves, 19 MiB of descriptors and 24 MiB of GT bytes: sizes stay far from any overflow

struct sbn_g2_lines {
  sbn_ctx* ctx = nullptr;
  void* d = nullptr;             // nlines x 128 B of line values, then nlines x u32 square_first
  size_t nlines = 0, bytes = 0;
};

// the shared end of the two KZG checks: L = sum_k s_k P_k (the caller's terms, then -y G and z pi are appended here), then the product
static int kzg_check_run(sbn_ctx* c, const sbn_g2_lines* g2, const sbn_g2_lines* tau_g2, std::vector<uint8_t>& pts, std::vector<uint8_t>& scal,
                         const uint8_t y[32], const uint8_t z[32], const uint8_t proof_xy[64], int* accepted) {
  static const uint8_t G1_GEN[64] = {1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 2};
  uint8_t ny[32]; fr_neg_bytes(y, ny);
  pts.insert(pts.end(), G1_GEN, G1_GEN + 64); scal.insert(scal.end(), ny, ny + 32);
  pts.insert(pts.end(), proof_xy, proof_xy + 64); scal.insert(scal.end(), z, z + 32);
  const uint32_t nterms = (uint32_t)(scal.size() / 32);
  uint8_t pair_p[128], is_inf = 0;
  int rc;
  if ((rc = sbn_g1_small_sums(c, pts.data(), scal.data(), &nterms, 1, pair_p, &is_inf))) return rc;
  g1_neg_bytes(proof_xy, pair_p + 64);
  const sbn_g2_lines* qs[2] = {g2, tau_g2};
  const uint32_t two = 2;
  uint8_t is_one = 0;
  if ((rc = sbn_pairing_products(c, pair_p, qs, &two, 1, &is_one, nullptr))) return rc;
  *accepted = is_one ? 1 : 0;
  return SBN_OK;
}

extern "C" {

int sbn_g2_prepare(sbn_ctx* c, const uint8_t q_xy[128], uint32_t flags, sbn_g2_lines** out) {
  namespace pr = sbn_host::pairing;
  if (!c) return SBN_EINVAL;
  if (!q_xy || !out) return fail(c, SBN_EINVAL, "g2 prepare: a null pointer");
  if (flags & ~SBN_POINTS_MONT) return fail(c, SBN_EINVAL, "g2 prepare: unknown flags 0x%x", flags);
  pr::G2 q;
  static const char* const why[] = {"", "a coordinate is not canonical (>= q)", "the identity has no line table", "the point is not on the twist E'",
                                    "the point is on E' but outside the r-torsion (the cofactor of E'(Fq2) is 2q - r)"};
  const pr::ParseResult r = pr::g2_parse_checked(q_xy, (flags & SBN_POINTS_MONT) != 0, &q);
  if (r != pr::G2_OK) return fail(c, SBN_EINVAL, "g2 prepare: %s", why[(int)r]);
  std::vector<pr::Line> t;
  if (!pr::line_table(q, &t)) return fail(c, SBN_EINVAL, "g2 prepare: a vertical line in the Miller loop");
  std::vector<uint8_t> img(t.size() * (pr::LINE_BYTES + 4));
  pr::lines_to_device(t, img.data(), (uint32_t*)(img.data() + t.size() * pr::LINE_BYTES));
  std::lock_guard<std::mutex> g(c->mu); hipSetDevice(c->device);
  sbn_g2_lines* l = new sbn_g2_lines();
  l->ctx = c; l->nlines = t.size();
  const hipError_t e = pool_get(c, img.size(), &l->d, &l->bytes);
  if (e != hipSuccess) { delete l; return fail(c, SBN_ENOMEM, "hipMalloc g2 lines: %s", hipGetErrorString(e)); }
  const hipError_t e2 = hipMemcpy(l->d, img.data(), img.size(), hipMemcpyHostToDevice);
  if (e2 != hipSuccess) { pool_put(c, l->d, l->bytes); delete l; return fail(c, SBN_EHIP, "g2 prepare: upload failed: %s", hipGetErrorString(e2)); }
  *out = l;
  return SBN_OK;
}

void sbn_g2_lines_free(sbn_ctx* c, sbn_g2_lines* l) {
  if (!l) return;
  (void)c;
  sbn_ctx* own = l->ctx;                            // the buffer came from its own context's pool and goes back there, whatever the caller passes
  { std::lock_guard<std::mutex> g(own->mu); hipSetDevice(own->device); hipStreamSynchronize(own->stream); pool_put(own, l->d, l->bytes); }
  delete l;
}

int sbn_pairing_products(sbn_ctx* c, const uint8_t* p_xy, const sbn_g2_lines* const* q, const uint32_t* counts, size_t nchecks,
                         uint8_t* out_is_one, uint8_t* out_gt) {
  if (!c) return SBN_EINVAL;
  if (nchecks == 0) return SBN_OK;
  if (!counts || !out_is_one) return fail(c, SBN_EINVAL, "pairing products: a null pointer with %zu checks", nchecks);
  if (nchecks > PAIR_CHECKS_MAX) return fail(c, SBN_EINVAL, "pairing products: %zu checks in one call (at most %zu)", nchecks, PAIR_CHECKS_MAX);
  size_t total = 0;
  for (size_t i = 0; i < nchecks; i++) {
    if (counts[i] > (uint32_t)PAIR_TERMS_MAX) return fail(c, SBN_EINVAL, "pairing products: check %zu has %u terms (at most %d)", i, counts[i], PAIR_TERMS_MAX);
    total += counts[i];
  }
  if (total && (!p_xy || !q)) return fail(c, SBN_EINVAL, "pairing products: a null pointer with %zu terms", total);
  for (size_t j = 0; j < total; j++) {
    if (!q[j]) return fail(c, SBN_EINVAL, "pairing products: term %zu has no G2 handle", j);
    if (q[j]->ctx != c) return fail(c, SBN_EINVAL, "pairing products: the G2 handle of term %zu belongs to another context", j);
    if (!g1_xy_valid(p_xy + 64 * j)) return fail(c, SBN_EINVAL, "pairing products: point %zu is not a canonical point of the curve", j);
  }
  // descriptors built outside the context's mutex; a term whose P is the identity contributes 1 and is dropped here
  std::vector<PairCheck> stage(nchecks);
  const sbn_g2_lines* any = nullptr;
  size_t at = 0;
  for (size_t i = 0; i < nchecks; i++) {
    PairCheck& ck = stage[i];
    memset(&ck, 0, sizeof ck);
    for (uint32_t t = 0; t < counts[i]; t++, at++) {
      if (g1_is_identity(p_xy + 64 * at)) continue;
      const sbn_host::Fq x = fq_to_dev_mont(p_xy + 64 * at), y = fq_to_dev_mont(p_xy + 64 * at + 32);
      memcpy(ck.p[ck.count], x.v, 32); memcpy(ck.p[ck.count] + 8, y.v, 32);
      ck.lines[ck.count++] = (const uint8_t*)q[at]->d;
      any = q[at];
    }
  }
  const size_t desc_bytes = sizeof(PairCheck) * nchecks, o_one = (desc_bytes + 255) / 256 * 256, o_gt = o_one + (nchecks + 255) / 256 * 256;
  const size_t bytes = o_gt + (out_gt ? 384 * nchecks : 0), back = bytes - o_one;
  std::lock_guard<std::mutex> g(c->mu); hipSetDevice(c->device);
  int rc;
  if ((rc = ensure_pin(c, bytes))) return rc;
  memcpy(c->pin, stage.data(), desc_bytes);
  SlabLease slab(c);
  if ((rc = slab.get(bytes, "pairing products"))) return rc;
  uint8_t* p0 = (uint8_t*)slab.p;
  HIPCHK(c, hipMemcpyAsync(p0, c->pin, desc_bytes, hipMemcpyHostToDevice, c->stream));
  LAUNCH(c, "k_pairing_products", k_pairing_products, (unsigned)nchecks, 64, (const PairCheck*)p0,
         any ? (const uint32_t*)((const uint8_t*)any->d + any->nlines * PAIR_LINE_BYTES) : (const uint32_t*)nullptr, (uint32_t)(any ? any->nlines : 0),
         p0 + o_one, out_gt ? p0 + o_gt : (uint8_t*)nullptr);
  LAUNCHCHK(c);
  HIPCHK(c, hipMemcpyAsync((uint8_t*)c->pin + o_one, p0 + o_one, back, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  if (c->prof) prof_drain(c);
  memcpy(out_is_one, (uint8_t*)c->pin + o_one, nchecks);
  if (out_gt) memcpy(out_gt, (uint8_t*)c->pin + o_gt, 384 * nchecks);
  return SBN_OK;
}

int sbn_kzg_verify(sbn_ctx* c, const sbn_g2_lines* g2, const sbn_g2_lines* tau_g2, const uint8_t comm_xy[64], const uint8_t z[32],
                   const uint8_t eval[32], const uint8_t proof_xy[64], int* accepted) {
  if (!c) return SBN_EINVAL;
  if (!g2 || !tau_g2 || !comm_xy || !z || !eval || !proof_xy || !accepted) return fail(c, SBN_EINVAL, "kzg verify: a null pointer");
  if (g2->ctx != c || tau_g2->ctx != c) return fail(c, SBN_EINVAL, "kzg verify: a G2 handle of another context");
  if (!fr_canonical(z) || !fr_canonical(eval)) return fail(c, SBN_EINVAL, "kzg verify: z or eval is not canonical  [scalar.rs:87-95]");
  if (!g1_xy_valid(comm_xy)) return fail(c, SBN_EINVAL, "kzg verify: the commitment is not a canonical point of the curve");
  if (!g1_xy_valid(proof_xy)) { *accepted = 0; return SBN_OK; }              // the prover's point: a refusal, not misuse
  static const uint8_t ONE[32] = {1};
  std::vector<uint8_t> pts(comm_xy, comm_xy + 64), scal(ONE, ONE + 32);
  return kzg_check_run(c, g2, tau_g2, pts, scal, eval, z, proof_xy, accepted);
}

int sbn_kzg_verify_batched(sbn_ctx* c, const sbn_g2_lines* g2, const sbn_g2_lines* tau_g2, const uint8_t* comms_xy, size_t count,
                           const uint8_t z[32], const uint8_t gamma[32], const uint8_t* evals, const uint8_t proof_xy[64], int* accepted) {
  namespace fr = sbn_host::fr;
  if (!c) return SBN_EINVAL;
  if (!g2 || !tau_g2 || !z || !gamma || !proof_xy || !accepted || (count && (!comms_xy || !evals))) return fail(c, SBN_EINVAL, "kzg verify batched: a null pointer");
  if (count > (size_t)SS_TERMS_MAX - 2) return fail(c, SBN_EINVAL, "kzg verify batched: %zu commitments (at most %d)", count, SS_TERMS_MAX - 2);
  if (g2->ctx != c || tau_g2->ctx != c) return fail(c, SBN_EINVAL, "kzg verify batched: a G2 handle of another context");
  if (!fr_canonical(z) || !fr_canonical(gamma)) return fail(c, SBN_EINVAL, "kzg verify batched: z or gamma is not canonical  [scalar.rs:87-95]");
  for (size_t k = 0; k < count; k++) {
    if (!fr_canonical(evals + 32 * k)) return fail(c, SBN_EINVAL, "kzg verify batched: eval %zu is not canonical  [scalar.rs:87-95]", k);
    if (!g1_xy_valid(comms_xy + 64 * k)) return fail(c, SBN_EINVAL, "kzg verify batched: commitment %zu is not a canonical point of the curve", k);
  }
  if (!g1_xy_valid(proof_xy)) { *accepted = 0; return SBN_OK; }
  // sum_k gamma^k C_k and sum_k gamma^k eval_k (kzg.rs:327-341)
  fr::El gm, pw = fr::from_u64(1), y = fr::from_u64(0);
  memcpy(gm.v, gamma, 32);
  std::vector<uint8_t> pts(comms_xy, comms_xy + 64 * count), scal(32 * count);
  for (size_t k = 0; k < count; k++) {
    fr::El e; memcpy(e.v, evals + 32 * k, 32);
    memcpy(scal.data() + 32 * k, pw.v, 32);
    y = fr::add(y, fr::fmul(e, pw));
    pw = fr::fmul(pw, gm);
  }
  uint8_t yb[32]; memcpy(yb, y.v, 32);
  return kzg_check_run(c, g2, tau_g2, pts, scal, yb, z, proof_xy, accepted);
}

}  // extern "C"
