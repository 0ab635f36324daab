// abi_kzg.inc — C ABI: KZG commitments and openings over a resident SRS (include/sbn254.h, reference src/kzg.rs).
// The SRS is an sbn_bases handle without h and without the duplicate tables; commitments and opening proofs are msm_device over it,
// so the MSM's sort, GLV rule and window model apply unchanged.  Polynomials are the first n entries of a table, low to high.

// z^(2^k), k < 64, in the device's Montgomery form (canonical)
static void kzg_pow2_table(const uint8_t z[32], ScScalar out[64]) {
  sbn_host::fr::El x = el_from(z);
  for (int k = 0; k < 64; k++) { out[k] = scs_from(sbn_host::fr::to_dev_mont(x)); x = sbn_host::fr::mmul(sbn_host::fr::to_m(x), x); }
}
// workspace of one division: per level above the single tile, the tile values h and their carries (nt entries each)
static size_t kzg_levels_bytes(size_t n) {
  size_t bytes = 0;
  for (size_t nt = (n + KZG_TILE - 1) / KZG_TILE; nt > 1; nt = (nt + KZG_TILE - 1) / KZG_TILE) bytes += 2 * nt * 32;
  return bytes;
}
// one level of the division: p (n >= 1 entries) with the multiplier z^(2^k0).  q (qlen entries) or null; eval_dev receives p(z) as a
// canonical integer from the single-tile level.  Enqueue only.
static int kzg_div_level(sbn_ctx* c, const uint32_t* p, size_t n, const ScScalar* p2, int k0, uint32_t* q, size_t qlen, uint32_t* eval_dev, uint32_t* ws) {
  if (k0 + 2 + KZG_SCAN_STEPS > 63) return fail(c, SBN_EINVAL, "kzg: polynomial too long");
  KzgPow pw; pw.z = p2[k0];
  for (int s = 0; s < KZG_SCAN_STEPS; s++) pw.w[s] = p2[k0 + 2 + s];      // z^(E 2^s), E = 4
  const size_t nt = (n + KZG_TILE - 1) / KZG_TILE;
  if (nt == 1) {
    LAUNCH(c, "k_kzg_div_quot", k_kzg_div_quot, 1, KZG_THREADS, p, n, (const uint32_t*)nullptr, pw, q, q ? qlen : 0, eval_dev);
    return SBN_OK;
  }
  uint32_t* h = ws; uint32_t* carry = ws + 8 * nt;
  LAUNCH(c, "k_kzg_div_tiles", k_kzg_div_tiles, (unsigned)nt, KZG_THREADS, p, n, pw, h);
  int rc;
  if ((rc = kzg_div_level(c, h, nt, p2, k0 + KZG_TILE_LOG, carry, nt, eval_dev, ws + 16 * nt))) return rc;     // carry[t] = r_{t+1} of h at z^T
  if (q) LAUNCH(c, "k_kzg_div_quot", k_kzg_div_quot, (unsigned)nt, KZG_THREADS, p, n, (const uint32_t*)carry, pw, q, qlen, (uint32_t*)nullptr);
  return SBN_OK;
}
// eval = p(z) into eval_dev; q_j = r_{j+1} for j < qlen (zero from n - 1 on) when q != null.  ws: kzg_levels_bytes(n).  Enqueue only.
static int kzg_div_enqueue(sbn_ctx* c, const uint32_t* p, size_t n, const ScScalar* p2, uint32_t* q, size_t qlen, uint32_t* eval_dev, uint32_t* ws) {
  if (n == 0) { HIPCHK(c, hipMemsetAsync(eval_dev, 0, 32, c->stream)); return SBN_OK; }
  if (q && qlen > n) HIPCHK(c, hipMemsetAsync(q + 8 * n, 0, (qlen - n) * 32, c->stream));
  int rc;
  if ((rc = kzg_div_level(c, p, n, p2, 0, q, qlen, eval_dev, ws))) return rc;
  LAUNCHCHK(c);
  return SBN_OK;
}
// copy `count` 32-byte results from the device and wait
static int kzg_fetch(sbn_ctx* c, const void* dev, size_t count, uint8_t* out) {
  int rc; if ((rc = ensure_pin(c, std::max<size_t>(4096, count * 32)))) return rc;
  if (count) HIPCHK(c, hipMemcpyAsync(c->pin, dev, count * 32, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  if (c->prof) prof_drain(c);
  if (count) memcpy(out, c->pin, count * 32);
  return SBN_OK;
}
// MSM of m internal-form table entries over the SRS (m >= 1)
static int kzg_msm_internal(sbn_ctx* c, const sbn_bases* srs, const uint32_t* d, size_t m, uint8_t out_xy[64], int* out_is_inf) {
  int rc; if ((rc = ensure(c, c->scal_canon, m * 32))) return rc;
  LAUNCH(c, "k_scalars_from_mont", k_scalars_from_internal, (unsigned)((m + 255) / 256), 256, d, (uint32_t*)c->scal_canon.p, m);
  LAUNCHCHK(c);
  return msm_device(c, (const uint32_t*)c->scal_canon.p, (const uint32_t*)srs->d_pts, m, out_xy, out_is_inf, srs);
}
static void kzg_identity(uint8_t out_xy[64], int* out_is_inf) { memset(out_xy, 0, 64); if (out_is_inf) *out_is_inf = 1; }
// quotient buffer of qlen entries from the table cache
static int kzg_qbuf(sbn_ctx* c, size_t qlen, void** q, size_t* qbytes) {
  hipError_t e = pool_get(c, qlen * 32, q, qbytes);
  if (e != hipSuccess) { *q = nullptr; return fail(c, SBN_ENOMEM, "hipMalloc quotient (%zu entries): %s", qlen, hipGetErrorString(e)); }
  return SBN_OK;
}

extern "C" {

int sbn_kzg_srs_upload(sbn_ctx* c, const uint8_t* powers_xy, size_t n, uint32_t flags, sbn_bases** out) {
  if (!c || !out || (!powers_xy && n)) return SBN_EINVAL;
  std::lock_guard<std::mutex> g(c->mu);
  hipSetDevice(c->device);
  sbn_bases* b = new sbn_bases(); b->n = n; b->has_h = false;
  hipError_t e = hipMalloc(&b->d_pts, (n ? n : 1) * 64);
  if (e != hipSuccess) { delete b; return fail(c, SBN_ENOMEM, "hipMalloc SRS: %s", hipGetErrorString(e)); }
  if (n) {
    HIPCHK(c, hipMemcpyAsync(b->d_pts, powers_xy, n * 64, hipMemcpyHostToDevice, c->stream));
    if (!(flags & SBN_POINTS_MONT)) LAUNCH(c, "k_points_to_mont", k_points_to_mont, (unsigned)((n + 255) / 256), 256, (const uint32_t*)b->d_pts, (uint32_t*)b->d_pts, n);
    else LAUNCH(c, "k_points_to_mont", k_points_from_ark, (unsigned)((n + 255) / 256), 256, (const uint32_t*)b->d_pts, (uint32_t*)b->d_pts, n);
  }
  hipError_t le = hipGetLastError(), se = hipStreamSynchronize(c->stream);
  if (le != hipSuccess || se != hipSuccess) { sbn_bases_free(c, b); return fail(c, SBN_EHIP, "SRS upload: %s", hipGetErrorString(le != hipSuccess ? le : se)); }
  *out = b;
  return SBN_OK;
}

int sbn_kzg_srs_from_tau(sbn_ctx* c, const uint8_t tau[32], size_t n, sbn_bases** out) {
  if (!c || !tau || !out || n == 0) return SBN_EINVAL;
  if (!fr_canonical(tau) || sbn_host::fr::is_zero(el_from(tau))) return fail(c, SBN_EINVAL, "srs_from_tau: tau must be canonical and non-zero");
  if (n > ((size_t)1 << KZG_POW_BITS)) return fail(c, SBN_EINVAL, "srs_from_tau: n=%zu too large", n);
  std::lock_guard<std::mutex> g(c->mu);
  hipSetDevice(c->device);
  ScScalar p2[64]; kzg_pow2_table(tau, p2);
  KzgPow2 pw2; for (int k = 0; k < KZG_POW_BITS; k++) pw2.v[k] = p2[k];
  void *d_s = nullptr, *d_x = nullptr;
  sbn_bases* b = new sbn_bases(); b->n = n; b->has_h = false;
  hipError_t e = hipMalloc(&b->d_pts, n * 64);
  if (e == hipSuccess) e = hipMalloc(&d_s, n * 32);
  if (e == hipSuccess) e = hipMalloc(&d_x, n * 128);
  if (e == hipSuccess) {
    const size_t lanes = (n + KZG_POW_RUN - 1) / KZG_POW_RUN;
    LAUNCH(c, "k_fr_powers", k_fr_powers, (unsigned)((lanes + 255) / 256), 256, pw2, n, (uint32_t*)d_s);
    LAUNCH(c, "k_mul_generator", k_mul_generator, (unsigned)((n + 63) / 64), 64, (const uint32_t*)d_s, n, (uint32_t*)d_x);
    LAUNCH(c, "k_xyzz_to_affine", k_xyzz_to_affine, (unsigned)((n + 63) / 64), 64, (const uint32_t*)d_x, (uint32_t*)b->d_pts, (uint32_t*)nullptr, (uint8_t*)nullptr, n);
    e = hipGetLastError();
    const hipError_t se = hipStreamSynchronize(c->stream);
    if (e == hipSuccess) e = se;
  }
  if (d_s) hipFree(d_s);
  if (d_x) hipFree(d_x);
  if (c->prof) prof_drain(c);
  if (e != hipSuccess) { (void)hipGetLastError(); sbn_bases_free(c, b); return fail(c, SBN_EHIP, "srs_from_tau (n=%zu): %s", n, hipGetErrorString(e)); }
  *out = b;
  return SBN_OK;
}

int sbn_kzg_commit(sbn_ctx* c, const sbn_bases* srs, const sbn_table* t, size_t n, uint8_t out_xy[64], int* out_is_inf) {
  if (!c || !srs || !t || !out_xy) return SBN_EINVAL;
  if (n > t->len) return fail(c, SBN_EINVAL, "kzg_commit: n=%zu exceeds the table (%zu)", n, t->len);
  std::lock_guard<std::mutex> g(c->mu);
  hipSetDevice(c->device);
  const size_t m = std::min(n, srs->n);                 // KZGPolyCommitment::commit truncates to the SRS (kzg.rs:389)
  if (m == 0) { kzg_identity(out_xy, out_is_inf); return SBN_OK; }
  return kzg_msm_internal(c, srs, (const uint32_t*)t->d, m, out_xy, out_is_inf);
}

int sbn_poly_div_linear(sbn_ctx* c, const sbn_table* t, size_t n, const uint8_t z[32], uint8_t eval[32], sbn_table** q) {
  if (!c || !t || !z || !eval || !q) return SBN_EINVAL;
  *q = nullptr;
  if (n > t->len) return fail(c, SBN_EINVAL, "poly_div_linear: n=%zu exceeds the table (%zu)", n, t->len);
  if (!fr_canonical(z)) return fail(c, SBN_EINVAL, "poly_div_linear: z is not canonical (>= r)");
  std::lock_guard<std::mutex> g(c->mu);
  hipSetDevice(c->device);
  int rc;
  if ((rc = ensure(c, c->kzg_ws, 64 + kzg_levels_bytes(n)))) return rc;
  uint32_t* ev = (uint32_t*)c->kzg_ws.p;
  ScScalar p2[64]; kzg_pow2_table(z, p2);
  TableScope S(c); sbn_table* qt = nullptr;
  if (n >= 2) {
    size_t qlen = 1; while (qlen < n - 1) qlen <<= 1;
    if ((rc = S.alloc(qlen, "quotient", &qt))) return rc;
  }
  if ((rc = kzg_div_enqueue(c, (const uint32_t*)t->d, n, p2, qt ? (uint32_t*)qt->d : nullptr, qt ? qt->len : 0, ev, ev + 16))) return rc;
  if ((rc = kzg_fetch(c, ev, 1, eval))) return rc;
  if (qt) *q = S.give(qt);
  return S.done();
}

int sbn_kzg_open(sbn_ctx* c, const sbn_bases* srs, const sbn_table* t, size_t n, const uint8_t z[32], uint8_t eval[32], uint8_t proof_xy[64], int* proof_is_inf) {
  if (!c || !srs || !t || !z || !eval || !proof_xy) return SBN_EINVAL;
  if (n > t->len) return fail(c, SBN_EINVAL, "kzg_open: n=%zu exceeds the table (%zu)", n, t->len);
  if (!fr_canonical(z)) return fail(c, SBN_EINVAL, "kzg_open: z is not canonical (>= r)");
  if (n >= 2 && n - 1 > srs->n) return fail(c, SBN_EINVAL, "kzg_open: the quotient has %zu coefficients, the SRS %zu points (kzg.rs:186 slices past its end)", n - 1, srs->n);
  std::lock_guard<std::mutex> g(c->mu);
  hipSetDevice(c->device);
  int rc;
  if ((rc = ensure(c, c->kzg_ws, 64 + kzg_levels_bytes(n)))) return rc;
  uint32_t* ev = (uint32_t*)c->kzg_ws.p;
  ScScalar p2[64]; kzg_pow2_table(z, p2);
  void* qd = nullptr; size_t qbytes = 0;
  if (n >= 2 && (rc = kzg_qbuf(c, n - 1, &qd, &qbytes))) return rc;
  rc = kzg_div_enqueue(c, (const uint32_t*)t->d, n, p2, (uint32_t*)qd, qd ? n - 1 : 0, ev, ev + 16);
  if (rc == SBN_OK) rc = kzg_fetch(c, ev, 1, eval);
  if (rc == SBN_OK) {
    if (qd) rc = kzg_msm_internal(c, srs, (const uint32_t*)qd, n - 1, proof_xy, proof_is_inf);
    else kzg_identity(proof_xy, proof_is_inf);                       // n <= 1: an empty quotient (kzg.rs:183-184)
  }
  if (qd) { hipStreamSynchronize(c->stream); pool_put(c, qd, qbytes); }
  return rc;
}

int sbn_kzg_open_batched(sbn_ctx* c, const sbn_bases* srs, const sbn_table* const* ts, const size_t* ns, size_t count, const uint8_t z[32], const uint8_t gamma[32],
                         uint8_t* evals, uint8_t proof_xy[64], int* proof_is_inf) {
  if (!c || !srs || !z || !gamma || !proof_xy || (count && (!ts || !ns || !evals))) return SBN_EINVAL;
  if (!fr_canonical(z) || !fr_canonical(gamma)) return fail(c, SBN_EINVAL, "kzg_open_batched: z or gamma is not canonical (>= r)");
  size_t maxn = 0;
  for (size_t k = 0; k < count; k++) {
    if (!ts[k]) return SBN_EINVAL;
    if (ns[k] > ts[k]->len) return fail(c, SBN_EINVAL, "kzg_open_batched: ns[%zu]=%zu exceeds its table (%zu)", k, ns[k], ts[k]->len);
    maxn = std::max(maxn, ns[k]);
  }
  if (maxn >= 2 && maxn - 1 > srs->n) return fail(c, SBN_EINVAL, "kzg_open_batched: the quotient has %zu coefficients, the SRS %zu points", maxn - 1, srs->n);
  if (count == 0) { kzg_identity(proof_xy, proof_is_inf); return SBN_OK; }    // no polynomials: the identity (kzg.rs:278-303 over empty vectors)
  std::lock_guard<std::mutex> g(c->mu);
  hipSetDevice(c->device);
  // workspace: count + 1 eval slots, the combination's arguments (pointers, lengths, gamma^k), then the division levels
  const size_t ev_bytes = ((count + 1) * 32 + 255) & ~(size_t)255;
  const size_t arg_bytes = ((count * (8 + 8 + 32)) + 255) & ~(size_t)255;
  int rc;
  if ((rc = ensure(c, c->kzg_ws, ev_bytes + arg_bytes + kzg_levels_bytes(maxn)))) return rc;
  uint8_t* ws = (uint8_t*)c->kzg_ws.p;
  uint32_t* ev = (uint32_t*)ws;
  const uint32_t** d_tabs = (const uint32_t**)(ws + ev_bytes);
  size_t* d_ns = (size_t*)(ws + ev_bytes + count * 8);
  uint32_t* d_gp = (uint32_t*)(ws + ev_bytes + count * 16);
  uint32_t* lv = (uint32_t*)(ws + ev_bytes + arg_bytes);
  ScScalar p2[64]; kzg_pow2_table(z, p2);
  // evals[k] = p_k(z) (KZGBatchedEvalProof::prove, kzg.rs:485-488)
  for (size_t k = 0; k < count && rc == SBN_OK; k++) rc = kzg_div_enqueue(c, (const uint32_t*)ts[k]->d, ns[k], p2, nullptr, 0, ev + 8 * k, lv);
  void *comb = nullptr, *qd = nullptr; size_t comb_bytes = 0, qbytes = 0;
  std::vector<uint8_t> args(count * 48);
  if (rc == SBN_OK && maxn >= 2) {
    // the combined polynomial sum_k gamma^k p_k over maxn coefficients (kzg.rs:278-288) and its quotient (kzg.rs:299); its value at z
    // (slot count) is sum_k gamma^k evals[k] (kzg.rs:291-296), which the quotient does not depend on
    sbn_host::fr::El gk = sbn_host::fr::from_u64(1);
    const sbn_host::fr::El gm = sbn_host::fr::to_m(el_from(gamma));
    for (size_t k = 0; k < count; k++) {
      const uint64_t pk = (uint64_t)(uintptr_t)ts[k]->d, nk = (uint64_t)ns[k];
      memcpy(&args[8 * k], &pk, 8); memcpy(&args[count * 8 + 8 * k], &nk, 8);
      const sbn_host::fr::El m = sbn_host::fr::to_dev_mont(gk);
      memcpy(&args[count * 16 + 32 * k], m.v, 32);
      gk = sbn_host::fr::mmul(gm, gk);
    }
    if ((rc = kzg_qbuf(c, maxn, &comb, &comb_bytes)) == SBN_OK && (rc = kzg_qbuf(c, maxn - 1, &qd, &qbytes)) == SBN_OK) {
      hipError_t e = hipMemcpyAsync(d_tabs, args.data(), count * 48, hipMemcpyHostToDevice, c->stream);
      if (e != hipSuccess) rc = fail(c, SBN_EHIP, "kzg_open_batched: %s", hipGetErrorString(e));
    }
    if (rc == SBN_OK) {
      LAUNCH(c, "k_kzg_combine", k_kzg_combine, stream_grid(maxn), 256, (const uint32_t* const*)d_tabs, (const size_t*)d_ns, (const uint32_t*)d_gp, count, maxn, (uint32_t*)comb);
      rc = kzg_div_enqueue(c, (const uint32_t*)comb, maxn, p2, (uint32_t*)qd, maxn - 1, ev + 8 * count, lv);
    }
  }
  if (rc == SBN_OK) rc = kzg_fetch(c, ev, count, evals);
  if (rc == SBN_OK) {
    if (qd) rc = kzg_msm_internal(c, srs, (const uint32_t*)qd, maxn - 1, proof_xy, proof_is_inf);
    else kzg_identity(proof_xy, proof_is_inf);
  }
  hipStreamSynchronize(c->stream);
  if (comb) pool_put(c, comb, comb_bytes);
  if (qd) pool_put(c, qd, qbytes);
  return rc;
}

}  // extern "C"
