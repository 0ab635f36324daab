// abi_kzg_srs.inc — C ABI: the KZG SRS as a file buffer (include/sbn254.h; reference kzg.rs:66-115, KZGSrs::load_from_file / save_to_file).
//   sbn_kzg_srs_load          file bytes -> the handle sbn_kzg_srs_upload makes and the two handles sbn_g2_prepare makes.  The host reads the length field
//                             and decompresses the two G2 points (srs_host.hpp); the n powers go up in chunks through pinned staging, the copy of chunk
//                             k + 1 beside k_srs_decompress of chunk k, and land in the handle's layout with nothing else written per point.
//   sbn_kzg_srs_check         are the powers the powers of ONE tau that matches tau_g2?  One MSM over the handle, two short sums, one pairing product.
//   sbn_kzg_srs_save          the other direction: k_srs_compress in the same chunks, the two G2 points compressed on the host.
//   sbn_ptau_scan             host only: the section table and the header section of a powers-of-tau ceremony file (ptau_host.hpp)
//   sbn_kzg_srs_load_ptau     the bytes of a .ptau file -> the same three handles: the first n points of section 2 through the SAME chunk loop with 64-byte
//                             points and k_ptau_points (no square root), points 0 and 1 of section 3 converted on the host
//   sbn_kzg_srs_g2_from_tau   host only: g2 and [tau] g2 for a caller who supplies tau (with sbn_kzg_srs_from_tau: the "generate" half of load_or_generate).
// Included by sbn254.hip; needs abi_kzg.inc (kzg_pow2_table), abi_small_sums.inc and abi_pairing.inc.

// The chunk is sbn_ctx::srs_chunk points (2^18 = 8 MiB of file bytes unless SBN_SRS_CHUNK says otherwise; DESIGN, "the SRS from a file").

// two pinned staging buffers and two device buffers of `chunk` points of `width` file bytes each (32: a compressed power; 64: a point of a .ptau file)
static int srs_staging(sbn_ctx* c, size_t chunk, size_t width = 32) {
  const size_t bytes = chunk * width;
  int rc;
  for (int k = 0; k < 2; k++) if ((rc = ensure(c, c->zstage[k], bytes + 64))) return rc;
  if (!c->copy_stream) HIPCHK(c, hipStreamCreateWithFlags(&c->copy_stream, hipStreamNonBlocking));
  if (bytes <= c->srs_pin_cap) return SBN_OK;
  HIPCHK(c, hipStreamSynchronize(c->stream));
  for (int k = 0; k < 2; k++) if (c->srs_pin[k]) { HIPCHK(c, hipHostFree(c->srs_pin[k])); c->srs_pin[k] = nullptr; }
  c->srs_pin_cap = 0;
  for (int k = 0; k < 2; k++) HIPCHK(c, hipHostMalloc(&c->srs_pin[k], bytes, hipHostMallocDefault));
  c->srs_pin_cap = bytes;
  return SBN_OK;
}
// why the device refused power i, from its 32 bytes
static const char* srs_g1_reason(const uint8_t p[32]) {
  const unsigned flags = p[31] >> 6;
  if (flags == 3) return "both flag bits are set";
  if (flags & 1) return "the identity is no power of tau";
  uint64_t x[4]; uint8_t t[32]; memcpy(t, p, 32); t[31] &= 0x3f; memcpy(x, t, 32);
  if (sbn_host::geq_p(x)) return "x is not canonical (>= q)";
  return "x^3 + 3 is not a square";
}
// the words of the refusal index: the device word lives behind the input-check counter, its two pinned copies behind that counter's copy
static unsigned long long* srs_bad_dev(sbn_ctx* c) { return (unsigned long long*)(c->d_bad + 2); }
static volatile unsigned long long* srs_bad_host(sbn_ctx* c, int k) { return (volatile unsigned long long*)(c->h_bad + 2 + 2 * k); }

// the n points at `in` into b->d_pts (n >= 1; the context's mutex is held).  *bad <- the smallest refused index, or SIZE_MAX.  The ONE chunk loop of both
// loads: `width` is the file's bytes per point and picks the kernel, 32 = k_srs_decompress (a compressed power), 64 = k_ptau_points (x | y in ark-ff's
// Montgomery limbs); a chunk is srs_chunk points whatever its width.
static int srs_load_chunks(sbn_ctx* c, const uint8_t* in, size_t n, size_t width, uint32_t* d_pts, size_t* bad) {
  const size_t chunk = std::min(c->srs_chunk, n), nchunks = (n + chunk - 1) / chunk;
  int rc;
  if ((rc = srs_staging(c, chunk, width))) return rc;
  HIPCHK(c, hipMemsetAsync(srs_bad_dev(c), 0xff, 8, c->stream));
  hipEvent_t copied[2], done[2];
  for (int k = 0; k < 2; k++) { copied[k] = evt_get(c); done[k] = evt_get(c); }
  hipError_t e = hipSuccess;
  bool stop = false;
  for (size_t i = 0; i < nchunks && e == hipSuccess && !stop; i++) {
    const int k = (int)(i & 1);
    const size_t first = i * chunk, cnt = std::min(chunk, n - first);
    // chunk i - 2 has left both staging buffers, and its copy of the refusal word has landed: the one host read a chunk
    if (i >= 2) { e = hipEventSynchronize(done[k]); if (e != hipSuccess) break; if (*srs_bad_host(c, k) != ~0ull) { stop = true; break; } }
    memcpy(c->srs_pin[k], in + width * first, width * cnt);
    e = hipMemcpyAsync(c->zstage[k].p, c->srs_pin[k], width * cnt, hipMemcpyHostToDevice, c->copy_stream);
    if (e == hipSuccess) e = hipEventRecord(copied[k], c->copy_stream);
    if (e == hipSuccess) e = hipStreamWaitEvent(c->stream, copied[k], 0);
    if (e != hipSuccess) break;
    if (width == 32) LAUNCH(c, "k_srs_decompress", k_srs_decompress, (unsigned)((cnt + 63) / 64), 64, (const uint32_t*)c->zstage[k].p, cnt, first, d_pts, srs_bad_dev(c));
    else LAUNCH(c, "k_ptau_points", k_ptau_points, (unsigned)((cnt + 63) / 64), 64, (const uint32_t*)c->zstage[k].p, cnt, first, d_pts, srs_bad_dev(c));
    e = hipGetLastError();
    if (e == hipSuccess) e = hipMemcpyAsync((void*)srs_bad_host(c, k), srs_bad_dev(c), 8, hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipEventRecord(done[k], c->stream);
  }
  // drained on every path: what is still queued ran in file order, so the word holds the smallest index of the first chunk with a refusal
  if (e == hipSuccess) e = hipMemcpyAsync((void*)srs_bad_host(c, 0), srs_bad_dev(c), 8, hipMemcpyDeviceToHost, c->stream);
  hipStreamSynchronize(c->copy_stream);
  const hipError_t es = hipStreamSynchronize(c->stream);
  if (e == hipSuccess) e = es;
  for (int k = 0; k < 2; k++) { c->evt_pool.push_back(copied[k]); c->evt_pool.push_back(done[k]); }
  if (c->prof) prof_drain(c);
  if (e != hipSuccess) { (void)hipGetLastError(); return fail(c, SBN_EHIP, "srs load (n=%zu): %s", n, hipGetErrorString(e)); }
  const unsigned long long w = *srs_bad_host(c, 0);
  *bad = w == ~0ull ? SIZE_MAX : (size_t)w;
  return SBN_OK;
}

// the handle's n points as n x 32 file bytes at `out` (n >= 1; the context's mutex is held)
static int srs_compress_chunks(sbn_ctx* c, const uint32_t* d_pts, size_t n, uint8_t* out) {
  const size_t chunk = std::min(c->srs_chunk, n), nchunks = (n + chunk - 1) / chunk;
  int rc;
  if ((rc = srs_staging(c, chunk))) return rc;
  hipEvent_t packed[2], landed[2];
  for (int k = 0; k < 2; k++) { packed[k] = evt_get(c); landed[k] = evt_get(c); }
  hipError_t e = hipSuccess;
  auto span = [&](size_t i, size_t* first, size_t* cnt) { *first = i * chunk; *cnt = std::min(chunk, n - *first); };
  for (size_t i = 0; i < nchunks && e == hipSuccess; i++) {
    const int k = (int)(i & 1);
    size_t first, cnt; span(i, &first, &cnt);
    // chunk i - 2 has landed in the pinned buffer: out it goes, and both staging buffers of this parity are free
    if (i >= 2) { e = hipEventSynchronize(landed[k]); if (e != hipSuccess) break; size_t f2, c2; span(i - 2, &f2, &c2); memcpy(out + 32 * f2, c->srs_pin[k], 32 * c2); }
    LAUNCH(c, "k_srs_compress", k_srs_compress, (unsigned)((cnt + 63) / 64), 64, d_pts, cnt, first, (uint32_t*)c->zstage[k].p);
    e = hipGetLastError();
    if (e == hipSuccess) e = hipEventRecord(packed[k], c->stream);
    if (e == hipSuccess) e = hipStreamWaitEvent(c->copy_stream, packed[k], 0);
    if (e == hipSuccess) e = hipMemcpyAsync(c->srs_pin[k], c->zstage[k].p, 32 * cnt, hipMemcpyDeviceToHost, c->copy_stream);
    if (e == hipSuccess) e = hipEventRecord(landed[k], c->copy_stream);
  }
  for (size_t i = nchunks > 2 ? nchunks - 2 : 0; i < nchunks && e == hipSuccess; i++) {
    const int k = (int)(i & 1);
    size_t first, cnt; span(i, &first, &cnt);
    e = hipEventSynchronize(landed[k]);
    if (e == hipSuccess) memcpy(out + 32 * first, c->srs_pin[k], 32 * cnt);
  }
  hipStreamSynchronize(c->copy_stream);
  const hipError_t es = hipStreamSynchronize(c->stream);
  if (e == hipSuccess) e = es;
  for (int k = 0; k < 2; k++) { c->evt_pool.push_back(packed[k]); c->evt_pool.push_back(landed[k]); }
  if (c->prof) prof_drain(c);
  if (e != hipSuccess) { (void)hipGetLastError(); return fail(c, SBN_EHIP, "srs save (n=%zu): %s", n, hipGetErrorString(e)); }
  return SBN_OK;
}

// 32 bytes from the OS as a scalar in [1, 2^253): the batching coefficient of a load with SBN_SRS_CHECK
static bool srs_draw_rho(uint8_t rho[32]) {
  FILE* f = fopen("/dev/urandom", "rb");
  if (!f) return false;
  const size_t got = fread(rho, 1, 32, f);
  fclose(f);
  if (got != 32) return false;
  rho[31] &= 0x1f;
  bool zero = true; for (int k = 0; k < 32; k++) if (rho[k]) zero = false;
  if (zero) rho[0] = 1;
  return true;
}

// why the device refused point i of a .ptau file, from its 64 bytes
static const char* ptau_g1_reason(const uint8_t p[64]) {
  uint64_t x[4], y[4]; memcpy(x, p, 32); memcpy(y, p + 32, 32);
  if (sbn_host::geq_p(x) || sbn_host::geq_p(y)) return "a coordinate is not canonical (>= q)";
  bool zero = true; for (int k = 0; k < 64; k++) if (p[k]) zero = false;
  if (zero) return "the identity is no power of tau";
  return "the point is not on the curve (y^2 != x^3 + 3)";
}

// What sbn_kzg_srs_load and sbn_kzg_srs_load_ptau share behind their parsers: n points of `width` file bytes at `in` into a fresh handle (srs_load_chunks), the
// two G2 handles from g2s (g2 | tau_g2, canonical bytes), the check under SBN_SRS_CHECK, and the refusal conventions.  `what` opens every error text.
static int srs_load_points(sbn_ctx* c, const char* what, const uint8_t* in, size_t n, size_t width, const uint8_t g2s[256], uint32_t flags, sbn_bases** out_srs,
                           sbn_g2_lines** out_g2, sbn_g2_lines** out_tau_g2, uint8_t out_g2_xy[256], size_t* bad_index) {
  sbn_bases* b = nullptr;
  int rc;
  {
    std::lock_guard<std::mutex> g(c->mu);
    hipSetDevice(c->device);
    b = new sbn_bases(); b->n = n; b->has_h = false;
    const hipError_t he = hipMalloc(&b->d_pts, n * 64);
    if (he != hipSuccess) { delete b; return fail(c, SBN_ENOMEM, "hipMalloc SRS (%zu points): %s", n, hipGetErrorString(he)); }
    size_t bad = SIZE_MAX;
    rc = srs_load_chunks(c, in, n, width, (uint32_t*)b->d_pts, &bad);
    if (rc == SBN_OK && bad != SIZE_MAX) {
      if (bad_index) *bad_index = bad;
      rc = fail(c, SBN_EINVAL, "%s: power %zu: %s", what, bad, width == 32 ? srs_g1_reason(in + 32 * bad) : ptau_g1_reason(in + 64 * bad));
    }
    if (rc) { sbn_bases_free(c, b); return rc; }
  }
  sbn_g2_lines *l_g2 = nullptr, *l_tau = nullptr;
  const bool want_lines = out_g2 != nullptr || (flags & SBN_SRS_CHECK);
  if (want_lines) {
    rc = sbn_g2_prepare(c, g2s, 0, &l_g2);
    if (rc == SBN_OK) rc = sbn_g2_prepare(c, g2s + 128, 0, &l_tau);
  }
  if (rc == SBN_OK && (flags & SBN_SRS_CHECK)) {
    uint8_t rho[32]; int ok = 0;
    if (!srs_draw_rho(rho)) rc = fail(c, SBN_EHIP, "%s: no randomness from the OS for the consistency check", what);
    else if ((rc = sbn_kzg_srs_check(c, b, l_g2, l_tau, rho, &ok)) == SBN_OK && !ok)
      rc = fail(c, SBN_EINVAL, "%s: the powers are not the powers of one tau that matches tau_g2 (sbn_kzg_srs_check)", what);
  }
  if (rc || !out_g2) { sbn_g2_lines_free(c, l_g2); sbn_g2_lines_free(c, l_tau); l_g2 = l_tau = nullptr; }
  if (rc) { std::lock_guard<std::mutex> g(c->mu); sbn_bases_free(c, b); return rc; }
  *out_srs = b;
  if (out_g2) { *out_g2 = l_g2; *out_tau_g2 = l_tau; }
  if (out_g2_xy) memcpy(out_g2_xy, g2s, 256);
  return SBN_OK;
}

extern "C" {

int sbn_kzg_srs_g2_from_tau(const uint8_t tau[32], uint8_t out_g2_xy[128], uint8_t out_tau_g2_xy[128]) {
  if (!tau || !out_g2_xy || !out_tau_g2_xy) return SBN_EINVAL;
  return sbn_host::srs::g2_from_tau(tau, out_g2_xy, out_tau_g2_xy) ? SBN_OK : SBN_EINVAL;
}

int sbn_kzg_srs_check(sbn_ctx* c, const sbn_bases* srs, const sbn_g2_lines* g2, const sbn_g2_lines* tau_g2, const uint8_t rho[32], int* consistent) {
  namespace fr = sbn_host::fr;
  if (!c) return SBN_EINVAL;
  if (!srs || !g2 || !tau_g2 || !rho || !consistent) return fail(c, SBN_EINVAL, "srs check: a null pointer");
  if (g2->ctx != c || tau_g2->ctx != c) return fail(c, SBN_EINVAL, "srs check: a G2 handle of another context");
  if (!fr_canonical(rho) || fr::is_zero(el_from(rho))) return fail(c, SBN_EINVAL, "srs check: rho must be canonical (< r) and non-zero");
  const size_t n = srs->n;
  if (n == 0) return fail(c, SBN_EINVAL, "srs check: the SRS holds no powers");
  if (n > ((size_t)1 << KZG_POW_BITS)) return fail(c, SBN_EINVAL, "srs check: n=%zu too large", n);
  static const uint8_t G1_GEN[64] = {1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 2};
  int rc;
  // pts: T, P_0, T, P_{n-1}
  uint8_t pts[4 * 64];
  if ((rc = sbn_bases_download(c, srs, 0, 1, pts + 64))) return rc;
  if (memcmp(pts + 64, G1_GEN, 64)) { *consistent = 0; return SBN_OK; }        // P_0 is the G that sbn_kzg_verify hard-wires
  if (n == 1) { *consistent = 1; return SBN_OK; }
  if ((rc = sbn_bases_download(c, srs, n - 1, 1, pts + 192))) return rc;
  // T = sum_i rho^i P_i: the scalars of an SRS in rho (k_fr_powers), the MSM of a commitment
  {
    std::lock_guard<std::mutex> g(c->mu);
    hipSetDevice(c->device);
    if ((rc = ensure(c, c->scal_canon, n * 32))) return rc;
    ScScalar p2[64]; kzg_pow2_table(rho, p2);
    KzgPow2 pw2; for (int k = 0; k < KZG_POW_BITS; k++) pw2.v[k] = p2[k];
    const size_t lanes = (n + KZG_POW_RUN - 1) / KZG_POW_RUN;
    LAUNCH(c, "k_fr_powers", k_fr_powers, (unsigned)((lanes + 255) / 256), 256, pw2, n, (uint32_t*)c->scal_canon.p);
    LAUNCHCHK(c);
    if ((rc = msm_device(c, (const uint32_t*)c->scal_canon.p, (const uint32_t*)srs->d_pts, n, pts, nullptr, srs))) return rc;
  }
  memcpy(pts + 128, pts, 64);
  // A = T - P_0 and -B = -rho T + rho^n P_{n-1}: e(A, g2) e(-B, tau_g2) = 1 exactly when sum_i rho^(i+1) (P_{i+1} - tau P_i) = O
  const fr::El one = fr::from_u64(1), zero = fr::from_u64(0), r = el_from(rho), rm = fr::to_m(r);
  fr::El rn = one;                                                              // rho^n, left to right over the bits of n
  for (int i = 63; i >= 0; i--) { rn = fr::mmul(fr::to_m(rn), rn); if ((n >> i) & 1) rn = fr::mmul(rm, rn); }
  const fr::El sc[4] = {one, fr::sub(zero, one), fr::sub(zero, r), rn};
  uint8_t scal[4 * 32];
  for (int k = 0; k < 4; k++) memcpy(scal + 32 * k, sc[k].v, 32);
  const uint32_t counts[2] = {2, 2};
  uint8_t pair_p[128];
  if ((rc = sbn_g1_small_sums(c, pts, scal, counts, 2, pair_p, nullptr))) return rc;
  const sbn_g2_lines* qs[2] = {g2, tau_g2};
  const uint32_t two = 2;
  uint8_t is_one = 0;
  if ((rc = sbn_pairing_products(c, pair_p, qs, &two, 1, &is_one, nullptr))) return rc;
  *consistent = is_one ? 1 : 0;
  return SBN_OK;
}

int sbn_kzg_srs_load(sbn_ctx* c, const uint8_t* bytes, size_t len, uint32_t flags, sbn_bases** out_srs, sbn_g2_lines** out_g2, sbn_g2_lines** out_tau_g2,
                     uint8_t out_g2_xy[256], size_t* bad_index) {
  namespace sr = sbn_host::srs;
  if (!c) return SBN_EINVAL;
  if (out_srs) *out_srs = nullptr;
  if (out_g2) *out_g2 = nullptr;
  if (out_tau_g2) *out_tau_g2 = nullptr;
  if (bad_index) *bad_index = SIZE_MAX;
  if (!out_srs || (!bytes && len)) return fail(c, SBN_EINVAL, "srs load: a null pointer");
  if (flags & ~SBN_SRS_CHECK) return fail(c, SBN_EINVAL, "srs load: unknown flags 0x%x", flags);
  if ((out_g2 == nullptr) != (out_tau_g2 == nullptr)) return fail(c, SBN_EINVAL, "srs load: the two G2 handles come together or not at all");
  sr::Scan s;
  int e = sr::scan(bytes, len, &s);
  if (e) return fail(c, SBN_EINVAL, "srs load: %s", sr::err_text(e));
  uint8_t g2s[256];                                                             // g2 | tau_g2
  if ((e = sr::g2_decompress(bytes + s.tau_g2_off, g2s + 128))) return fail(c, SBN_EINVAL, "srs load: tau_g2: %s", sr::err_text(e));
  if ((e = sr::g2_decompress(bytes + s.g2_off, g2s))) return fail(c, SBN_EINVAL, "srs load: g2: %s", sr::err_text(e));
  return srs_load_points(c, "srs load", bytes + s.powers_off, (size_t)s.n, 32, g2s, flags, out_srs, out_g2, out_tau_g2, out_g2_xy, bad_index);
}

int sbn_ptau_scan(const uint8_t* bytes, size_t len, sbn_ptau_info* out) {
  namespace pt = sbn_host::ptau;
  if ((!bytes && len) || !out) return SBN_EINVAL;
  pt::Scan s;
  if (pt::scan(bytes, len, &s)) return SBN_EINVAL;
  out->power = s.power; out->ceremony_power = s.ceremony_power; out->n_g1 = s.n_g1; out->n_g2 = s.n_g2; out->off_g1 = s.off_g1; out->off_g2 = s.off_g2;
  return SBN_OK;
}

int sbn_kzg_srs_load_ptau(sbn_ctx* c, const uint8_t* bytes, size_t len, size_t n, uint32_t flags, sbn_bases** out_srs, sbn_g2_lines** out_g2,
                          sbn_g2_lines** out_tau_g2, uint8_t out_g2_xy[256], size_t* bad_index) {
  namespace pt = sbn_host::ptau;
  if (!c) return SBN_EINVAL;
  if (out_srs) *out_srs = nullptr;
  if (out_g2) *out_g2 = nullptr;
  if (out_tau_g2) *out_tau_g2 = nullptr;
  if (bad_index) *bad_index = SIZE_MAX;
  if (!out_srs || (!bytes && len)) return fail(c, SBN_EINVAL, "ptau load: a null pointer");
  if (flags & ~SBN_SRS_CHECK) return fail(c, SBN_EINVAL, "ptau load: unknown flags 0x%x", flags);
  if ((out_g2 == nullptr) != (out_tau_g2 == nullptr)) return fail(c, SBN_EINVAL, "ptau load: the two G2 handles come together or not at all");
  pt::Scan s;
  int e = pt::scan(bytes, len, &s);
  if (e) return fail(c, SBN_EINVAL, "ptau load: %s", pt::err_text(e));
  if (n > s.n_g1) return fail(c, SBN_EINVAL, "ptau load: n=%zu, the file holds %llu powers", n, (unsigned long long)s.n_g1);
  if (n == 0) n = (size_t)s.n_g1;
  uint8_t g2s[256];                                                             // g2 | tau_g2: points 0 and 1 of section 3
  if ((e = pt::g2_convert(bytes + s.off_g2 + 128, g2s + 128))) return fail(c, SBN_EINVAL, "ptau load: tau_g2: %s", pt::err_text(e));
  if ((e = pt::g2_convert(bytes + s.off_g2, g2s))) return fail(c, SBN_EINVAL, "ptau load: g2: %s", pt::err_text(e));
  return srs_load_points(c, "ptau load", bytes + s.off_g1, n, 64, g2s, flags, out_srs, out_g2, out_tau_g2, out_g2_xy, bad_index);
}

int sbn_kzg_srs_save(sbn_ctx* c, const sbn_bases* srs, const uint8_t g2_xy[128], const uint8_t tau_g2_xy[128], uint32_t flags, uint8_t* out, size_t cap, size_t* out_len) {
  namespace sr = sbn_host::srs;
  if (!c) return SBN_EINVAL;
  if (!srs || !out_len) return fail(c, SBN_EINVAL, "srs save: a null pointer");
  if (flags & ~SBN_POINTS_MONT) return fail(c, SBN_EINVAL, "srs save: unknown flags 0x%x", flags);
  const size_t n = srs->n;
  size_t need = 0;
  if (!sr::file_bytes(n, &need)) return fail(c, SBN_EINVAL, "srs save: n=%zu too large", n);
  *out_len = need;
  if (!out) return SBN_OK;                                                      // the size query
  if (!g2_xy || !tau_g2_xy) return fail(c, SBN_EINVAL, "srs save: a null pointer");
  if (cap < need) return fail(c, SBN_EINVAL, "srs save: the buffer holds %zu bytes, the file needs %zu", cap, need);
  uint8_t tail[128];
  int e;
  if ((e = sr::g2_compress(tau_g2_xy, (flags & SBN_POINTS_MONT) != 0, tail))) return fail(c, SBN_EINVAL, "srs save: tau_g2: %s", sr::err_text(e));
  if ((e = sr::g2_compress(g2_xy, (flags & SBN_POINTS_MONT) != 0, tail + 64))) return fail(c, SBN_EINVAL, "srs save: g2: %s", sr::err_text(e));
  if (n) {
    std::lock_guard<std::mutex> g(c->mu);
    hipSetDevice(c->device);
    int rc;
    if ((rc = srs_compress_chunks(c, (const uint32_t*)srs->d_pts, n, out + 8))) return rc;
  }
  const uint64_t n64 = n;
  for (int k = 0; k < 8; k++) out[k] = (uint8_t)(n64 >> (8 * k));
  memcpy(out + 8 + 32 * n, tail, 128);
  return SBN_OK;
}

}  // extern "C"
