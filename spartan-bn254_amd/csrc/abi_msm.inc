// abi_msm.inc — C ABI: context, device memory, generator tables, MSM and commitments (include/sbn254.h, B1 + B2).
// ------------------------------------------------------------------------------------------------ C ABI
extern "C" {

const char* sbn_version(void) { return "sbn254-hip 0.1 (gfx950)"; }

int sbn_ctx_create(int device, sbn_ctx** out) {
  if (!out) return SBN_EINVAL;
  *out = nullptr;
  int count = 0;
  if (hipGetDeviceCount(&count) != hipSuccess || count <= 0) return SBN_ENODEV;
  if (device < 0 || device >= count) return SBN_ENODEV;
  if (hipSetDevice(device) != hipSuccess) return SBN_ENODEV;
  sbn_ctx* c = new sbn_ctx();
  c->device = device;
  if (hipStreamCreateWithFlags(&c->own_stream, hipStreamNonBlocking) != hipSuccess) { delete c; return SBN_EHIP; }
  c->stream = c->own_stream;
  if (hipMalloc((void**)&c->d_bad, 64) != hipSuccess || hipHostMalloc((void**)&c->h_bad, 64, hipHostMallocDefault) != hipSuccess || hipMemset(c->d_bad, 0, 64) != hipSuccess) {
    if (c->d_bad) hipFree(c->d_bad);
    hipStreamDestroy(c->own_stream); delete c; return SBN_ENOMEM;
  }
  *c->h_bad = 0;
  c->sck = sc_knobs_read();
  // 128 KiB of dynamic LDS per sort block (32768 counters); gfx950 has 160 KiB per CU
  if (hipFuncSetAttribute((const void*)k_hist_lds, hipFuncAttributeMaxDynamicSharedMemorySize, 32768 * 4) == hipSuccess &&
      hipFuncSetAttribute((const void*)k_scatter_lds, hipFuncAttributeMaxDynamicSharedMemorySize, 32768 * 4) == hipSuccess) c->sort_rs_max = 32768;
  else (void)hipGetLastError();
  if (hipFuncSetAttribute((const void*)k_sort_rows, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024) == hipSuccess) c->sort_rows_ok = true;
  else (void)hipGetLastError();
  c->sort2_ok = sort2_set_lds();
  if (const char* e2 = getenv("SBN_SORT2_MIN")) c->sort2_min = (size_t)strtoull(e2, nullptr, 0);
  if (const char* eg = getenv("SBN_MSM_GLV")) { const int v = atoi(eg); if (v == 0 || v == 1) c->msm_glv = v; }
  if (const char* es = getenv("SBN_SRS_CHUNK")) { const long long v = atoll(es); if (v >= 1 && v <= (1ll << 26)) c->srs_chunk = (size_t)v; }   // tests: force many small chunks
  *out = c;
  return SBN_OK;
}
void sbn_ctx_destroy(sbn_ctx* c) {
  if (!c) return;
  hipSetDevice(c->device);
  hipStreamSynchronize(c->stream);
  prof_drain(c);
  DevBuf* bufs[] = {&c->scal_canon, &c->hist, &c->offs, &c->sorted, &c->buckets, &c->red_a, &c->red_b, &c->wsum, &c->stage_scal, &c->stage_pts, &c->out_small,
                    &c->sc_args, &c->sc_partial, &c->sc_out, &c->sc_r, &c->sc_tabs, &c->sc_tickets, &c->sc_prove, &c->gen_tmp, &c->acc_ctr, &c->extra_list, &c->extra_out, &c->big_list, &c->digits, &c->blockhist, &c->perm, &c->merged, &c->zstage[0], &c->zstage[1], &c->out_rows, &c->comb_partial, &c->s2_cnt, &c->s2_part, &c->s2_idx, &c->s2_lo, &c->glv_scal, &c->kzg_ws, &c->r1cs_ws, &c->dense_ws};
  for (DevBuf* b : bufs) if (b->p) hipFree(b->p);
  for (auto& b : c->pool) hipFree(b.first);
  if (c->pin) hipHostFree(c->pin);
  for (void* p : c->srs_pin) if (p) hipHostFree(p);
  if (c->d_bad) hipFree(c->d_bad);
  if (c->h_bad) hipHostFree(c->h_bad);
  if (c->mbox) hipHostFree(c->mbox);
  if (c->vbox) hipHostFree(c->vbox);
  if (c->sbox) hipHostFree(c->sbox);
  for (hipEvent_t e : c->evt_pool) hipEventDestroy(e);
  if (c->copy_stream) hipStreamDestroy(c->copy_stream);
  if (c->pp_stream) hipStreamDestroy(c->pp_stream);
  hipStreamDestroy(c->own_stream);
  delete c;
}
const char* sbn_last_error(const sbn_ctx* c) { return c ? c->err.c_str() : "null context"; }
// the old stream is drained first: cached buffers are recycled in stream order, which only holds within one stream
int sbn_ctx_set_stream(sbn_ctx* c, void* s) { if (!c) return SBN_EINVAL; std::lock_guard<std::mutex> g(c->mu); hipSetDevice(c->device); HIPCHK(c, hipStreamSynchronize(c->stream)); if (c->prof) prof_drain(c); c->stream = s ? (hipStream_t)s : c->own_stream; return SBN_OK; }
int sbn_ctx_sync(sbn_ctx* c) { if (!c) return SBN_EINVAL; std::lock_guard<std::mutex> g(c->mu); HIPCHK(c, hipStreamSynchronize(c->stream)); if (c->prof) prof_drain(c); return SBN_OK; }

int sbn_dev_alloc(sbn_ctx* c, size_t bytes, void** out) { if (!c || !out) return SBN_EINVAL; std::lock_guard<std::mutex> g(c->mu); hipSetDevice(c->device); hipError_t e = hipMalloc(out, bytes ? bytes : 1); if (e != hipSuccess) return fail(c, SBN_ENOMEM, "hipMalloc(%zu): %s", bytes, hipGetErrorString(e)); return SBN_OK; }
int sbn_dev_free(sbn_ctx* c, void* p) { if (!c) return SBN_EINVAL; std::lock_guard<std::mutex> g(c->mu); hipSetDevice(c->device); HIPCHK(c, hipStreamSynchronize(c->stream)); HIPCHK(c, hipFree(p)); return SBN_OK; }
int sbn_dev_upload(sbn_ctx* c, void* dst, const void* src, size_t bytes) { if (!c || (!dst && bytes) || (!src && bytes)) return SBN_EINVAL; std::lock_guard<std::mutex> g(c->mu); HIPCHK(c, hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, c->stream)); HIPCHK(c, hipStreamSynchronize(c->stream)); return SBN_OK; }
int sbn_dev_download(sbn_ctx* c, void* dst, const void* src, size_t bytes) { if (!c || (!dst && bytes) || (!src && bytes)) return SBN_EINVAL; std::lock_guard<std::mutex> g(c->mu); HIPCHK(c, hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, c->stream)); HIPCHK(c, hipStreamSynchronize(c->stream)); return SBN_OK; }

int sbn_bases_upload(sbn_ctx* c, const uint8_t* G_xy, size_t n, const uint8_t* h_xy, uint32_t flags, sbn_bases** out) {
  if (!c || !out || (!G_xy && n)) return SBN_EINVAL;
  std::lock_guard<std::mutex> g(c->mu);
  hipSetDevice(c->device);
  const size_t tot = n + (h_xy ? 1 : 0);
  sbn_bases* b = new sbn_bases(); b->n = n; b->has_h = h_xy != nullptr;
  hipError_t e = hipMalloc(&b->d_pts, (tot ? tot : 1) * 64);
  if (e != hipSuccess) { delete b; return fail(c, SBN_ENOMEM, "hipMalloc bases: %s", hipGetErrorString(e)); }
  if (n) HIPCHK(c, hipMemcpyAsync(b->d_pts, G_xy, n * 64, hipMemcpyHostToDevice, c->stream));
  if (h_xy) HIPCHK(c, hipMemcpyAsync((uint8_t*)b->d_pts + n * 64, h_xy, 64, hipMemcpyHostToDevice, c->stream));
  if (tot) {
    if (!(flags & SBN_POINTS_MONT)) LAUNCH(c, "k_points_to_mont", k_points_to_mont, (unsigned)((tot + 255) / 256), 256, (const uint32_t*)b->d_pts, (uint32_t*)b->d_pts, tot);
    else LAUNCH(c, "k_points_to_mont", k_points_from_ark, (unsigned)((tot + 255) / 256), 256, (const uint32_t*)b->d_pts, (uint32_t*)b->d_pts, tot);     // ark-ff's R = 2^256 -> R = 2^261
  }
  LAUNCHCHK(c);
  HIPCHK(c, hipStreamSynchronize(c->stream));
  {
    std::vector<std::string> keys(tot);
    for (size_t j = 0; j < n; j++) keys[j].assign((const char*)G_xy + 64 * j, 64);
    if (h_xy) keys[n].assign((const char*)h_xy, 64);
    int rc = bases_build_dedupe(c, b, keys);
    if (rc) { sbn_bases_free(c, b); return rc; }
  }
  *out = b;
  return SBN_OK;
}
void sbn_bases_free(sbn_ctx* c, sbn_bases* b) {
  if (!b) return;
  if (c) { hipSetDevice(c->device); hipStreamSynchronize(c->stream); }     // nothing may still be reading the tables
  if (b->uniq) { sbn_bases_free(c, b->uniq); b->uniq = nullptr; }
  for (auto& kv : b->derived) sbn_bases_free(c, kv.second);
  b->derived.clear();
  for (void* p : {b->d_comb, b->d_csr_off, b->d_csr_cols, b->d_big, b->d_glv, b->d_pts}) if (p) hipFree(p);
  for (auto& kv : b->tables) hipFree(kv.second);
  delete b;
}
size_t sbn_bases_len(const sbn_bases* b) { return b ? b->n : 0; }
int sbn_bases_precompute(sbn_ctx* c, sbn_bases* b, size_t max_bytes, int* window_bits) {
  if (!c || !b) return SBN_EINVAL;
  std::lock_guard<std::mutex> g(c->mu);
  hipSetDevice(c->device);
  int rc = bases_build_comb(c, b->uniq ? b->uniq : b, max_bytes);
  if (rc) return rc;
  if (window_bits) *window_bits = (b->uniq ? b->uniq : b)->comb_c;
  return SBN_OK;
}

int sbn_msm_bases_dev(sbn_ctx* c, const sbn_bases* b, const void* d_scalars, size_t n, uint32_t flags, uint8_t out_xy[64], int* out_is_inf) {
  if (!c || !b || !out_xy || (!d_scalars && n)) return SBN_EINVAL;
  if (n > b->n + (b->has_h ? 1 : 0)) return fail(c, SBN_EINVAL, "msm: n=%zu exceeds the table (%zu)", n, b->n + (b->has_h ? 1 : 0));
  std::lock_guard<std::mutex> g(c->mu);
  hipSetDevice(c->device);
  if (n == 0) { memset(out_xy, 0, 64); if (out_is_inf) *out_is_inf = 1; return SBN_OK; }      // before any launch: a zero-size grid is an error
  const uint32_t* ds; int rc;
  if ((rc = canon_scalars_dev(c, d_scalars, n, flags, &ds))) return rc;
  return msm_device(c, ds, (const uint32_t*)b->d_pts, n, out_xy, out_is_inf, b);
}
int sbn_msm_bases(sbn_ctx* c, const sbn_bases* b, const uint8_t* scalars, size_t n, uint32_t flags, uint8_t out_xy[64], int* out_is_inf) {
  if (!c || !b || !out_xy || (!scalars && n)) return SBN_EINVAL;
  if (n > b->n + (b->has_h ? 1 : 0)) return fail(c, SBN_EINVAL, "msm: n=%zu exceeds the table (%zu)", n, b->n + (b->has_h ? 1 : 0));
  std::lock_guard<std::mutex> g(c->mu);
  hipSetDevice(c->device);
  if (n == 0) { memset(out_xy, 0, 64); if (out_is_inf) *out_is_inf = 1; return SBN_OK; }
  const uint32_t* ds; int rc;
  if ((rc = stage_scalars(c, scalars, n, flags, &ds))) return rc;
  return msm_device(c, ds, (const uint32_t*)b->d_pts, n, out_xy, out_is_inf, b);
}
int sbn_msm(sbn_ctx* c, const uint8_t* scalars, const uint8_t* points, size_t n, uint32_t flags, uint8_t out_xy[64], int* out_is_inf) {
  if (!c || !out_xy || ((!scalars || !points) && n)) return SBN_EINVAL;
  std::lock_guard<std::mutex> g(c->mu);
  hipSetDevice(c->device);
  if (n == 0) { memset(out_xy, 0, 64); if (out_is_inf) *out_is_inf = 1; return SBN_OK; }
  int rc; const uint32_t* ds;
  if ((rc = stage_scalars(c, scalars, n, flags, &ds))) return rc;
  if ((rc = ensure(c, c->stage_pts, n * 64))) return rc;
  HIPCHK(c, hipMemcpyAsync(c->stage_pts.p, points, n * 64, hipMemcpyHostToDevice, c->stream));
  if (!(flags & SBN_POINTS_MONT)) LAUNCH(c, "k_points_to_mont", k_points_to_mont, (unsigned)((n + 255) / 256), 256, (const uint32_t*)c->stage_pts.p, (uint32_t*)c->stage_pts.p, n);
  else LAUNCH(c, "k_points_to_mont", k_points_from_ark, (unsigned)((n + 255) / 256), 256, (const uint32_t*)c->stage_pts.p, (uint32_t*)c->stage_pts.p, n);
  return msm_device(c, ds, (const uint32_t*)c->stage_pts.p, n, out_xy, out_is_inf);
}

}  // extern "C"
// flags: SBN_SCALARS_MONT, or the private SBN_SCALARS_INTERNAL (sbn_commit_table: Z and the blinds are this library's table values).  The
// exported entry point below admits the public bit only.
static int commit_rows_dev_impl(sbn_ctx* c, const sbn_bases* b, const void* Z_dev, const void* blinds_dev, size_t L, size_t R, uint32_t flags, uint8_t* out_xy, uint8_t* out_inf) {
  if (!c || !b || (!out_xy && L) || (!Z_dev && L * R)) return SBN_EINVAL;
  if (R != b->n) return fail(c, SBN_EINVAL, "commit: gens_n.n (%zu) != row length (%zu)  [commitments.rs:146 assert_eq]", b->n, R);
  if (blinds_dev && !b->has_h) return fail(c, SBN_EINVAL, "commit: blinds given but the table has no h");
  if (L == 0) return SBN_OK;                     // before any launch: a zero-size grid is an error
  std::lock_guard<std::mutex> g(c->mu);
  hipSetDevice(c->device);
  const uint32_t* dZ = (const uint32_t*)Z_dev; const uint32_t* dB = (const uint32_t*)blinds_dev;
  if ((flags & SBN_SCALARS_INTERNAL) && b->uniq) {
    // this library's table over a generator set with merged duplicates (every set the reference derives): the merge pass reads each
    // scalar once anyway and converts on the way out — no separate pass over the matrix
    RowInfo ri; ri.mont_scalars = true;
    return commit_rows_device(c, b, dZ, dB, L, R, out_xy, out_inf, ri);
  }
  if (flags & (SBN_SCALARS_MONT | SBN_SCALARS_INTERNAL)) {
    // SBN_SCALARS_MONT: ark-ff's limbs (R = 2^256).  SBN_SCALARS_INTERNAL (sbn_commit_table): this library's tables (R = 2^261, lazy).
    int rc;
    if ((rc = ensure(c, c->scal_canon, (L * R + L) * 32))) return rc;
    uint32_t* o = (uint32_t*)c->scal_canon.p;
    const bool internal = (flags & SBN_SCALARS_INTERNAL) != 0;
    if (L * R) { if (internal) LAUNCH(c, "k_scalars_from_mont", k_scalars_from_internal, (unsigned)((L * R + 255) / 256), 256, dZ, o, L * R); else LAUNCH(c, "k_scalars_from_mont", k_scalars_from_mont, (unsigned)((L * R + 255) / 256), 256, dZ, o, L * R); }
    dZ = o;
    if (dB) {
      if (internal) LAUNCH(c, "k_scalars_from_mont", k_scalars_from_internal, (unsigned)((L + 255) / 256), 256, dB, o + 8 * L * R, L); else LAUNCH(c, "k_scalars_from_mont", k_scalars_from_mont, (unsigned)((L + 255) / 256), 256, dB, o + 8 * L * R, L);
      dB = o + 8 * L * R;
    }
  }
  return commit_rows_device(c, b, dZ, dB, L, R, out_xy, out_inf);
}
extern "C" {
int sbn_commit_rows_dev(sbn_ctx* c, const sbn_bases* b, const void* Z_dev, const void* blinds_dev, size_t L, size_t R, uint32_t flags, uint8_t* out_xy, uint8_t* out_inf) {
  if (c && (flags & ~SBN_SCALARS_MONT)) return fail(c, SBN_EINVAL, "commit: unknown flags %#x", flags);
  return commit_rows_dev_impl(c, b, Z_dev, blinds_dev, L, R, flags, out_xy, out_inf);
}
// Host-pointer variant.  A large matrix is cut into row chunks: while chunk i is being committed, chunk i+1 crosses PCIe
// into the other of two staging buffers (copy stream), so the 1 GiB of a keyless derefs commitment costs about
// max(transfer, compute) instead of their sum.  Rows are independent (hyrax.rs:259-261), so chunking cannot change results.
}  // extern "C"
// row i of the matrix lies at Z + i * row_stride bytes (row_stride = R * 32 for a dense matrix; a multiple of it when the caller
// commits every N-th row of a larger matrix: sbn_group_commit_rows)
static int commit_rows_host(sbn_ctx* c, const sbn_bases* b, const uint8_t* Z, size_t row_stride, const uint8_t* blinds, size_t L, size_t R, uint32_t flags, uint8_t* out_xy, uint8_t* out_inf) {
  if (!c || !b || (!out_xy && L) || (!Z && L * R)) return SBN_EINVAL;
  if (flags & ~SBN_SCALARS_MONT) return fail(c, SBN_EINVAL, "commit: unknown flags %#x", flags);
  if (R != b->n) return fail(c, SBN_EINVAL, "commit: gens_n.n (%zu) != row length (%zu)  [commitments.rs:146 assert_eq]", b->n, R);
  if (blinds && !b->has_h) return fail(c, SBN_EINVAL, "commit: blinds given but the table has no h");
  if (L == 0) return SBN_OK;
  std::lock_guard<std::mutex> g(c->mu);
  hipSetDevice(c->device);
  int rc;
  const size_t row_bytes = R * 32;
  size_t chunk = L;
  size_t chunk_mb = 128;   // measured on the 1 GiB derefs matrix: 64 MB 35.0 ms, 128 MB 28.8, 256 MB 29.4, 512 MB 32.4 (one shot: 40.9)
  if (const char* ec = getenv("SBN_COMMIT_CHUNK_MB")) { int v = atoi(ec); if (v >= 1 && v <= 4096) chunk_mb = (size_t)v; }
  size_t chunk_min_mb = 160;   // below this the matrix goes up in one piece
  if (const char* em = getenv("SBN_COMMIT_CHUNK_MIN_MB")) { int v = atoi(em); if (v >= 0 && v <= 1 << 20) chunk_min_mb = (size_t)v; }
  if (const char* eb = getenv("SBN_COMMIT_CHUNK_BYTES")) { long long v = atoll(eb); if (v >= 32) { chunk_min_mb = 0; chunk_mb = 0; chunk = std::max<size_t>(1, (size_t)v / std::max<size_t>(row_bytes, 1)); } }   // tests: force many small chunks
  if (chunk_mb && L * row_bytes > (chunk_min_mb << 20) && row_bytes) { chunk = (chunk_mb << 20) / row_bytes; if (chunk < 1) chunk = 1; }
  const size_t nchunks = (L + chunk - 1) / chunk;
  if (!c->copy_stream) HIPCHK(c, hipStreamCreateWithFlags(&c->copy_stream, hipStreamNonBlocking));
  if ((rc = ensure(c, c->out_rows, L * 65))) return rc;
  if ((rc = ensure_pin(c, std::max<size_t>(4096, L * 65)))) return rc;
  for (int k = 0; k < (nchunks > 1 ? 2 : 1); k++) if ((rc = ensure(c, c->zstage[k], chunk * row_bytes + 64))) return rc;
  const uint32_t* dB_all = nullptr;
  if (blinds) {
    if ((rc = ensure(c, c->stage_scal, L * 64))) return rc;
    HIPCHK(c, hipMemcpyAsync(c->stage_scal.p, blinds, L * 32, hipMemcpyHostToDevice, c->stream));
    if (flags & SBN_SCALARS_MONT) {
      uint32_t* o = (uint32_t*)c->stage_scal.p + 8 * L;
      LAUNCH(c, "k_scalars_from_mont", k_scalars_from_mont, (unsigned)((L + 255) / 256), 256, (const uint32_t*)c->stage_scal.p, o, L);
      dB_all = o;
    } else dB_all = (const uint32_t*)c->stage_scal.p;
  }
  if ((rc = input_check_begin(c))) return rc;
  hipEvent_t copied[2] = {nullptr, nullptr}, consumed[2] = {nullptr, nullptr};
  for (int k = 0; k < 2; k++) { copied[k] = evt_get(c); consumed[k] = evt_get(c); }
  uint32_t* d_xy = (uint32_t*)c->out_rows.p; uint8_t* d_inf = (uint8_t*)c->out_rows.p + L * 64;
  rc = SBN_OK;
  for (size_t i = 0; i < nchunks && rc == SBN_OK; i++) {
    const int k = (int)(i & 1);
    const size_t r0 = i * chunk, rows = std::min(chunk, L - r0);
    // the staging buffer is free again once the chunk that used it two iterations ago has been read by its first kernels
    if (i >= 2) { hipError_t e = hipStreamWaitEvent(c->copy_stream, consumed[k], 0); if (e != hipSuccess) { rc = fail(c, SBN_EHIP, "hipStreamWaitEvent: %s", hipGetErrorString(e)); break; } }
    hipError_t e = row_stride == row_bytes ? hipMemcpyAsync(c->zstage[k].p, Z + r0 * row_bytes, rows * row_bytes, hipMemcpyHostToDevice, c->copy_stream)
                                          : hipMemcpy2DAsync(c->zstage[k].p, row_bytes, Z + r0 * row_stride, row_stride, row_bytes, rows, hipMemcpyHostToDevice, c->copy_stream);
    if (e == hipSuccess) e = hipEventRecord(copied[k], c->copy_stream);
    if (e == hipSuccess) e = hipStreamWaitEvent(c->stream, copied[k], 0);
    if (e != hipSuccess) { rc = fail(c, SBN_EHIP, "chunk upload: %s", hipGetErrorString(e)); break; }
    const uint32_t* dZ = (const uint32_t*)c->zstage[k].p;
    if (flags & SBN_SCALARS_MONT) {
      if ((rc = ensure(c, c->scal_canon, chunk * row_bytes))) break;
      LAUNCH(c, "k_scalars_from_mont", k_scalars_from_mont, (unsigned)((rows * R + 255) / 256), 256, dZ, (uint32_t*)c->scal_canon.p, rows * R);
      hipEventRecord(consumed[k], c->stream);
      dZ = (const uint32_t*)c->scal_canon.p;
      c->z_consumed = nullptr;
    } else c->z_consumed = consumed[k];
    rc = commit_rows_launch(c, b, dZ, dB_all ? dB_all + 8 * r0 : nullptr, rows, R, d_xy + 16 * r0, d_inf + r0);
    c->z_consumed = nullptr;
  }
  if (rc == SBN_OK) {
    hipError_t e = hipMemcpyAsync(c->pin, c->out_rows.p, L * 65, hipMemcpyDeviceToHost, c->stream);
    if (e != hipSuccess) rc = fail(c, SBN_EHIP, "result download: %s", hipGetErrorString(e));
    if (rc == SBN_OK) rc = input_check_fetch(c);
  }
  hipStreamSynchronize(c->copy_stream);
  hipError_t es = hipStreamSynchronize(c->stream);
  if (rc == SBN_OK && es != hipSuccess) rc = fail(c, SBN_EHIP, "commit: %s", hipGetErrorString(es));
  for (int k = 0; k < 2; k++) { c->evt_pool.push_back(copied[k]); c->evt_pool.push_back(consumed[k]); }
  if (c->prof) prof_drain(c);
  if (rc) return rc;
  if ((rc = input_check_end(c))) return rc;
  memcpy(out_xy, c->pin, L * 64);
  if (out_inf) memcpy(out_inf, (uint8_t*)c->pin + L * 64, L);
  return SBN_OK;
}
extern "C" {
int sbn_commit_rows(sbn_ctx* c, const sbn_bases* b, const uint8_t* Z, const uint8_t* blinds, size_t L, size_t R, uint32_t flags, uint8_t* out_xy, uint8_t* out_inf) {
  return commit_rows_host(c, b, Z, R * 32, blinds, L, R, flags, out_xy, out_inf);
}

int sbn_g1_compress(const uint8_t* xy, size_t n, uint8_t* out32) {
  if ((!xy || !out32) && n) return SBN_EINVAL;
  for (size_t i = 0; i < n; i++) sbn_host::g1_compress(xy + 64 * i, out32 + 32 * i);
  return SBN_OK;
}
int sbn_g1_sum(const uint8_t* xy, size_t n, uint8_t out_xy[64], int* out_is_inf) {
  if (!out_xy || (!xy && n)) return SBN_EINVAL;
  sbn_host::Pt acc = sbn_host::inf();
  for (size_t i = 0; i < n; i++) {
    const uint8_t* p = xy + 64 * i;
    bool inf = true; for (int k = 0; k < 64; k++) if (p[k]) { inf = false; break; }
    if (inf) continue;
    sbn_host::Fq x, y; memcpy(x.v, p, 32); memcpy(y.v, p + 32, 32);
    if (sbn_host::geq_p(x.v) || sbn_host::geq_p(y.v)) return SBN_EINVAL;   // not canonical
    sbn_host::Pt q; q.X = sbn_host::to_mont(x); q.Y = sbn_host::to_mont(y); q.ZZ = sbn_host::one(); q.ZZZ = sbn_host::one();
    acc = sbn_host::padd(acc, q);
  }
  sbn_host::to_affine_bytes(acc, out_xy, out_is_inf);
  return SBN_OK;
}
static bool fr_load_canon(const uint8_t* b, sbn_host::fr::El* o) { memcpy(o->v, b, 32); return !sbn_host::fr::geq(o->v); }
int sbn_unipoly_from_evals(const uint8_t* evals, size_t n, uint8_t* coeffs) {
  using namespace sbn_host::fr;
  if (!evals || !coeffs || (n != 3 && n != 4)) return SBN_EINVAL;               // unipoly.rs:29 assert
  El e[4];
  for (size_t i = 0; i < n; i++) if (!fr_load_canon(evals + 32 * i, &e[i])) return SBN_EINVAL;
  const El two_inv = inv_small(2), six_inv = inv_small(6);
  if (n == 3) {
    // c = e0 ; a = (e2 - 2 e1 + e0)/2 ; b = e1 - c - a          (unipoly.rs:32-39)
    El c = e[0], a = mul(two_inv, add(sub(sub(e[2], e[1]), e[1]), c)), b = sub(sub(e[1], c), a);
    memcpy(coeffs, c.v, 32); memcpy(coeffs + 32, b.v, 32); memcpy(coeffs + 64, a.v, 32);
  } else {
    // d = e0 ; a = (e3 - 3 e2 + 3 e1 - e0)/6 ; b = (2 e0 - 5 e1 + 4 e2 - e3)/2 ; c = e1 - d - a - b     (unipoly.rs:41-56)
    El d = e[0];
    El a = mul(six_inv, sub(add(add(add(sub(sub(sub(e[3], e[2]), e[2]), e[2]), e[1]), e[1]), e[1]), e[0]));
    El t = add(e[0], e[0]); for (int k = 0; k < 5; k++) t = sub(t, e[1]); for (int k = 0; k < 4; k++) t = add(t, e[2]); t = sub(t, e[3]);
    El b = mul(two_inv, t), c = sub(sub(sub(e[1], d), a), b);
    memcpy(coeffs, d.v, 32); memcpy(coeffs + 32, c.v, 32); memcpy(coeffs + 64, b.v, 32); memcpy(coeffs + 96, a.v, 32);
  }
  return SBN_OK;
}
int sbn_unipoly_eval(const uint8_t* coeffs, size_t n, const uint8_t r[32], uint8_t out[32]) {
  using namespace sbn_host::fr;
  if (!coeffs || !r || !out || n == 0) return SBN_EINVAL;
  El rr, ev, pw, c;
  if (!fr_load_canon(r, &rr) || !fr_load_canon(coeffs, &ev)) return SBN_EINVAL;
  pw = rr;
  for (size_t i = 1; i < n; i++) { if (!fr_load_canon(coeffs + 32 * i, &c)) return SBN_EINVAL; ev = add(ev, mul(pw, c)); pw = mul(pw, rr); }   // unipoly.rs:74-82
  memcpy(out, ev.v, 32);
  return SBN_OK;
}
void sbn_factored_lens(size_t ell, size_t* left, size_t* right) { if (left) *left = ell / 2; if (right) *right = ell - ell / 2; }

// ---- generators: MultiCommitGens::new (commitments.rs:31-62) ----
// GroupElement::from_uniform_bytes (group.rs:110-131): the scalar s with point = s*G
static void uniform_bytes_scalar(const uint8_t ub[64], uint8_t s[32]) {
  sbn_host::sha3_256(ub, 64, s);
  if (fr_canonical(s)) return;                 // Scalar::from_bytes accepts only < r (scalar.rs:87-95)
  uint8_t tmp[72]; memcpy(tmp, "fallback", 8); memcpy(tmp + 8, ub, 64);
  sbn_host::sha3_256(tmp, 72, s);
  if (fr_canonical(s)) return;
  memset(s, 0, 32); s[0] = 1;                  // unwrap_or(Scalar::one())
}
int sbn_gens_new(sbn_ctx* c, size_t n, const uint8_t* label, size_t label_len, uint8_t* out_xy, sbn_bases** out) {
  if (!c || !out || (!label && label_len)) return SBN_EINVAL;
  std::lock_guard<std::mutex> g(c->mu);
  hipSetDevice(c->device);
  const size_t tot = n + 1;
  // SHAKE256(label || compressed generator); the generator (1,2) compresses to 01 00..00 (y = 2 is the smaller root)
  uint8_t gc[32] = {1};
  sbn_host::Keccak xof(136, 0x1f);
  xof.absorb(label, label_len); xof.absorb(gc, 32);
  std::vector<uint8_t> dl(tot * 32);
  for (size_t i = 0; i < tot; i++) { uint8_t ub[64]; xof.squeeze(ub, 64); uniform_bytes_scalar(ub, &dl[32 * i]); }
  int rc;
  if ((rc = ensure(c, c->gen_tmp, tot * (32 + 128)))) return rc;
  uint8_t* d_s = (uint8_t*)c->gen_tmp.p; uint8_t* d_x = d_s + tot * 32;
  HIPCHK(c, hipMemcpyAsync(d_s, dl.data(), tot * 32, hipMemcpyHostToDevice, c->stream));
  LAUNCH(c, "k_mul_generator", k_mul_generator, (unsigned)((tot + 63) / 64), 64, (const uint32_t*)d_s, tot, (uint32_t*)d_x);
  sbn_bases* b = new sbn_bases(); b->n = n; b->has_h = true;
  hipError_t e = hipMalloc(&b->d_pts, tot * 64);
  if (e != hipSuccess) { delete b; return fail(c, SBN_ENOMEM, "hipMalloc gens: %s", hipGetErrorString(e)); }
  uint32_t* d_xy = nullptr;
  if (out_xy) { if ((rc = ensure(c, c->out_small, tot * 64))) { hipFree(b->d_pts); delete b; return rc; } d_xy = (uint32_t*)c->out_small.p; }
  LAUNCH(c, "k_xyzz_to_affine", k_xyzz_to_affine, (unsigned)((tot + 63) / 64), 64, (const uint32_t*)d_x, (uint32_t*)b->d_pts, d_xy, (uint8_t*)nullptr, tot);
  LAUNCHCHK(c);
  if (out_xy) HIPCHK(c, hipMemcpyAsync(out_xy, d_xy, tot * 64, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  {
    std::vector<std::string> keys(tot);     // equal discrete logs <=> equal points
    for (size_t j = 0; j < tot; j++) keys[j].assign((const char*)&dl[32 * j], 32);
    if ((rc = bases_build_dedupe(c, b, keys))) { sbn_bases_free(c, b); return rc; }
  }
  *out = b;
  return SBN_OK;
}

int sbn_msm_jacobian(sbn_ctx* c, const uint8_t* scalars, const uint8_t* points_xyz, size_t n, uint32_t flags, uint8_t out_xy[64], int* out_is_inf) {
  if (!c || !out_xy || ((!scalars || !points_xyz) && n)) return SBN_EINVAL;
  std::lock_guard<std::mutex> g(c->mu);
  hipSetDevice(c->device);
  if (n == 0) { memset(out_xy, 0, 64); if (out_is_inf) *out_is_inf = 1; return SBN_OK; }
  int rc; const uint32_t* ds;
  if ((rc = stage_scalars(c, scalars, n, flags, &ds))) return rc;
  if ((rc = ensure(c, c->gen_tmp, n * 96))) return rc;
  if ((rc = ensure(c, c->stage_pts, n * 64))) return rc;
  HIPCHK(c, hipMemcpyAsync(c->gen_tmp.p, points_xyz, n * 96, hipMemcpyHostToDevice, c->stream));
  LAUNCH(c, "k_jacobian_to_affine", k_jacobian_to_affine, (unsigned)((n + 63) / 64), 64, (const uint32_t*)c->gen_tmp.p, (flags & SBN_POINTS_MONT) ? 1 : 0, n, (uint32_t*)c->stage_pts.p);
  return msm_device(c, ds, (const uint32_t*)c->stage_pts.p, n, out_xy, out_is_inf);
}
// device-side copy of a point range into a new handle (keys for the duplicate detection are read back once)
static int bases_from_device(sbn_ctx* c, const void* d_G, size_t n, const void* d_h, sbn_bases** out) {
  const size_t tot = n + (d_h ? 1 : 0);
  sbn_bases* b = new sbn_bases(); b->n = n; b->has_h = d_h != nullptr;
  hipError_t e = hipMalloc(&b->d_pts, (tot ? tot : 1) * 64);
  if (e != hipSuccess) { delete b; return fail(c, SBN_ENOMEM, "hipMalloc bases: %s", hipGetErrorString(e)); }
  if (n) HIPCHK(c, hipMemcpyAsync(b->d_pts, d_G, n * 64, hipMemcpyDeviceToDevice, c->stream));
  if (d_h) HIPCHK(c, hipMemcpyAsync((uint8_t*)b->d_pts + n * 64, d_h, 64, hipMemcpyDeviceToDevice, c->stream));
  std::vector<std::string> keys(tot);
  std::vector<uint8_t> host(tot * 64);
  if (tot) HIPCHK(c, hipMemcpyAsync(host.data(), b->d_pts, tot * 64, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  for (size_t j = 0; j < tot; j++) keys[j].assign((const char*)&host[64 * j], 64);
  int rc = bases_build_dedupe(c, b, keys);
  if (rc) { sbn_bases_free(c, b); return rc; }
  *out = b;
  return SBN_OK;
}
}  // extern "C"
// The generator sets the provers derive from a caller's handle, each built once and kept by that handle (sbn_bases::derived, released with it).
// A key is the kind byte, then what tells two sets of a kind apart (a bullet set's Q or nothing, a ZK set's gens_1 points): kinds never collide.
enum DerivedKind : char { DERIVED_BULLET = 1, DERIVED_POLYEVAL, DERIVED_ZK, DERIVED_R1CS_GENS_N, DERIVED_R1CS_GENS_1 };
static std::mutex g_derived_mu;      // guards every handle's `derived`; taken with the context's mutex held, never the other way round
// the set `owner` keeps under (kind, rest), built by build(&set) on the first call
template <class Build>
static int derived_set(const sbn_bases* owner, DerivedKind kind, const std::string& rest, Build build, const sbn_bases** out) {
  const std::string key = std::string(1, (char)kind) + rest;
  std::lock_guard<std::mutex> tg(g_derived_mu);
  for (auto& kv : owner->derived) if (kv.first == key) { *out = kv.second; return SBN_OK; }
  sbn_bases* set = nullptr;
  const int rc = build(&set);
  if (rc != SBN_OK) return rc;
  owner->derived.emplace_back(key, set);
  *out = set;
  return SBN_OK;
}
extern "C" {
int sbn_bases_split_at(sbn_ctx* c, const sbn_bases* b, size_t mid, sbn_bases** left, sbn_bases** right) {
  if (!c || !b || !left || !right || mid > b->n) return SBN_EINVAL;
  std::lock_guard<std::mutex> g(c->mu);
  hipSetDevice(c->device);
  const uint8_t* p = (const uint8_t*)b->d_pts; const void* h = b->has_h ? p + 64 * b->n : nullptr;
  int rc;
  if ((rc = bases_from_device(c, p, mid, h, left))) return rc;
  if ((rc = bases_from_device(c, p + 64 * mid, b->n - mid, h, right))) { sbn_bases_free(c, *left); *left = nullptr; return rc; }
  return SBN_OK;
}
int sbn_bases_scale(sbn_ctx* c, const sbn_bases* b, const uint8_t s[32], sbn_bases** out) {
  if (!c || !b || !s || !out) return SBN_EINVAL;
  if (!fr_canonical(s)) return fail(c, SBN_EINVAL, "scale: scalar not canonical");
  std::lock_guard<std::mutex> g(c->mu);
  hipSetDevice(c->device);
  int rc; const size_t n = b->n;
  if ((rc = ensure(c, c->gen_tmp, 64 + n * 128 + n * 64))) return rc;
  uint8_t* d_s = (uint8_t*)c->gen_tmp.p; uint8_t* d_x = d_s + 64; uint8_t* d_a = d_x + n * 128;
  HIPCHK(c, hipMemcpyAsync(d_s, s, 32, hipMemcpyHostToDevice, c->stream));
  if (n) {
    LAUNCH(c, "k_scale_points", k_scale_points, (unsigned)((n + 63) / 64), 64, (const uint32_t*)b->d_pts, n, (const uint32_t*)d_s, (uint32_t*)d_x);
    LAUNCH(c, "k_xyzz_to_affine", k_xyzz_to_affine, (unsigned)((n + 63) / 64), 64, (const uint32_t*)d_x, (uint32_t*)d_a, (uint32_t*)nullptr, (uint8_t*)nullptr, n);
  }
  LAUNCHCHK(c);
  return bases_from_device(c, d_a, n, b->has_h ? (const uint8_t*)b->d_pts + 64 * n : nullptr, out);
}
int sbn_bases_synthetic(sbn_ctx* c, size_t n, uint64_t first, const uint8_t s0[32], const uint8_t d[32], sbn_bases** out) {
  if (!c || !out || !s0 || !d || n == 0) return SBN_EINVAL;
  if (!fr_canonical(s0) || !fr_canonical(d)) return fail(c, SBN_EINVAL, "synthetic bases: s0/d not canonical");
  std::lock_guard<std::mutex> g(c->mu);
  hipSetDevice(c->device);
  int rc;
  if ((rc = ensure(c, c->gen_tmp, 64 + 256 + n * 128))) return rc;
  uint8_t* d_s = (uint8_t*)c->gen_tmp.p; uint8_t* d_p0d = d_s + 64; uint8_t* d_x = d_p0d + 256;
  HIPCHK(c, hipMemcpyAsync(d_s, s0, 32, hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemcpyAsync(d_s + 32, d, 32, hipMemcpyHostToDevice, c->stream));
  LAUNCH(c, "k_mul_generator", k_mul_generator, 1, 64, (const uint32_t*)d_s, (size_t)2, (uint32_t*)d_p0d);
  LAUNCH(c, "k_arith_points", k_arith_points, (unsigned)((n + 63) / 64), 64, (const uint32_t*)d_p0d, (unsigned long long)first, n, (uint32_t*)d_x);
  sbn_bases* b = new sbn_bases(); b->n = n; b->has_h = false;
  hipError_t e = hipMalloc(&b->d_pts, n * 64);
  if (e != hipSuccess) { delete b; return fail(c, SBN_ENOMEM, "hipMalloc synthetic bases: %s", hipGetErrorString(e)); }
  LAUNCH(c, "k_xyzz_to_affine", k_xyzz_to_affine, (unsigned)((n + 63) / 64), 64, (const uint32_t*)d_x, (uint32_t*)b->d_pts, (uint32_t*)nullptr, (uint8_t*)nullptr, n);
  LAUNCHCHK(c);
  HIPCHK(c, hipStreamSynchronize(c->stream));
  *out = b;
  return SBN_OK;
}
int sbn_scalars_synthetic(sbn_ctx* c, uint64_t seed, uint64_t first, size_t n, void* out_dev) {
  if (!c || (!out_dev && n)) return SBN_EINVAL;
  if (n == 0) return SBN_OK;
  std::lock_guard<std::mutex> g(c->mu);
  hipSetDevice(c->device);
  LAUNCH(c, "k_scalars_synthetic", k_scalars_synthetic, (unsigned)((n + 255) / 256), 256, (unsigned long long)seed, (unsigned long long)first, n, (uint32_t*)out_dev);
  LAUNCHCHK(c);
  HIPCHK(c, hipStreamSynchronize(c->stream));
  if (c->prof) prof_drain(c);
  return SBN_OK;
}
int sbn_bases_download(sbn_ctx* c, const sbn_bases* b, size_t first, size_t count, uint8_t* out_xy) {
  if (!c || !b || (!out_xy && count)) return SBN_EINVAL;
  const size_t tot = b->n + (b->has_h ? 1 : 0);
  if (first > tot || count > tot - first) return fail(c, SBN_EINVAL, "bases_download: range outside the table");
  if (count == 0) return SBN_OK;
  std::lock_guard<std::mutex> g(c->mu);
  hipSetDevice(c->device);
  int rc; if ((rc = ensure(c, c->stage_pts, count * 64))) return rc;
  LAUNCH(c, "k_points_from_mont", k_points_from_mont, (unsigned)((count + 255) / 256), 256, (const uint32_t*)b->d_pts + 16 * first, (uint32_t*)c->stage_pts.p, count);
  LAUNCHCHK(c);
  HIPCHK(c, hipMemcpyAsync(out_xy, c->stage_pts.p, count * 64, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return SBN_OK;
}

}  // extern "C"
