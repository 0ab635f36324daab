// abi_dense.inc — C ABI: MultiSparseMatPolynomialAsDense on the device (include/sbn254.h; reference src/sparse_mlpoly_full.rs:89-101, 120-174, 211-243).
// The host validates and uploads the triplets once; padded address arrays, timestamps and the two merged tables are made by dense_kernels.cuh.

struct sbn_dense {
  size_t batch = 0, N = 0, cells = 0;
  uint32_t log_n = 0;
  void* u32s = nullptr;          // row addr | row read_ts | col addr | col read_ts (batch * N each), then row audit_ts | col audit_ts (cells each)
  sbn_table ops, mem;            // comb_ops, comb_mem: owned by the handle (their buffers come from the context's pool)
};
static uint32_t* dense_addr(const sbn_dense* h, int side) { return (uint32_t*)h->u32s + (size_t)side * 2 * h->batch * h->N; }
static uint32_t* dense_read_ts(const sbn_dense* h, int side) { return dense_addr(h, side) + h->batch * h->N; }
static uint32_t* dense_audit(const sbn_dense* h, int side) { return (uint32_t*)h->u32s + 4 * h->batch * h->N + (size_t)side * h->cells; }

static void dense_release(sbn_ctx* c, sbn_dense* h) {
  if (h->u32s) hipFree(h->u32s);
  if (h->ops.d) pool_put(c, h->ops.d, h->ops.cap * 32);
  if (h->mem.d) pool_put(c, h->mem.d, h->mem.cap * 32);
  delete h;
}

// read_ts and audit_ts of one side: stable LSD radix sort of the batch * N addresses (payload: the op index), then run starts and ranks.  Enqueue only.
static void dense_timestamps(sbn_ctx* c, const sbn_dense* h, int side, uint32_t* key[2], uint32_t* idx[2], uint32_t* counts, uint32_t* sums, uint32_t* start) {
  const uint32_t n = (uint32_t)(h->batch * h->N), cells = (uint32_t)h->cells;
  const uint32_t ntiles = (n + DENSE_TILE - 1) / DENSE_TILE, nc = DENSE_BINS * ntiles, nchunks = (nc + DENSE_SCAN_CHUNK - 1) / DENSE_SCAN_CHUNK;
  uint32_t bits = 0; while (((size_t)1 << bits) < h->cells) bits++;
  // only the bits an address can have are sorted on, in equal passes of at most DENSE_RADIX_BITS (21 bits: 3 passes of 7)
  const uint32_t npass = std::max(1u, (bits + DENSE_RADIX_BITS - 1) / DENSE_RADIX_BITS), dbits = (bits + npass - 1) / npass;
  const uint32_t* kin = dense_addr(h, side); const uint32_t* iin = nullptr;
  int cur = 0;
  for (uint32_t p = 0; p < npass; p++) {
    const uint32_t shift = p * dbits, mask = (1u << dbits) - 1u;
    LAUNCH(c, "k_dense_hist", k_dense_hist, ntiles, DENSE_BLOCK, kin, n, shift, mask, ntiles, counts);
    LAUNCH(c, "k_dense_scan", k_dense_scan, nchunks, DENSE_BLOCK, counts, nc, sums);
    LAUNCH(c, "k_dense_scan_top", k_dense_scan_top, 1, DENSE_BLOCK, sums, nchunks);
    LAUNCH(c, "k_dense_scatter", k_dense_scatter, ntiles, DENSE_BLOCK, kin, iin, n, shift, mask, ntiles, (const uint32_t*)counts, (const uint32_t*)sums, key[cur], idx[cur]);
    kin = key[cur]; iin = idx[cur]; cur ^= 1;
  }
  hipMemsetAsync(dense_audit(h, side), 0, h->cells * 4, c->stream);
  LAUNCH(c, "k_dense_bounds", k_dense_bounds, stream_grid(n), 256, kin, n, cells, start);
  LAUNCH(c, "k_dense_rank", k_dense_rank, stream_grid(n), 256, kin, iin, n, cells, (const uint32_t*)start, dense_read_ts(h, side), dense_audit(h, side));
}

// the sort's share of the dense workspace for M = batch * N ops over `cells` cells
struct DenseWs { size_t b_m, b_cnt, b_sum, b_start, bytes; };
static DenseWs dense_ws_sizes(size_t M, size_t cells) {
  const uint32_t ntiles = (uint32_t)((M + DENSE_TILE - 1) / DENSE_TILE);
  const size_t nc = (size_t)DENSE_BINS * ntiles, nchunks = (nc + DENSE_SCAN_CHUNK - 1) / DENSE_SCAN_CHUNK;
  DenseWs w;
  w.b_m = r1cs_align(M * 4); w.b_cnt = r1cs_align(nc * 4); w.b_sum = r1cs_align(nchunks * 4); w.b_start = r1cs_align(cells * 4);
  w.bytes = 4 * w.b_m + w.b_cnt + w.b_sum + w.b_start;
  return w;
}
// sbn_dense_build behind its validation and its three copies: the triplets lie on the device already — rows_dev / cols_dev / vals_dev, matrix k's nnz[k]
// entries from a.off[k] on, canonical values (ark-ff's limbs under SBN_SCALARS_MONT), every address below `cells` — and are read, not kept.  The first
// ws_off bytes of the context's dense workspace are the caller's (the host entry point stages its copies there).  The caller holds the context's mutex;
// the call returns behind the stream, so what the triplets lie in is free again
static int dense_build_staged(sbn_ctx* c, const uint32_t* rows_dev, const uint32_t* cols_dev, const uint32_t* vals_dev, const DenseArgs& a, size_t batch, size_t N, size_t cells,
                              size_t ws_off, uint32_t flags, sbn_dense** out) {
  const size_t M = batch * N;
  size_t ops_len = 1; while (ops_len < 5 * M) ops_len <<= 1;    // DensePolynomial::merge pads to the next power of two (hyrax.rs:237-251)
  const size_t mem_len = 2 * cells;
  sbn_dense* h = new sbn_dense();
  h->batch = batch; h->N = N; h->cells = cells; h->log_n = r1cs_log2(N);
  h->ops.owned = h->mem.owned = false;                          // a stray sbn_table_free must not recycle the handle's buffers
  size_t got = 0;
  hipError_t e = pool_get(c, ops_len * 32, &h->ops.d, &got);
  if (e != hipSuccess) { (void)hipGetLastError(); h->ops.d = nullptr; dense_release(c, h); return fail(c, SBN_ENOMEM, "dense_build: comb_ops (%zu entries, %zu bytes): %s", ops_len, ops_len * 32, hipGetErrorString(e)); }
  h->ops.len = ops_len; h->ops.cap = got / 32;
  e = pool_get(c, mem_len * 32, &h->mem.d, &got);
  if (e != hipSuccess) { (void)hipGetLastError(); h->mem.d = nullptr; dense_release(c, h); return fail(c, SBN_ENOMEM, "dense_build: comb_mem (%zu entries): %s", mem_len, hipGetErrorString(e)); }
  h->mem.len = mem_len; h->mem.cap = got / 32;
  e = hipMalloc(&h->u32s, (4 * M + 2 * cells) * 4);
  if (e != hipSuccess) { (void)hipGetLastError(); h->u32s = nullptr; dense_release(c, h); return fail(c, SBN_ENOMEM, "dense_build: address and timestamp arrays (%zu bytes): %s", (4 * M + 2 * cells) * 4, hipGetErrorString(e)); }

  // workspace behind the caller's part: two (key, index) buffers of the sort, its counts and chunk sums, the run starts
  const DenseWs w = dense_ws_sizes(M, cells);
  int rc = ensure(c, c->dense_ws, ws_off + w.bytes);
  if (rc) { dense_release(c, h); return rc; }
  uint8_t* p = (uint8_t*)c->dense_ws.p + ws_off;
  uint32_t *key[2], *idx[2];
  key[0] = (uint32_t*)p; p += w.b_m; key[1] = (uint32_t*)p; p += w.b_m; idx[0] = (uint32_t*)p; p += w.b_m; idx[1] = (uint32_t*)p; p += w.b_m;
  uint32_t* counts = (uint32_t*)p; p += w.b_cnt;
  uint32_t* sums = (uint32_t*)p; p += w.b_sum;
  uint32_t* start = (uint32_t*)p;

  LAUNCH(c, "k_dense_expand", k_dense_expand, stream_grid(M), 256, rows_dev, cols_dev, a, h->log_n, (uint32_t)M, dense_addr(h, 0), dense_addr(h, 1));
  for (int side = 0; side < 2; side++) dense_timestamps(c, h, side, key, idx, counts, sums, start);
  LAUNCH(c, "k_dense_tables", k_dense_tables, stream_grid(ops_len + mem_len), 256, (const uint32_t*)h->u32s, vals_dev, a, h->log_n, (uint32_t)batch,
         (flags & SBN_SCALARS_MONT) ? 1 : 0, (const uint32_t*)dense_audit(h, 0), ops_len, mem_len, (uint32_t*)h->ops.d, (uint32_t*)h->mem.d);
  const hipError_t ce = hipGetLastError();
  const hipError_t se = hipStreamSynchronize(c->stream);        // the triplets and the staged copies are free again from here
  if (c->prof) prof_drain(c);
  if (ce != hipSuccess || se != hipSuccess) {
    dense_release(c, h);
    return fail(c, SBN_EHIP, "dense_build: %s", hipGetErrorString(ce != hipSuccess ? ce : se));
  }
  *out = h;
  return SBN_OK;
}

extern "C" {

void sbn_dense_free(sbn_ctx* c, sbn_dense* h) {
  if (!h) return;
  std::unique_lock<std::mutex> g;
  if (c) { g = std::unique_lock<std::mutex>(c->mu); hipSetDevice(c->device); hipStreamSynchronize(c->stream); }
  dense_release(c, h);
}
size_t sbn_dense_num_ops(const sbn_dense* h) { return h ? h->N : 0; }
size_t sbn_dense_num_cells(const sbn_dense* h) { return h ? h->cells : 0; }
size_t sbn_dense_batch(const sbn_dense* h) { return h ? h->batch : 0; }
const void* sbn_dense_addr_dev(const sbn_dense* h, int side, size_t k) { return (h && (side == 0 || side == 1) && k < h->batch) ? dense_addr(h, side) + k * h->N : nullptr; }
const void* sbn_dense_read_ts_dev(const sbn_dense* h, int side, size_t k) { return (h && (side == 0 || side == 1) && k < h->batch) ? dense_read_ts(h, side) + k * h->N : nullptr; }
const void* sbn_dense_audit_ts_dev(const sbn_dense* h, int side) { return (h && (side == 0 || side == 1)) ? dense_audit(h, side) : nullptr; }
const sbn_table* sbn_dense_comb_ops(const sbn_dense* h) { return h ? &h->ops : nullptr; }
const sbn_table* sbn_dense_comb_mem(const sbn_dense* h) { return h ? &h->mem : nullptr; }

int sbn_dense_build(sbn_ctx* c, size_t num_vars_x, size_t num_vars_y, const uint32_t* const* rows, const uint32_t* const* cols, const uint8_t* const* vals,
                    const size_t* nnz, size_t batch, uint32_t flags, sbn_dense** out) {
  if (!c || !out) return SBN_EINVAL;
  *out = nullptr;
  if (batch < 1 || batch > (size_t)DENSE_MAX_BATCH) return fail(c, SBN_EINVAL, "dense_build: batch=%zu (1 to %d matrices)", batch, DENSE_MAX_BATCH);
  if (!rows || !cols || !vals || !nnz) return fail(c, SBN_EINVAL, "dense_build: NULL argument");
  const size_t bits = std::max(num_vars_x, num_vars_y);
  if (bits > 31) return fail(c, SBN_EINVAL, "dense_build: num_vars_x=%zu, num_vars_y=%zu (addresses are 32-bit: at most 31 variables)", num_vars_x, num_vars_y);
  const size_t cells = (size_t)1 << bits;                       // sparse_mlpoly_full.rs:145-149
  size_t N = 1, total = 0;                                      // N = max next_power_of_two(nnz[k]), next_power_of_two(0) = 1
  for (size_t k = 0; k < batch; k++) {
    if (nnz[k] && (!rows[k] || !cols[k] || !vals[k])) return fail(c, SBN_EINVAL, "dense_build: matrix %zu has %zu entries and a NULL array", k, nnz[k]);
    if (nnz[k] > ((size_t)1 << 31)) return fail(c, SBN_EINVAL, "dense_build: matrix %zu has %zu entries: batch * N exceeds 2^31 (timestamps are 32-bit)", k, nnz[k]);
    while (N < nnz[k]) N <<= 1;
    total += nnz[k];
  }
  if (batch * N > ((size_t)1 << 31)) return fail(c, SBN_EINVAL, "dense_build: batch * N = %zu * %zu exceeds 2^31 (timestamps are 32-bit)", batch, N);
  for (size_t k = 0; k < batch; k++)
    for (size_t e = 0; e < nnz[k]; e++) {
      // AddrTimestamps::new asserts addr < num_cells (sparse_mlpoly_full.rs:226)
      if (rows[k][e] >= cells) return fail(c, SBN_EINVAL, "dense_build: matrix %zu entry %zu: row %u >= num_cells %zu", k, e, rows[k][e], cells);
      if (cols[k][e] >= cells) return fail(c, SBN_EINVAL, "dense_build: matrix %zu entry %zu: col %u >= num_cells %zu", k, e, cols[k][e], cells);
      if (!fr_canonical(vals[k] + 32 * e)) return fail(c, SBN_EINVAL, "dense_build: matrix %zu entry %zu: value >= r", k, e);
    }
  const size_t M = batch * N;

  std::lock_guard<std::mutex> g(c->mu);
  hipSetDevice(c->device);
  // workspace: the staged triplets, then what dense_build_staged takes behind them
  const size_t b_idx = r1cs_align(std::max<size_t>(total, 1) * 4), b_val = r1cs_align(std::max<size_t>(total, 1) * 32);
  const size_t staged = b_val + 2 * b_idx;
  int rc = ensure(c, c->dense_ws, staged + dense_ws_sizes(M, cells).bytes);
  if (rc) return rc;
  uint8_t* w = (uint8_t*)c->dense_ws.p;
  uint32_t* s_val = (uint32_t*)w; w += b_val;
  uint32_t* s_row = (uint32_t*)w; w += b_idx;
  uint32_t* s_col = (uint32_t*)w;

  DenseArgs a; memset(&a, 0, sizeof a);
  hipError_t ce = hipSuccess;
  size_t off = 0;
  for (size_t k = 0; k < batch && ce == hipSuccess; k++) {
    a.off[k] = (uint32_t)off; a.nnz[k] = (uint32_t)nnz[k];
    if (nnz[k]) {
      ce = hipMemcpyAsync(s_row + off, rows[k], nnz[k] * 4, hipMemcpyHostToDevice, c->stream);
      if (ce == hipSuccess) ce = hipMemcpyAsync(s_col + off, cols[k], nnz[k] * 4, hipMemcpyHostToDevice, c->stream);
      if (ce == hipSuccess) ce = hipMemcpyAsync(s_val + 8 * off, vals[k], nnz[k] * 32, hipMemcpyHostToDevice, c->stream);
    }
    off += nnz[k];
  }
  if (ce != hipSuccess) {
    hipStreamSynchronize(c->stream);                            // the caller's arrays are free again from here
    return fail(c, SBN_EHIP, "dense_build: %s", hipGetErrorString(ce));
  }
  return dense_build_staged(c, s_row, s_col, s_val, a, batch, N, cells, staged, flags, out);
}

}  // extern "C"
