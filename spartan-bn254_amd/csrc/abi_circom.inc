// abi_circom.inc — C ABI: circom's .r1cs and .wtns files straight onto the device (include/sbn254.h; reference src/r1cs_reader.rs, examples/keyless_benchmark.rs:38-72).
// The host scans the sections and walks the 3 * nConstraints entry counts (circom_host.hpp); the section's payload goes up in ONE copy and everything per
// entry is circom_kernels.cuh's:
//   load          k_circom_entries (the record, the value against r, remap_col) into per-matrix (row, col, canonical value) arrays in file order; ONE host wait
//                 for the drop counts and the bad-wire flag; where a value was dropped (never in a file circom wrote) k_dense_scan / _scan_top over the
//                 keep flags and k_circom_compact, and a second wait
//   from_circom   r1cs_from_staged: the handle of sbn_r1cs_upload without the host's two counting sorts — row-major [A; B; C] is the staged order itself
//                 (the file is in constraint order): k_circom_gkeys, k_circom_ends, two copies; column-major: the radix passes of dense_kernels.cuh on
//                 (column, position), k_circom_ends, k_circom_gather; then the tail both routes share (r1cs_csr_finish)
//   encode        sbn_snark_encode from sbn_r1cs_upload on, with r1cs_from_staged and dense_build_staged on the staged arrays
//   wtns          the value section in one copy, k_circom_wtns: the test against r and the vars table
//   digest        the library's own circuit digest (circom_host.hpp: the definition): k_circom_digest_leaves, one lane a leaf of 128 staged entries, the
//                 leaves brought back behind ONE host wait, the root one SHAKE256 over them on the host
// A handle made from a sbn_circom_r1cs copies what it keeps: the parsed circuit may be freed right after.  Included by sbn254.hip behind abi_nizk.inc.

struct sbn_circom_r1cs {
  sbn_host::circom::R1csScan scan;
  sbn_host::snark::Shape sh;
  size_t nnz[3] = {0, 0, 0}, dropped[3] = {0, 0, 0}, off[3] = {0, 0, 0};      // kept entries per matrix and where they start
  size_t total = 0;                                                           // nnz[0] + nnz[1] + nnz[2]
  void* mem = nullptr;
  uint32_t *rows = nullptr, *cols = nullptr, *vals = nullptr;                 // total entries each (vals: 8 words an entry, canonical)
};

// rows | cols | vals of `n` entries in one allocation
static int circom_alloc(sbn_ctx* c, size_t n, void** mem, uint32_t** rows, uint32_t** cols, uint32_t** vals) {
  const size_t b_idx = r1cs_align(std::max<size_t>(n, 1) * 4), b_val = r1cs_align(std::max<size_t>(n, 1) * 32);
  const hipError_t e = hipMalloc(mem, 2 * b_idx + b_val);
  if (e != hipSuccess) { (void)hipGetLastError(); *mem = nullptr; return fail(c, SBN_ENOMEM, "circom r1cs: hipMalloc (%zu entries): %s", n, hipGetErrorString(e)); }
  uint8_t* p = (uint8_t*)*mem;
  *vals = (uint32_t*)p; *rows = (uint32_t*)(p + b_val); *cols = (uint32_t*)(p + b_val + b_idx);
  return SBN_OK;
}

// the two compressed copies of sbn_r1cs_upload from the staged arrays.  Enqueue only; the caller holds the context's mutex and waits for the stream
static int r1cs_from_staged(sbn_ctx* c, const sbn_circom_r1cs* f, sbn_r1cs* h) {
  const size_t nc = f->sh.nc, nv = f->sh.nv, nr = 3 * nc, nz = 2 * nv, K = f->total;
  h->nc = nc; h->nv = nv; h->log_nc = r1cs_log2(nc); h->log_z = r1cs_log2(nz);
  for (int m = 0; m < 3; m++) h->nnz[m] = f->nnz[m];                        // (a remapped column is below 2 num_vars: nothing is dropped here)
  int rc;
  if ((rc = r1cs_csr_alloc(c, h->rowm, nr, K))) return rc;
  if ((rc = r1cs_csr_alloc(c, h->colm, nz, K))) return rc;
  // workspace: gkey, the sort's two (key, index) buffers, its counts and chunk sums
  const uint32_t ntiles = (uint32_t)((K + DENSE_TILE - 1) / DENSE_TILE);
  const size_t ncnt = (size_t)DENSE_BINS * std::max(ntiles, 1u), nchunks = (ncnt + DENSE_SCAN_CHUNK - 1) / DENSE_SCAN_CHUNK;
  const size_t b_k = r1cs_align(std::max<size_t>(K, 1) * 4), b_cnt = r1cs_align(ncnt * 4), b_sum = r1cs_align(nchunks * 4);
  if ((rc = ensure(c, c->dense_ws, 5 * b_k + b_cnt + b_sum))) return rc;
  uint8_t* w = (uint8_t*)c->dense_ws.p;
  uint32_t* gkey = (uint32_t*)w; w += b_k;
  uint32_t *key[2], *idx[2];
  key[0] = (uint32_t*)w; w += b_k; key[1] = (uint32_t*)w; w += b_k; idx[0] = (uint32_t*)w; w += b_k; idx[1] = (uint32_t*)w; w += b_k;
  uint32_t* counts = (uint32_t*)w; w += b_cnt;
  uint32_t* sums = (uint32_t*)w;
  const uint32_t n = (uint32_t)K;
  const uint32_t* sorted_cols = f->cols;                                      // (never read where n = 0)
  if (n) {
    LAUNCH(c, "k_circom_gkeys", k_circom_gkeys, stream_grid(n), 256, (const uint32_t*)f->rows, n, (uint32_t)f->off[1], (uint32_t)f->off[2], (uint32_t)nc, gkey);
    // row-major: the staged order is [A; B; C] by constraint already
    HIPCHK(c, hipMemcpyAsync(h->rowm.idx, f->cols, K * 4, hipMemcpyDeviceToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(h->rowm.val, f->vals, K * 32, hipMemcpyDeviceToDevice, c->stream));
    // column-major: stable by column, over the bits a column can have, in equal passes of at most DENSE_RADIX_BITS (as dense_timestamps)
    const uint32_t bits = h->log_z;
    const uint32_t npass = std::max(1u, (bits + DENSE_RADIX_BITS - 1) / DENSE_RADIX_BITS), dbits = (bits + npass - 1) / npass;
    const uint32_t* kin = f->cols; const uint32_t* iin = nullptr;
    int cur = 0;
    for (uint32_t p = 0; p < npass; p++) {
      const uint32_t shift = p * dbits, mask = (1u << dbits) - 1u;
      LAUNCH(c, "k_dense_hist", k_dense_hist, ntiles, DENSE_BLOCK, kin, n, shift, mask, ntiles, counts);
      LAUNCH(c, "k_dense_scan", k_dense_scan, (unsigned)nchunks, DENSE_BLOCK, counts, (uint32_t)ncnt, sums);
      LAUNCH(c, "k_dense_scan_top", k_dense_scan_top, 1, DENSE_BLOCK, sums, (uint32_t)nchunks);
      LAUNCH(c, "k_dense_scatter", k_dense_scatter, ntiles, DENSE_BLOCK, kin, iin, n, shift, mask, ntiles, (const uint32_t*)counts, (const uint32_t*)sums, key[cur], idx[cur]);
      kin = key[cur]; iin = idx[cur]; cur ^= 1;
    }
    sorted_cols = kin;
    LAUNCH(c, "k_circom_gather", k_circom_gather, stream_grid(n), 256, iin, (const uint32_t*)gkey, (const uint32_t*)f->vals, n, h->colm.idx, h->colm.val);
  }
  LAUNCH(c, "k_circom_ends", k_circom_ends, stream_grid(nr), 256, (const uint32_t*)gkey, n, (uint32_t)nr, h->rowm.row_end);
  LAUNCH(c, "k_circom_ends", k_circom_ends, stream_grid(nz), 256, sorted_cols, n, (uint32_t)nz, h->colm.row_end);
  LAUNCHCHK(c);
  if ((rc = r1cs_csr_finish(c, h->rowm, 0))) return rc;
  return r1cs_csr_finish(c, h->colm, 0);
}

// a resident sbn_r1cs from the parsed circuit; the caller holds the mutex.  Returns behind the stream
static int r1cs_from_circom_locked(sbn_ctx* c, const sbn_circom_r1cs* f, sbn_r1cs** out) {
  sbn_r1cs* h = new sbn_r1cs();
  int rc = r1cs_from_staged(c, f, h);
  const hipError_t se = hipStreamSynchronize(c->stream);
  if (c->prof) prof_drain(c);
  if (rc == SBN_OK && se != hipSuccess) rc = fail(c, SBN_EHIP, "r1cs_from_circom: %s", hipGetErrorString(se));
  if (rc) {
    if (h->rowm.mem) hipFree(h->rowm.mem);
    if (h->colm.mem) hipFree(h->colm.mem);
    delete h;
    return rc;
  }
  *out = h;
  return SBN_OK;
}

extern "C" {

void sbn_circom_r1cs_free(sbn_ctx* c, sbn_circom_r1cs* f) {
  if (!f) return;
  if (c) { std::lock_guard<std::mutex> g(c->mu); hipSetDevice(c->device); hipStreamSynchronize(c->stream); }
  if (f->mem) hipFree(f->mem);
  delete f;
}

int sbn_circom_r1cs_load(sbn_ctx* c, const uint8_t* file, size_t len, sbn_circom_r1cs** out) {
  if (!c || !file || !out) return SBN_EINVAL;
  *out = nullptr;
  namespace cf = sbn_host::circom;
  std::unique_ptr<sbn_circom_r1cs> f(new sbn_circom_r1cs());
  int e = cf::r1cs_scan(file, len, &f->scan);
  if (e) return fail(c, SBN_EINVAL, "circom r1cs: the file is refused: %s", cf::why(e));
  const cf::R1csScan& s = f->scan;
  std::vector<uint32_t> run_first, mat_first;
  uint64_t cnt[3];
  if ((e = cf::r1cs_walk(file, s, run_first, mat_first, cnt))) return fail(c, SBN_EINVAL, "circom r1cs: the file is refused: %s", cf::why(e));
  if (!cf::shape_of(s, &f->sh)) return fail(c, SBN_EINVAL, "circom r1cs: %llu constraints x %llu wires is too large", (unsigned long long)s.n_cons, (unsigned long long)s.n_wires);
  const size_t nruns = mat_first.size(), total = run_first[nruns];
  const size_t words = (s.payload_len + 3) / 4;

  std::lock_guard<std::mutex> g(c->mu);
  hipSetDevice(c->device);
  int rc;
  uint32_t *rows = nullptr, *cols = nullptr, *vals = nullptr; void* mem = nullptr;
  if ((rc = circom_alloc(c, total, &mem, &rows, &cols, &vals))) return rc;
  auto drop = [&](int code) { hipStreamSynchronize(c->stream); if (mem) hipFree(mem); return code; };
  // workspace: flags | payload | run_first | mat_first | keep | its scan | the scan's chunk sums
  const size_t nchunks = (total + DENSE_SCAN_CHUNK - 1) / DENSE_SCAN_CHUNK;
  const size_t b_pay = r1cs_align(words * 4 + 4), b_rf = r1cs_align((nruns + 1) * 4), b_mf = r1cs_align(std::max<size_t>(nruns, 1) * 4);
  const size_t b_keep = r1cs_align(std::max<size_t>(total, 1) * 4), b_sum = r1cs_align(std::max<size_t>(nchunks, 1) * 4);
  if ((rc = ensure(c, c->dense_ws, 256 + b_pay + b_rf + b_mf + 2 * b_keep + b_sum))) return drop(rc);
  if ((rc = ensure_pin(c, 4096))) return drop(rc);
  uint8_t* w = (uint8_t*)c->dense_ws.p;
  uint32_t* flags = (uint32_t*)w; w += 256;
  uint32_t* d_pay = (uint32_t*)w; w += b_pay;
  uint32_t* d_rf = (uint32_t*)w; w += b_rf;
  uint32_t* d_mf = (uint32_t*)w; w += b_mf;
  uint32_t* d_keep = (uint32_t*)w; w += b_keep;
  uint32_t* d_scan = (uint32_t*)w; w += b_keep;
  uint32_t* d_sums = (uint32_t*)w;
  static const uint32_t FLAGS0[4] = {0, 0, 0, 0xffffffffu};
  hipError_t ce = hipMemcpyAsync(flags, FLAGS0, 16, hipMemcpyHostToDevice, c->stream);
  if (total) {
    if (ce == hipSuccess) ce = hipMemsetAsync((uint8_t*)d_pay + (words - 1) * 4, 0, 4, c->stream);      // the last dword's bytes behind an odd section size
    if (ce == hipSuccess) ce = hipMemcpyAsync(d_pay, file + s.payload_off, s.payload_len, hipMemcpyHostToDevice, c->stream);
    if (ce == hipSuccess) ce = hipMemcpyAsync(d_rf, run_first.data(), (nruns + 1) * 4, hipMemcpyHostToDevice, c->stream);
    if (ce == hipSuccess) ce = hipMemcpyAsync(d_mf, mat_first.data(), nruns * 4, hipMemcpyHostToDevice, c->stream);
    if (ce == hipSuccess) {
      CircomArgs a;
      a.n_pub = (uint32_t)s.n_pub; a.n_wires = (uint32_t)s.n_wires; a.nv_padded = (uint32_t)f->sh.nv;
      a.mat_off[0] = 0; a.mat_off[1] = (uint32_t)cnt[0]; a.mat_off[2] = (uint32_t)(cnt[0] + cnt[1]);
      LAUNCH(c, "k_circom_entries", k_circom_entries, stream_grid(total), 256, (const uint32_t*)d_pay, words, (const uint32_t*)d_rf, (const uint32_t*)d_mf, (uint32_t)nruns,
             (uint32_t)total, a, rows, cols, vals, d_keep, flags);
      ce = hipGetLastError();
    }
  }
  if (ce == hipSuccess) ce = hipMemcpyAsync(c->pin, flags, 16, hipMemcpyDeviceToHost, c->stream);
  if (ce == hipSuccess) ce = hipStreamSynchronize(c->stream);                 // the one wait: the file's bytes and the two prefix arrays are free again
  if (c->prof) prof_drain(c);
  if (ce != hipSuccess) return drop(fail(c, SBN_EHIP, "circom r1cs: %s", hipGetErrorString(ce)));
  uint32_t got[4]; memcpy(got, c->pin, 16);
  if (got[3] != 0xffffffffu) {
    // which run the entry lies in: the host's own prefix array
    const size_t k = (size_t)(std::upper_bound(run_first.begin(), run_first.end(), got[3]) - run_first.begin()) - 1;
    return drop(fail(c, SBN_EINVAL, "circom r1cs: entry %u of the file (matrix %c, constraint %zu, entry %u of its run): wire >= nWires = %llu", got[3], "ABC"[k % 3], k / 3,
                     got[3] - run_first[k], (unsigned long long)s.n_wires));
  }
  size_t kept = 0;
  for (int m = 0; m < 3; m++) { f->dropped[m] = got[m]; f->nnz[m] = (size_t)cnt[m] - got[m]; f->off[m] = kept; kept += f->nnz[m]; }
  f->total = kept;
  if (kept != total) {                                                        // values >= r: close the gaps, in order
    uint32_t *r2 = nullptr, *c2 = nullptr, *v2 = nullptr; void* mem2 = nullptr;
    if ((rc = circom_alloc(c, kept, &mem2, &r2, &c2, &v2))) return drop(rc);
    ce = hipMemcpyAsync(d_scan, d_keep, total * 4, hipMemcpyDeviceToDevice, c->stream);
    if (ce == hipSuccess) {
      LAUNCH(c, "k_dense_scan", k_dense_scan, (unsigned)nchunks, DENSE_BLOCK, d_scan, (uint32_t)total, d_sums);
      LAUNCH(c, "k_dense_scan_top", k_dense_scan_top, 1, DENSE_BLOCK, d_sums, (uint32_t)nchunks);
      LAUNCH(c, "k_circom_compact", k_circom_compact, stream_grid(total), 256, (const uint32_t*)d_keep, (const uint32_t*)d_scan, (const uint32_t*)d_sums, (uint32_t)total,
             (uint32_t)kept, (const uint32_t*)rows, (const uint32_t*)cols, (const uint32_t*)vals, r2, c2, v2);
      ce = hipGetLastError();
    }
    if (ce == hipSuccess) ce = hipStreamSynchronize(c->stream);
    if (c->prof) prof_drain(c);
    hipFree(mem);
    mem = mem2; rows = r2; cols = c2; vals = v2;
    if (ce != hipSuccess) return drop(fail(c, SBN_EHIP, "circom r1cs: %s", hipGetErrorString(ce)));
  }
  f->mem = mem; f->rows = rows; f->cols = cols; f->vals = vals;
  *out = f.release();
  return SBN_OK;
}

int sbn_circom_r1cs_info(const sbn_circom_r1cs* f, sbn_circom_info* out) {
  if (!f || !out) return SBN_EINVAL;
  out->num_constraints = f->scan.n_cons; out->num_variables = f->scan.n_wires; out->num_pub_inputs = f->scan.n_pub; out->num_prv_inputs = f->scan.n_prv_in;
  out->num_labels = f->scan.n_labels;
  for (int m = 0; m < 3; m++) { out->nnz[m] = f->nnz[m]; out->dropped[m] = f->dropped[m]; }
  out->num_vars = f->sh.num_vars; out->num_cons_padded = f->sh.nc; out->num_vars_padded = f->sh.nv;
  return SBN_OK;
}

int sbn_circom_r1cs_download(sbn_ctx* c, const sbn_circom_r1cs* f, int m, uint32_t* rows, uint32_t* cols, uint8_t* vals) {
  if (!c || !f) return SBN_EINVAL;
  if (m < 0 || m > 2) return fail(c, SBN_EINVAL, "circom download: matrix %d (0, 1 or 2)", m);
  const size_t n = f->nnz[m], o = f->off[m];
  if (n && (!rows || !cols || !vals)) return fail(c, SBN_EINVAL, "circom download: matrix %d has %zu entries and a NULL array", m, n);
  if (!n) return SBN_OK;
  std::lock_guard<std::mutex> g(c->mu);
  hipSetDevice(c->device);
  HIPCHK(c, hipMemcpyAsync(rows, f->rows + o, n * 4, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipMemcpyAsync(cols, f->cols + o, n * 4, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipMemcpyAsync(vals, f->vals + 8 * o, n * 32, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return SBN_OK;
}

int sbn_circom_r1cs_digest(sbn_ctx* c, const sbn_circom_r1cs* f, uint8_t out[32]) {
  if (!c || !f || !out) return SBN_EINVAL;
  namespace cf = sbn_host::circom;
  CircomDigestArgs a; memset(&a, 0, sizeof a);
  {
    uint8_t head[28]; memset(head, 0, sizeof head);                             // the zero byte in front, the domain string, a zero byte where m goes
    static_assert(sizeof cf::DIGEST_LEAF_DOMAIN - 1 == 26, "the leaf header is 39 bytes: k_circom_digest_leaves' word stream depends on it");
    memcpy(head + 1, cf::DIGEST_LEAF_DOMAIN, 26);
    memcpy(a.head, head, 28);
  }
  size_t first[3], leaves = 0;
  for (int m = 0; m < 3; m++) {
    // what the kernel's two guards rest on: a lane that met one would leave its 32 bytes unwritten, and the root would hash what lay there before
    if (f->off[m] + f->nnz[m] > f->total || f->total > UINT32_MAX) return fail(c, SBN_EINVAL, "circom digest: matrix %d holds entries %zu .. %zu of %zu", m, f->off[m], f->off[m] + f->nnz[m], f->total);
    first[m] = leaves; leaves += cf::digest_leaves(f->nnz[m]);
    a.off[m] = (uint32_t)f->off[m]; a.nnz[m] = (uint32_t)f->nnz[m]; a.leaf_first[m] = (uint32_t)first[m];
  }
  a.leaves = (uint32_t)leaves;
  std::vector<uint8_t> h(32 * std::max<size_t>(leaves, 1));
  if (leaves) {
    std::lock_guard<std::mutex> g(c->mu);
    hipSetDevice(c->device);
    int rc;
    if ((rc = ensure(c, c->dense_ws, 32 * leaves))) return rc;
    LAUNCH(c, "k_circom_digest_leaves", k_circom_digest_leaves, (unsigned)((leaves + 63) / 64), 64, (const uint32_t*)f->rows, (const uint32_t*)f->cols, (const uint32_t*)f->vals,
           f->total, a, (uint64_t*)c->dense_ws.p);
    LAUNCHCHK(c);
    HIPCHK(c, hipMemcpyAsync(h.data(), c->dense_ws.p, 32 * leaves, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));                                 // the one wait
    if (c->prof) prof_drain(c);
  }
  const uint64_t shape[5] = {f->scan.n_cons, f->scan.n_wires, f->scan.n_pub, f->sh.nc, f->sh.nv};
  const uint64_t nnz[3] = {f->nnz[0], f->nnz[1], f->nnz[2]};
  const uint8_t* const lv[3] = {h.data() + 32 * first[0], h.data() + 32 * first[1], h.data() + 32 * first[2]};
  cf::digest_root(shape, nnz, lv, out);
  return SBN_OK;
}

int sbn_r1cs_from_circom(sbn_ctx* c, const sbn_circom_r1cs* f, sbn_r1cs** out) {
  if (!c || !f || !out) return SBN_EINVAL;
  *out = nullptr;
  std::lock_guard<std::mutex> g(c->mu);
  hipSetDevice(c->device);
  return r1cs_from_circom_locked(c, f, out);
}

int sbn_nizk_instance_from_circom(sbn_ctx* c, const sbn_circom_r1cs* f, const uint8_t* digest, size_t digest_len, sbn_nizk_inst** out) {
  if (!c || !f || (!digest && digest_len) || !out) return SBN_EINVAL;
  *out = nullptr;
  if (digest_len > UINT32_MAX) return fail(c, SBN_EINVAL, "nizk instance: a digest of %zu bytes: a transcript message has a 32-bit length", digest_len);
  if (f->sh.nv < 2) return fail(c, SBN_EINVAL, "nizk instance: num_vars = %zu pads to %zu: the opening of the witness needs at least one variable  [hyrax.rs:77]", f->sh.num_vars, f->sh.nv);
  std::unique_ptr<sbn_nizk_inst> k(new sbn_nizk_inst());
  k->sh = f->sh;
  if (digest_len) k->digest.assign(digest, digest + digest_len);
  NizkShapes s;
  if (!nizk_shapes(k.get(), &s)) return fail(c, SBN_EINVAL, "nizk instance: shape %zu x %zu is outside what the proof takes", f->sh.nc, f->sh.nv);
  {
    std::lock_guard<std::mutex> g(c->mu);
    hipSetDevice(c->device);
    const int rc = r1cs_from_circom_locked(c, f, &k->inst);
    if (rc) return rc;
  }
  *out = k.release();
  return SBN_OK;
}

int sbn_snark_encode_circom(sbn_ctx* c, const sbn_circom_r1cs* f, const sbn_snark_gens* gens, sbn_snark_key** out) {
  if (!c || !f || !gens || !out) return SBN_EINVAL;
  *out = nullptr;
  namespace sn = sbn_host::snark;
  const sn::Shape& sh = f->sh;
  if (sh.nv < 2) return fail(c, SBN_EINVAL, "snark encode: num_vars = %zu pads to %zu: the opening of the witness needs at least one variable  [hyrax.rs:77]", sh.num_vars, sh.nv);
  if (gens->nc != sh.nc || gens->nv != sh.nv) return fail(c, SBN_EINVAL, "snark encode: the generator bundle was made for %zu x %zu, the instance pads to %zu x %zu", gens->nc, gens->nv, sh.nc, sh.nv);
  size_t N = 1;
  for (int m = 0; m < 3; m++) while (N < f->nnz[m]) N <<= 1;
  if (N < 2) return fail(c, SBN_EINVAL, "snark encode: no matrix has more than one entry (N = %zu): the dot-product circuits cannot be split  [product_tree.rs:89 assert_eq]", N);
  if (sn::BATCH * N > ((size_t)1 << 31)) return fail(c, SBN_EINVAL, "snark encode: batch * N = 3 * %zu exceeds 2^31 (timestamps are 32-bit)", N);
  sbn_snark_key* k = new sbn_snark_key();
  int rc;
  {                                                                             // N is known before anything is built: a bundle made for another N launches nothing
    k->cm = sn::comm_of(sh, N);
    SnarkShapes s;
    if (!snark_shapes(k, false, &s)) { delete k; return fail(c, SBN_EINVAL, "snark encode: shape (%zu x %zu, N = %zu) is outside what the two proofs take", sh.nc, sh.nv, N); }
    const size_t ells[2] = {s.e.ell_o, s.e.ell_mm};
    for (int q = 0; q < 2; q++) {
      const sbn_bases* b = gens->g[q ? SNARK_MEM : SNARK_OPS];
      const size_t Rq = (size_t)1 << (ells[q] - ells[q] / 2);
      if (!b || b->n != Rq + 1 || !b->has_h) {
        delete k;
        return fail(c, SBN_EINVAL, "snark encode: %s has %zu points, N = %zu needs %zu with h: make the bundle with num_nz_entries = the largest nnz  [r1cs.rs:273-274]", q ? "gens_mem" : "gens_ops",
                    b ? b->n : (size_t)0, N, Rq + 1);
      }
    }
  }
  {
    std::lock_guard<std::mutex> g(c->mu);
    hipSetDevice(c->device);
    rc = r1cs_from_circom_locked(c, f, &k->inst);
    if (rc == SBN_OK) {
      // rows are constraint numbers (< num_cons <= cells) and columns remap_col's (< 2 num_vars_padded <= cells): k_dense_bounds / _rank guard them again
      DenseArgs a; memset(&a, 0, sizeof a);
      for (int m = 0; m < 3; m++) { a.off[m] = (uint32_t)f->off[m]; a.nnz[m] = (uint32_t)f->nnz[m]; }
      rc = dense_build_staged(c, f->rows, f->cols, f->vals, a, (size_t)sn::BATCH, N, (size_t)1 << std::max(sh.nx, sh.ny), 0, 0, &k->dense);
    }
  }
  if (rc) { snark_key_release(c, k); return rc; }
  return snark_encode_finish(c, k, sh, gens, out);
}

int sbn_circom_wtns_load(sbn_ctx* c, const uint8_t* file, size_t len, size_t num_inputs, sbn_table** vars, uint8_t* input, size_t* num_witness) {
  if (!c || !file || !vars || (!input && num_inputs) || !num_witness) return SBN_EINVAL;
  *vars = nullptr;
  namespace cf = sbn_host::circom;
  cf::WtnsSpan sp;
  const int e = cf::wtns_scan(file, len, &sp);
  if (e) return fail(c, SBN_EINVAL, "circom wtns: the file is refused: %s", cf::why(e));
  if (num_inputs >= sbn_host::snark::SHAPE_MAX || sp.count > 2 * sbn_host::snark::SHAPE_MAX) return fail(c, SBN_EINVAL, "circom wtns: %zu values, %zu inputs is too large", sp.count, num_inputs);
  if (sp.count < 1 + num_inputs) return fail(c, SBN_EINVAL, "circom wtns: %zu values, the constant and %zu inputs need %zu", sp.count, num_inputs, 1 + num_inputs);
  const size_t first = 1 + num_inputs, nvars = sp.count - first;
  const size_t tlen = sbn_host::snark::npo2(std::max(nvars, num_inputs + 1));   // num_vars_padded (snark.rs:75-81)
  std::lock_guard<std::mutex> g(c->mu);
  hipSetDevice(c->device);
  TableScope S(c); sbn_table* t = nullptr; int rc;
  if ((rc = S.alloc(tlen, "witness table", &t))) return rc;
  if ((rc = ensure(c, c->stage_scal, r1cs_align(sp.count * 32) + 256))) return rc;      // the section's values, then the flag word
  if ((rc = ensure_pin(c, 4096))) return rc;
  uint32_t* bad = (uint32_t*)((uint8_t*)c->stage_scal.p + r1cs_align(sp.count * 32));
  HIPCHK(c, hipMemcpyAsync(c->stage_scal.p, file + sp.off, sp.count * 32, hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemsetAsync(bad, 0xff, 4, c->stream));
  LAUNCH(c, "k_circom_wtns", k_circom_wtns, stream_grid(first + tlen), 256, (const uint32_t*)c->stage_scal.p, (uint32_t)sp.count, (uint32_t)first, (uint32_t)tlen, (uint32_t*)t->d, bad);
  LAUNCHCHK(c);
  HIPCHK(c, hipMemcpyAsync(c->pin, bad, 4, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  if (c->prof) prof_drain(c);
  const uint32_t b = *(const uint32_t*)c->pin;
  if (b != 0xffffffffu) return fail(c, SBN_EINVAL, "circom wtns: value %u is >= r  [scalar.rs:87-95]", b);
  if (num_inputs) memcpy(input, file + sp.off + 32, 32 * num_inputs);
  *num_witness = sp.count;
  *vars = S.give(t);
  return S.done();
}

}  // extern "C"
