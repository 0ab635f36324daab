// abi_r1cs.inc — C ABI: the R1CS matrices on the device (include/sbn254.h, reference src/r1cs.rs, src/sparse_mlpoly.rs, src/r1csproof.rs).
// The instance is uploaded once per circuit in two compressed copies (r1cs_kernels.cuh): row-major [A; B; C] for multiply and evaluate,
// column-major [A | B | C]^T for the phase-2 table.  Both are built on the host with a stable counting sort.

// one compressed matrix on the device: row_end (nrows), start_row (nchunks + 1), idx (nnz), val (nnz x 32 B, the table representation)
struct R1csCsr {
  uint32_t nrows = 0, nnz = 0, nchunks = 0;
  void* mem = nullptr;
  uint32_t *row_end = nullptr, *start_row = nullptr, *idx = nullptr, *val = nullptr;
};
struct sbn_r1cs {
  size_t nc = 0, nv = 0;                 // num_cons, num_vars
  uint32_t log_nc = 0, log_z = 0;        // log2(num_cons), log2(2 num_vars)
  size_t nnz[3] = {0, 0, 0};             // per matrix, after dropping columns >= 2 num_vars
  R1csCsr rowm, colm;                    // [A; B; C] (3 nc rows) and [A | B | C]^T (2 nv rows)
};

static size_t r1cs_align(size_t b) { return (b + 255) & ~(size_t)255; }
static uint32_t r1cs_log2(size_t n) { uint32_t l = 0; while (((size_t)1 << l) < n) l++; return l; }

// one compressed copy of `nrows` rows and `nnz` non-zeros: its device memory, nothing in it yet
static int r1cs_csr_alloc(sbn_ctx* c, R1csCsr& m, size_t nrows, size_t nnz) {
  m.nrows = (uint32_t)nrows; m.nnz = (uint32_t)nnz;
  m.nchunks = (uint32_t)(((uint64_t)m.nrows + m.nnz + R1CS_CHUNK - 1) / R1CS_CHUNK);
  const size_t b_re = r1cs_align((size_t)m.nrows * 4), b_sr = r1cs_align(((size_t)m.nchunks + 1) * 4), b_idx = r1cs_align((size_t)m.nnz * 4);
  const size_t b_val = r1cs_align((size_t)m.nnz * 32);
  hipError_t e = hipMalloc(&m.mem, b_re + b_sr + b_idx + std::max<size_t>(b_val, 256));
  if (e != hipSuccess) { m.mem = nullptr; return fail(c, SBN_ENOMEM, "r1cs_upload: hipMalloc (%zu non-zeros): %s", (size_t)m.nnz, hipGetErrorString(e)); }
  uint8_t* p = (uint8_t*)m.mem;
  m.row_end = (uint32_t*)p; m.start_row = (uint32_t*)(p + b_re); m.idx = (uint32_t*)(p + b_re + b_sr); m.val = (uint32_t*)(p + b_re + b_sr + b_idx);
  return SBN_OK;
}
// behind row_end, idx and val (canonical, or ark-ff's limbs under SBN_SCALARS_MONT): the values into the table representation, then the merge-path partition
static int r1cs_csr_finish(sbn_ctx* c, R1csCsr& m, uint32_t flags) {
  if (m.nnz) {
    if (!(flags & SBN_SCALARS_MONT)) LAUNCH(c, "k_fr_to_mont", k_fr_to_mont, stream_grid(m.nnz), 256, (const uint32_t*)m.val, m.val, (size_t)m.nnz);
    else LAUNCH(c, "k_fr_to_mont", k_fr_from_ark, stream_grid(m.nnz), 256, (const uint32_t*)m.val, m.val, (size_t)m.nnz);
  }
  LAUNCH(c, "k_r1cs_partition", k_r1cs_partition, stream_grid((size_t)m.nchunks + 1), 256, (const uint32_t*)m.row_end, m.nrows, m.nnz, m.nchunks, m.start_row);
  LAUNCHCHK(c);
  return SBN_OK;
}
// host arrays of one compressed copy -> device (values converted to the table representation), then the merge-path partition
static int r1cs_csr_upload(sbn_ctx* c, R1csCsr& m, const std::vector<uint32_t>& row_end, const std::vector<uint32_t>& idx, const std::vector<uint8_t>& val,
                           uint32_t flags) {
  int rc; if ((rc = r1cs_csr_alloc(c, m, row_end.size(), idx.size()))) return rc;
  HIPCHK(c, hipMemcpyAsync(m.row_end, row_end.data(), (size_t)m.nrows * 4, hipMemcpyHostToDevice, c->stream));
  if (m.nnz) {
    HIPCHK(c, hipMemcpyAsync(m.idx, idx.data(), (size_t)m.nnz * 4, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(m.val, val.data(), (size_t)m.nnz * 32, hipMemcpyHostToDevice, c->stream));
  }
  return r1cs_csr_finish(c, m, flags);
}

// y = M x into `out` (rows >= nrows dropped): merge-path pass, then fix-up passes until one lane is left.  Enqueue only.
static int r1cs_spmv_table(sbn_ctx* c, const R1csCsr& m, const uint32_t* x, const R1csOut& out) {
  const size_t n0 = m.nchunks, n1 = (n0 + R1CS_FIX_FIRST - 1) / R1CS_FIX_FIRST;
  const size_t bk0 = r1cs_align(n0 * 4), bv0 = r1cs_align(n0 * 32), bk1 = r1cs_align(n1 * 4), bv1 = r1cs_align(n1 * 32);
  int rc; if ((rc = ensure(c, c->r1cs_ws, bk0 + bv0 + bk1 + bv1))) return rc;
  uint8_t* ws = (uint8_t*)c->r1cs_ws.p;
  uint32_t *key[2] = {(uint32_t*)ws, (uint32_t*)(ws + bk0 + bv0)}, *val[2] = {(uint32_t*)(ws + bk0), (uint32_t*)(ws + bk0 + bv0 + bk1)};
  LAUNCH(c, "k_r1cs_spmv", k_r1cs_spmv<false>, (unsigned)((n0 + 255) / 256), 256, (const uint32_t*)m.row_end, (const uint32_t*)m.start_row, (const uint32_t*)m.idx,
         (const uint32_t*)m.val, m.nrows, m.nnz, m.nchunks, x, out, key[0], val[0], (const uint32_t*)nullptr, (uint32_t*)nullptr);
  int cur = 0;
  for (size_t n = n0, f = R1CS_FIX_FIRST; ; f = R1CS_FIX_CHUNK) {
    const size_t nt = (n + f - 1) / f;
    LAUNCH(c, "k_r1cs_fix", k_r1cs_fix, (unsigned)((nt + 255) / 256), 256, (const uint32_t*)key[cur], (const uint32_t*)val[cur], (uint32_t)n, (uint32_t)f, m.nrows, out,
           key[cur ^ 1], val[cur ^ 1]);
    if (nt == 1) break;
    n = nt; cur ^= 1;
  }
  LAUNCHCHK(c);
  return SBN_OK;
}

// the launches of sbn_r1cs_multiply / sbn_r1cs_eval_table; arguments checked, the caller holds the context's mutex (sbn_r1cs_proof_prove runs them too)
static int r1cs_multiply_locked(sbn_ctx* c, const sbn_r1cs* m, const sbn_table* z, sbn_table** Az, sbn_table** Bz, sbn_table** Cz) {
  TableScope S(c); sbn_table* t[3]; int rc;
  for (int k = 0; k < 3; k++) if ((rc = S.alloc(m->nc, "r1cs table", &t[k]))) return rc;
  R1csOut o; o.p[0] = (uint32_t*)t[0]->d; o.p[1] = (uint32_t*)t[1]->d; o.p[2] = (uint32_t*)t[2]->d; o.shift = m->log_nc;
  if ((rc = r1cs_spmv_table(c, m->rowm, (const uint32_t*)z->d, o))) return rc;
  if (c->prof) { hipStreamSynchronize(c->stream); prof_drain(c); }
  *Az = t[0]; *Bz = t[1]; *Cz = t[2];
  S.give_all();
  return S.done();
}
static int r1cs_eval_table_locked(sbn_ctx* c, const sbn_r1cs* m, const uint8_t* rx, size_t ell_x, const uint8_t rA[32], const uint8_t rB[32], const uint8_t rC[32],
                                  sbn_table** out) {
  TableScope S(c); sbn_table *eq = nullptr, *x = nullptr, *t = nullptr; int rc;
  if ((rc = eq_evals_locked(c, rx, ell_x, &eq))) return rc;
  S.keep(eq);
  if ((rc = S.alloc(3 * m->nc, "r1cs table", &x))) return rc;
  if ((rc = S.alloc(2 * m->nv, "r1cs table", &t))) return rc;
  // x = [r_A eq(rx) | r_B eq(rx) | r_C eq(rx)]: the combination of r1csproof.rs:376-387 folded into the gather
  const ScScalar a = scs_from(sbn_host::fr::to_dev_mont(el_from(rA))), b = scs_from(sbn_host::fr::to_dev_mont(el_from(rB))),
                 cc = scs_from(sbn_host::fr::to_dev_mont(el_from(rC)));
  LAUNCH(c, "k_r1cs_scale3", k_r1cs_scale3, stream_grid(3 * m->nc), 256, (const uint32_t*)eq->d, m->log_nc, a, b, cc, (uint32_t*)x->d);
  R1csOut o; o.p[0] = o.p[1] = o.p[2] = (uint32_t*)t->d; o.shift = m->log_z;
  if ((rc = r1cs_spmv_table(c, m->colm, (const uint32_t*)x->d, o))) return rc;
  if (c->prof) { hipStreamSynchronize(c->stream); prof_drain(c); }
  *out = S.give(t);
  return S.done();                                            // eq and x: recycled in stream order
}

// the launches of sbn_r1cs_evaluate; arguments checked, the caller holds the context's mutex (sbn_snark_prove runs them between its two halves)
static int r1cs_evaluate_locked(sbn_ctx* c, const sbn_r1cs* m, const uint8_t* rx, size_t ell_x, const uint8_t* ry, size_t ell_y, uint8_t out[96]) {
  const R1csCsr& rm = m->rowm;
  const unsigned nblk = (unsigned)std::max<size_t>(1, std::min<size_t>(R1CS_EVAL_BLOCKS, ((size_t)rm.nchunks + 255) / 256));
  TableScope S(c); sbn_table *ex = nullptr, *ey = nullptr;
  int rc = eq_evals_locked(c, rx, ell_x, &ex);
  S.keep(ex);
  if (rc == SBN_OK) rc = eq_evals_locked(c, ry, ell_y, &ey);
  S.keep(ey);
  if (rc == SBN_OK) rc = ensure(c, c->r1cs_ws, r1cs_align((size_t)nblk * 96) + 256);
  if (rc == SBN_OK) rc = ensure_pin(c, 4096);
  if (rc == SBN_OK) {
    uint32_t* partial = (uint32_t*)c->r1cs_ws.p;
    uint32_t* res = (uint32_t*)((uint8_t*)c->r1cs_ws.p + r1cs_align((size_t)nblk * 96));
    R1csOut o; o.p[0] = o.p[1] = o.p[2] = nullptr; o.shift = m->log_nc;
    // sum over the rows of M(row, .) . eq(ry), times eq(rx)[row], per matrix (sparse_mlpoly.rs:113-143), then the 3 x nblk block sums folded
    LAUNCH(c, "k_r1cs_spmv_eval", k_r1cs_spmv<true>, nblk, 256, (const uint32_t*)rm.row_end, (const uint32_t*)rm.start_row, (const uint32_t*)rm.idx,
           (const uint32_t*)rm.val, rm.nrows, rm.nnz, rm.nchunks, (const uint32_t*)ey->d, o, (uint32_t*)nullptr, (uint32_t*)nullptr,
           (const uint32_t*)ex->d, partial);
    LAUNCH(c, "k_sc_finish", k_sc_finish, 1, 64, (const uint32_t*)partial, (int)nblk, res);
    const hipError_t le = hipGetLastError();
    if (le != hipSuccess) rc = fail(c, SBN_EHIP, "r1cs_evaluate: %s", hipGetErrorString(le));
    else {
      hipError_t e = hipMemcpyAsync(c->pin, res, 96, hipMemcpyDeviceToHost, c->stream);
      if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
      if (c->prof) prof_drain(c);
      if (e != hipSuccess) rc = fail(c, SBN_EHIP, "r1cs_evaluate: %s", hipGetErrorString(e));
      else memcpy(out, c->pin, 96);
    }
  }
  return rc ? rc : S.done();
}

// Assignment::pad (snark.rs:149-156, :445-452): a vars table shorter than num_vars as a table of num_vars entries, zeros behind what the caller gave
// (zero words are the table's zero); a table of full length is used where it lies.  Enqueue only; the copy belongs to the caller's scope
static int r1cs_pad_vars(sbn_ctx* c, TableScope& T, const sbn_table* vars, size_t nv, const sbn_table** out) {
  if (vars->len == nv) { *out = vars; return SBN_OK; }
  sbn_table* p = nullptr; int rc;
  if ((rc = T.alloc(nv, "padded vars", &p))) return rc;
  HIPCHK(c, hipMemcpyAsync(p->d, vars->d, vars->len * 32, hipMemcpyDeviceToDevice, c->stream));
  HIPCHK(c, hipMemsetAsync((uint8_t*)p->d + vars->len * 32, 0, (nv - vars->len) * 32, c->stream));
  *out = p;
  return SBN_OK;
}
// R1CSShape::is_sat (r1cs.rs:105-123) on the device: z by k_r1cs_build_z, Az / Bz / Cz by the multiply, ONE k_r1cs_sat_check pass over them.  The three
// tables live in the call's scope and are released before it returns.  Arguments checked; the caller holds the context's mutex
static int r1cs_is_sat_locked(sbn_ctx* c, const sbn_r1cs* m, const sbn_table* vars, const uint8_t* input, size_t num_inputs, int* sat, uint64_t* num_bad, uint64_t* first_bad) {
  TableScope T(c);
  const sbn_table* pv = nullptr; sbn_table *z = nullptr, *in = nullptr, *Az = nullptr, *Bz = nullptr, *Cz = nullptr;
  int rc;
  if ((rc = ensure(c, c->sc_out, 4096))) return rc;
  if ((rc = ensure_pin(c, 4096))) return rc;
  if ((rc = r1cs_pad_vars(c, T, vars, m->nv, &pv))) return rc;
  if ((rc = T.alloc(2 * m->nv, "r1cs table", &z))) return rc;
  if (num_inputs) {                                                 // (canonical bytes, not table entries: k_r1cs_build_z converts them)
    if ((rc = T.alloc(num_inputs, "r1cs inputs", &in))) return rc;
    HIPCHK(c, hipMemcpyAsync(in->d, input, num_inputs * 32, hipMemcpyHostToDevice, c->stream));
  }
  LAUNCH(c, "k_r1cs_build_z", k_r1cs_build_z, stream_grid(2 * m->nv), 256, (const uint32_t*)pv->d, (const uint32_t*)(in ? in->d : nullptr), m->nv, num_inputs, (uint32_t*)z->d);
  LAUNCHCHK(c);
  if ((rc = r1cs_multiply_locked(c, m, z, &Az, &Bz, &Cz))) return rc;
  T.keep(Az); T.keep(Bz); T.keep(Cz);
  uint32_t* res = (uint32_t*)c->sc_out.p;                           // {violated rows, the lowest of them}
  HIPCHK(c, hipMemsetAsync(res, 0, 4, c->stream));
  HIPCHK(c, hipMemsetAsync(res + 1, 0xff, 4, c->stream));
  LAUNCH(c, "k_r1cs_sat_check", k_r1cs_sat_check, stream_grid(m->nc), 256, (const uint32_t*)Az->d, (const uint32_t*)Bz->d, (const uint32_t*)Cz->d, (uint32_t)m->nc, res);
  LAUNCHCHK(c);
  HIPCHK(c, hipMemcpyAsync(c->pin, res, 8, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  if (c->prof) prof_drain(c);
  const uint32_t* h = (const uint32_t*)c->pin;
  *sat = h[0] == 0 ? 1 : 0; *num_bad = h[0]; *first_bad = h[0] ? h[1] : 0;
  return T.done();
}
// what both witness checks refuse before any launch
static int r1cs_is_sat_check(sbn_ctx* c, const sbn_r1cs* m, const sbn_table* vars, const uint8_t* input, size_t num_inputs) {
  if (vars->len > m->nv) return fail(c, SBN_EINVAL, "r1cs is_sat: vars has %zu entries, the instance has num_vars = %zu  [snark.rs:142-144]", vars->len, m->nv);
  if (num_inputs >= m->nv) return fail(c, SBN_EINVAL, "r1cs is_sat: %zu inputs, num_vars = %zu: z = vars | 1 | inputs has 2 num_vars entries  [r1csproof.rs:253]", num_inputs, m->nv);
  for (size_t i = 0; i < num_inputs; i++) if (!fr_canonical(input + 32 * i)) return fail(c, SBN_EINVAL, "r1cs is_sat: input[%zu] is not canonical  [scalar.rs:87-95]", i);
  return SBN_OK;
}

extern "C" {

void sbn_r1cs_free(sbn_ctx* c, sbn_r1cs* m) {
  if (!m) return;
  if (c) { std::lock_guard<std::mutex> g(c->mu); hipSetDevice(c->device); hipStreamSynchronize(c->stream); }
  if (m->rowm.mem) hipFree(m->rowm.mem);
  if (m->colm.mem) hipFree(m->colm.mem);
  delete m;
}

int sbn_r1cs_upload(sbn_ctx* c, size_t num_cons, size_t num_vars, const uint32_t* const* rows, const uint32_t* const* cols, const uint8_t* const* vals,
                    const size_t* nnz, uint32_t flags, sbn_r1cs** out) {
  if (!c || !rows || !cols || !vals || !nnz || !out) return SBN_EINVAL;
  *out = nullptr;
  if (num_cons == 0 || (num_cons & (num_cons - 1)) || num_vars == 0 || (num_vars & (num_vars - 1)))
    return fail(c, SBN_EINVAL, "r1cs_upload: num_cons=%zu and num_vars=%zu must be powers of two", num_cons, num_vars);
  if (num_cons > ((size_t)1 << 29) || num_vars > ((size_t)1 << 29)) return fail(c, SBN_EINVAL, "r1cs_upload: shape too large");
  const size_t nz = 2 * num_vars;
  size_t total = 0;
  for (int m = 0; m < 3; m++) {
    if (nnz[m] && (!rows[m] || !cols[m] || !vals[m])) return fail(c, SBN_EINVAL, "r1cs_upload: matrix %d has %zu non-zeros and a NULL array", m, nnz[m]);
    total += nnz[m];
  }
  if (total > ((size_t)1 << 31)) return fail(c, SBN_EINVAL, "r1cs_upload: %zu non-zeros (at most 2^31)", total);
  for (int m = 0; m < 3; m++)
    for (size_t e = 0; e < nnz[m]; e++) {
      if (rows[m][e] >= num_cons) return fail(c, SBN_EINVAL, "r1cs_upload: matrix %d entry %zu: row %u >= num_cons %zu", m, e, rows[m][e], num_cons);
      if (!fr_canonical(vals[m] + 32 * e)) return fail(c, SBN_EINVAL, "r1cs_upload: matrix %d entry %zu: value >= r", m, e);
    }
  // the two compressed copies: stable counting sorts by row (row-major [A; B; C]) and by column (column-major [A | B | C]^T);
  // columns >= 2 num_vars are dropped (every reference loop skips them)
  const size_t nr = 3 * num_cons;
  std::vector<uint32_t> rp(nr + 1, 0), cp(nz + 1, 0);
  size_t kept = 0, kept_m[3] = {0, 0, 0};
  for (int m = 0; m < 3; m++)
    for (size_t e = 0; e < nnz[m]; e++) {
      const uint32_t col = cols[m][e];
      if (col >= nz) continue;
      rp[(size_t)m * num_cons + rows[m][e] + 1]++; cp[(size_t)col + 1]++; kept++; kept_m[m]++;
    }
  for (size_t i = 0; i < nr; i++) rp[i + 1] += rp[i];
  for (size_t i = 0; i < nz; i++) cp[i + 1] += cp[i];
  std::vector<uint32_t> r_idx(kept), c_idx(kept);
  std::vector<uint8_t> r_val(kept * 32), c_val(kept * 32);
  {
    std::vector<uint32_t> rpos(rp.begin(), rp.end() - 1), cpos(cp.begin(), cp.end() - 1);
    for (int m = 0; m < 3; m++)
      for (size_t e = 0; e < nnz[m]; e++) {
        const uint32_t col = cols[m][e];
        if (col >= nz) continue;
        const uint32_t g = (uint32_t)(m * num_cons + rows[m][e]);
        const uint32_t pr = rpos[g]++, pc = cpos[col]++;
        r_idx[pr] = col; memcpy(&r_val[(size_t)pr * 32], vals[m] + 32 * e, 32);
        c_idx[pc] = g;   memcpy(&c_val[(size_t)pc * 32], vals[m] + 32 * e, 32);
      }
  }
  std::vector<uint32_t> r_end(rp.begin() + 1, rp.end()), c_end(cp.begin() + 1, cp.end());
  std::lock_guard<std::mutex> g(c->mu);
  hipSetDevice(c->device);
  sbn_r1cs* h = new sbn_r1cs();
  h->nc = num_cons; h->nv = num_vars; h->log_nc = r1cs_log2(num_cons); h->log_z = r1cs_log2(nz);
  for (int m = 0; m < 3; m++) h->nnz[m] = kept_m[m];
  int rc = r1cs_csr_upload(c, h->rowm, r_end, r_idx, r_val, flags);
  if (rc == SBN_OK) rc = r1cs_csr_upload(c, h->colm, c_end, c_idx, c_val, flags);
  const hipError_t se = hipStreamSynchronize(c->stream);        // the host arrays go out of scope here
  if (c->prof) prof_drain(c);
  if (rc == SBN_OK && se != hipSuccess) rc = fail(c, SBN_EHIP, "r1cs_upload: %s", hipGetErrorString(se));
  if (rc) {
    if (h->rowm.mem) hipFree(h->rowm.mem);
    if (h->colm.mem) hipFree(h->colm.mem);
    delete h;
    return rc;
  }
  *out = h;
  return SBN_OK;
}

int sbn_r1cs_multiply(sbn_ctx* c, const sbn_r1cs* m, const sbn_table* z, sbn_table** Az, sbn_table** Bz, sbn_table** Cz) {
  if (!c || !m || !z || !Az || !Bz || !Cz) return SBN_EINVAL;
  *Az = *Bz = *Cz = nullptr;
  if (z->len != 2 * m->nv) return fail(c, SBN_EINVAL, "r1cs_multiply: z has %zu entries, the shape needs 2 num_vars = %zu (r1cs.rs:139)", z->len, 2 * m->nv);
  std::lock_guard<std::mutex> g(c->mu);
  hipSetDevice(c->device);
  return r1cs_multiply_locked(c, m, z, Az, Bz, Cz);
}

int sbn_r1cs_eval_table(sbn_ctx* c, const sbn_r1cs* m, const uint8_t* rx, size_t ell_x, const uint8_t rA[32], const uint8_t rB[32], const uint8_t rC[32],
                        sbn_table** out) {
  if (!c || !m || (!rx && ell_x) || !rA || !rB || !rC || !out) return SBN_EINVAL;
  *out = nullptr;
  if (ell_x != m->log_nc) return fail(c, SBN_EINVAL, "r1cs_eval_table: ell_x=%zu, the shape needs log2(num_cons) = %u", ell_x, m->log_nc);
  if (!fr_canonical(rA) || !fr_canonical(rB) || !fr_canonical(rC)) return fail(c, SBN_EINVAL, "r1cs_eval_table: r_A, r_B or r_C is not canonical (>= r)");
  std::lock_guard<std::mutex> g(c->mu);
  hipSetDevice(c->device);
  return r1cs_eval_table_locked(c, m, rx, ell_x, rA, rB, rC, out);
}

int sbn_r1cs_evaluate(sbn_ctx* c, const sbn_r1cs* m, const uint8_t* rx, size_t ell_x, const uint8_t* ry, size_t ell_y, uint8_t out[96]) {
  if (!c || !m || (!rx && ell_x) || (!ry && ell_y) || !out) return SBN_EINVAL;
  if (ell_x != m->log_nc || ell_y != m->log_z)
    return fail(c, SBN_EINVAL, "r1cs_evaluate: ell_x=%zu, ell_y=%zu; the shape needs %u and %u (r1cs.rs:126-129)", ell_x, ell_y, m->log_nc, m->log_z);
  std::lock_guard<std::mutex> g(c->mu);
  hipSetDevice(c->device);
  return r1cs_evaluate_locked(c, m, rx, ell_x, ry, ell_y, out);
}

int sbn_r1cs_is_sat(sbn_ctx* c, const sbn_r1cs* m, const sbn_table* vars, const uint8_t* input, size_t num_inputs, int* sat, uint64_t* num_bad, uint64_t* first_bad) {
  if (!c || !m || !vars || (!input && num_inputs) || !sat || !num_bad || !first_bad) return SBN_EINVAL;
  int rc;
  if ((rc = r1cs_is_sat_check(c, m, vars, input, num_inputs))) return rc;
  std::lock_guard<std::mutex> g(c->mu);
  hipSetDevice(c->device);
  int s = 0; uint64_t nb = 0, fb = 0;
  if ((rc = r1cs_is_sat_locked(c, m, vars, input, num_inputs, &s, &nb, &fb))) return rc;
  *sat = s; *num_bad = nb; *first_bad = fb;
  return SBN_OK;
}

}  // extern "C"
