// abi_derefs_key.inc — C ABI: sbn_derefs_key, the per-cell SRS sums of one (circuit, SRS) pair (include/sbn254.h), and the KZG build's derefs
// commitment from them (Derefs::commit_kzg, sparse_mlpoly_full.rs:307-312 -> KZGPolyCommitment::commit, kzg.rs:386-397).
//   derefs[i] = eq[addr[i]]  =>  sum_i derefs[i] [tau^i]G = sum_a eq[a] S_a,   S[side][a] = sum_{k < b} sum_{i < N, addr[side][k][i] = a} srs[(side b + k) N + i]
// The build is a segmented point sum over the counting sort sbn_dense already holds (audit_ts = count per cell, read_ts = rank within the cell): the
// bucket accumulate of run_bucket_job (launch_accumulate, msm_host.hpp) over P = 2 problems of nb = cells buckets, estride = batch * N, one lane per
// bucket, stopped before the reduction: the buckets are the result.  Cell 0 takes every padding op, so the heaviest
// bucket holds most of a side: it is cut into segments of SEG entries like any oversized bucket.  Included by sbn254.hip.

struct sbn_derefs_key {
  size_t batch = 0, N = 0, cells = 0, srs_n = 0;       // the shape and SRS length the key was built for
  const sbn_dense* dense = nullptr;                   // compared only, never dereferenced: sbn_sparse_eval_prove_kzg refuses a key of another pair
  const sbn_bases* srs = nullptr;
  sbn_bases* pts = nullptr;                            // the kept cells' sums: len Montgomery affine points, an MSM base set of its own (GLV table included)
  void* d_ids = nullptr;                               // len x u32: side << 31 | a, row side first, ascending
  std::vector<uint32_t> ids;
};

// SEG of the key build: the bucket job's rule (acc_seg, msm_plan.hpp) for (P = 2, nb = cells, estride = bN), then raised until the heaviest cell's merge chain fits a lane:
// k_acc_merge folds k = ceil(cnt / SEG) - 1 partials lane-strided over one wave, k / 64 additions per lane, and no lane may run more than ACC_SEG_MAX
static uint32_t derefs_key_seg(size_t cells, size_t bN, uint32_t maxcnt) {
  uint32_t SEG = acc_seg(2, bN, cells);
  while ((size_t)maxcnt / SEG / 64 > ACC_SEG_MAX && SEG < ACC_SEG_MAX) SEG <<= 1;
  return SEG;
}

static void derefs_key_release(sbn_ctx* c, sbn_derefs_key* k) {
  if (k->pts) sbn_bases_free(c, k->pts);
  if (k->d_ids) hipFree(k->d_ids);
  delete k;
}

// eq(rx)[a] / eq(ry)[a] of the kept cells, canonical, then the MSM over the key's points; the caller holds the mutex
static int derefs_key_commit_locked(sbn_ctx* c, const sbn_derefs_key* k, const sbn_table* mem_rx, const sbn_table* mem_ry, uint8_t out_xy[64], int* out_is_inf) {
  const size_t len = k->ids.size();
  int rc; if ((rc = ensure(c, c->scal_canon, len * 32))) return rc;
  LAUNCH(c, "k_dk_scalars", k_dk_scalars, stream_grid(len), 256, (const uint32_t*)mem_rx->d, (const uint32_t*)mem_ry->d, (const uint32_t*)k->d_ids, len, (uint32_t*)c->scal_canon.p);
  LAUNCHCHK(c);
  return msm_device(c, (const uint32_t*)c->scal_canon.p, (const uint32_t*)k->pts->d_pts, len, out_xy, out_is_inf, k->pts);
}

extern "C" {

int sbn_derefs_key_build(sbn_ctx* c, const sbn_dense* dn, const sbn_bases* srs, sbn_derefs_key** out) {
  if (!c || !dn || !srs || !out) return SBN_EINVAL;
  *out = nullptr;
  std::lock_guard<std::mutex> g(c->mu); hipSetDevice(c->device);
  const size_t b = dn->batch, N = dn->N, cells = dn->cells, bN = b * N, NB = 2 * cells;
  if (srs->has_h) return fail(c, SBN_EINVAL, "derefs key: the SRS handle has an h; an SRS is sbn_kzg_srs_upload's or sbn_kzg_srs_from_tau's");
  if (2 * bN >= ((size_t)1 << 31)) return fail(c, SBN_EINVAL, "derefs key: 2 * batch * N = %zu: an entry's index must leave bit 31 clear", 2 * bN);
  if (srs->n < 2 * bN) return fail(c, SBN_EINVAL, "derefs key: the SRS has %zu points, the derefs polynomial's non-zero prefix %zu coefficients", srs->n, 2 * bN);
  if (bN == 0 || cells == 0 || cells > ((size_t)1 << 30)) return fail(c, SBN_EINVAL, "derefs key: %zu cells, batch * N = %zu", cells, bN);
  int rc;
  // the 2 x cells counters on the host: the heaviest cell (SEG), the cells read at least once (scan and compaction run once per circuit)
  std::vector<uint32_t> h(NB);
  HIPCHK(c, hipStreamSynchronize(c->stream));
  HIPCHK(c, hipMemcpy(h.data(), dense_audit(dn, 0), NB * 4, hipMemcpyDeviceToHost));
  uint32_t maxcnt = 0;
  std::unique_ptr<sbn_derefs_key> kp(new sbn_derefs_key());
  for (size_t t = 0; t < NB; t++) {
    if (h[t] > bN) return fail(c, SBN_EINVAL, "derefs key: audit_ts[%zu] = %u exceeds batch * N = %zu", t, h[t], bN);
    maxcnt = std::max(maxcnt, h[t]);
    if (h[t]) kp->ids.push_back((uint32_t)((t / cells) << 31) | (uint32_t)(t % cells));
  }
  for (int side = 0; side < 2; side++) {
    size_t sum = 0; for (size_t a = 0; a < cells; a++) sum += h[(size_t)side * cells + a];
    if (sum != bN) return fail(c, SBN_EINVAL, "derefs key: the %s side's audit_ts sum to %zu, not batch * N = %zu", side ? "column" : "row", sum, bN);
  }
  const size_t len = kp->ids.size();
  AccPlan a; memset(&a, 0, sizeof a);          // no reduction: L, chunks, levels and quad stay 0, as sbn_prof_last_acc reports them
  a.LPB = 1; acc_set_seg(a, derefs_key_seg(cells, bN, maxcnt), 2, bN, cells);
  if ((rc = ensure_accumulate(c, NB, 2 * bN, a))) return rc;
  if ((rc = ensure(c, c->gen_tmp, len * 128))) return rc;
  const uint32_t* hist = dense_audit(dn, 0);
  uint32_t* offs = (uint32_t*)c->offs.p; uint32_t* sorted = (uint32_t*)c->sorted.p;
  sbn_bases* pts = new sbn_bases(); pts->n = len; pts->has_h = false;
  kp->pts = pts;
  auto bail = [&](int code) { hipStreamSynchronize(c->stream); sbn_derefs_key* k = kp.release(); derefs_key_release(nullptr, k); return code; };
  if (hipMalloc(&pts->d_pts, len * 64) != hipSuccess || hipMalloc(&kp->d_ids, len * 4) != hipSuccess) { (void)hipGetLastError(); return bail(fail(c, SBN_ENOMEM, "derefs key: hipMalloc of %zu points", len)); }
  if (hipMemcpyAsync(kp->d_ids, kp->ids.data(), len * 4, hipMemcpyHostToDevice, c->stream) != hipSuccess) return bail(fail(c, SBN_EHIP, "derefs key: upload of the cell ids"));
  if (hipMemsetAsync(c->acc_ctr.p, 0, ACC_CTR_BYTES, c->stream) != hipSuccess) return bail(fail(c, SBN_EHIP, "derefs key: clearing the counters"));
  c->last_job[0] = 0; c->last_job[1] = 2; c->last_job[2] = (uint64_t)(2 * bN); c->last_job[3] = (uint64_t)NB;
  store_last_acc(c, a);
  LAUNCH(c, "k_scan", k_scan, 2, 1024, hist, offs, (int)cells);
  LAUNCH(c, "k_dk_place", k_dk_place, stream_grid(2 * bN), 256, (const uint32_t*)dn->u32s, bN, (uint32_t)cells, hist, (const uint32_t*)offs, sorted);
  launch_accumulate(c, (const uint32_t*)srs->d_pts, NB, (int)cells, bN, a, hist);
  // the cells with audit_ts > 0 (a cell never read is the identity: it has no affine form), as a base set
  LAUNCH(c, "k_dk_gather", k_dk_gather, stream_grid(len), 256, (const uint32_t*)c->buckets.p, (const uint32_t*)kp->d_ids, (uint32_t)cells, len, (uint32_t*)c->gen_tmp.p);
  LAUNCH(c, "k_xyzz_to_affine", k_xyzz_to_affine, (unsigned)((len + 63) / 64), 64, (const uint32_t*)c->gen_tmp.p, (uint32_t*)pts->d_pts, (uint32_t*)nullptr, (uint8_t*)nullptr, len);
  const hipError_t le = hipGetLastError(), se = hipStreamSynchronize(c->stream);
  if (c->prof) prof_drain(c);
  if (le != hipSuccess || se != hipSuccess) return bail(fail(c, SBN_EHIP, "derefs key build: %s", hipGetErrorString(le != hipSuccess ? le : se)));
  kp->batch = b; kp->N = N; kp->cells = cells; kp->srs_n = srs->n; kp->dense = dn; kp->srs = srs;
  *out = kp.release();
  return SBN_OK;
}

void sbn_derefs_key_free(sbn_ctx* c, sbn_derefs_key* k) {
  if (!k) return;
  std::unique_lock<std::mutex> g;
  if (c) { g = std::unique_lock<std::mutex>(c->mu); hipSetDevice(c->device); hipStreamSynchronize(c->stream); }
  derefs_key_release(c, k);
}

size_t sbn_derefs_key_len(const sbn_derefs_key* k) { return k ? k->ids.size() : 0; }

int sbn_derefs_key_download(sbn_ctx* c, const sbn_derefs_key* k, size_t first, size_t count, uint32_t* out_cell, uint8_t* out_xy) {
  if (!c || !k || (count && (!out_cell || !out_xy))) return SBN_EINVAL;
  if (first > k->ids.size() || count > k->ids.size() - first) return fail(c, SBN_EINVAL, "derefs key download: [%zu, %zu) of %zu cells", first, first + count, k->ids.size());
  if (!count) return SBN_OK;
  std::lock_guard<std::mutex> g(c->mu); hipSetDevice(c->device);
  int rc; if ((rc = ensure(c, c->out_small, count * 64))) return rc;
  LAUNCH(c, "k_points_from_mont", k_points_from_mont, (unsigned)((count + 255) / 256), 256, (const uint32_t*)k->pts->d_pts + 16 * first, (uint32_t*)c->out_small.p, count);
  LAUNCHCHK(c);
  HIPCHK(c, hipMemcpyAsync(out_xy, c->out_small.p, count * 64, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  if (c->prof) prof_drain(c);
  memcpy(out_cell, k->ids.data() + first, count * 4);
  return SBN_OK;
}

int sbn_derefs_key_commit(sbn_ctx* c, const sbn_derefs_key* k, const sbn_table* mem_rx, const sbn_table* mem_ry, uint8_t out_xy[64], int* out_is_inf) {
  if (!c || !k || !mem_rx || !mem_ry || !out_xy) return SBN_EINVAL;
  if (mem_rx->len < k->cells || mem_ry->len < k->cells) return fail(c, SBN_EINVAL, "derefs key commit: the eq tables hold %zu and %zu entries, the memories %zu cells", mem_rx->len, mem_ry->len, k->cells);
  std::lock_guard<std::mutex> g(c->mu); hipSetDevice(c->device);
  return derefs_key_commit_locked(c, k, mem_rx, mem_ry, out_xy, out_is_inf);
}

}  // extern "C"
