// msm_host.hpp — launch code of the MSM / commitment path: the bucket pipeline (digits -> LDS counting sort -> load-ordered accumulation ->
// reduction) run from a plan (msm_plan.hpp: window choice, overrides, geometry), window tables, merging of equal bases, row-chunk launches.
// Reference boundary: group.rs:171-175, commitments.rs:144-154, hyrax.rs:253-308 (included by sbn254.hip only).
#pragma once
// ---- two-level sort of a large single MSM (sort2_kernels.cuh) ----
#define S2_FOR_EACH_C(X) X(13) X(14) X(15) X(16) X(17) X(18) X(19) X(20) X(21) X(22)
#define S2_GLV_FOR_EACH_C(X) X(13) X(14) X(15) X(16) X(17)        // window bits the GLV half-scalars (16-byte records) are instantiated for
// the level-1 kernels of every instantiated (record, window bits, scalars per thread): plain (8 words) and GLV (4 words), each at both SPT values
struct S2Variant {
  bool glv; int c, spt;
  void (*count)(const uint32_t*, S2Geom, uint32_t*, uint32_t*);
  void (*scatter)(const uint32_t*, S2Geom, const uint32_t*, const uint32_t*, uint32_t*, uint16_t*);
};
#define S2_ROW(C, SPT, SW) {SW == 4, C, SPT, k_s2_count<C, SPT, SW>, k_s2_scatter<C, SPT, SW>},
#define S2_PLAIN(C) S2_ROW(C, S2_SPT, 8) S2_ROW(C, S2_SPT_SMALL, 8)
#define S2_GLV(C) S2_ROW(C, S2_SPT, 4) S2_ROW(C, S2_SPT_SMALL, 4)
static const S2Variant s2_variants[] = { S2_FOR_EACH_C(S2_PLAIN) S2_GLV_FOR_EACH_C(S2_GLV) };
#undef S2_GLV
#undef S2_PLAIN
#undef S2_ROW
static const S2Variant* sort2_variant(bool glv, int c, int spt) {
  for (const S2Variant& v : s2_variants) if (v.glv == glv && v.c == c && v.spt == spt) return &v;
  return nullptr;
}
static bool sort2_set_lds() {
  bool ok = true;
  auto grant = [&](const void* kern, size_t bytes) { if (hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes) != hipSuccess) { (void)hipGetLastError(); ok = false; } };
  grant((const void*)k_s2_place, s2_place_lds_bytes(S2_LO_LOG_MAX));
  for (const S2Variant& v : s2_variants) { grant((const void*)v.scatter, s2_scatter_lds_bytes(S2_P_MAX)); grant((const void*)v.count, S2_COUNT_LDS_BYTES); }
  return ok;
}
static bool sort2_applies(const sbn_ctx* c, int mode, size_t n, int cbits) {
  return mode == MODE_SINGLE && c->sort2_ok && c->sort2_min && n >= c->sort2_min && cbits >= S2_C_MIN && cbits <= S2_C_MAX;
}
// scalars -> hist / offs / sorted of all W windows (the arrays the one-level sort leaves behind)
// glv: the n records are GLV half-scalars (16 B each, glv_kernels.cuh); record t >= n/2 indexes point t + glv_gap
static int sort2_run(sbn_ctx* c, const MsmOverrides& o, const uint32_t* scalars, size_t n, const MsmShape& s, size_t estride, uint32_t* hist, uint32_t* offs, uint32_t* sorted, bool glv = false, size_t glv_gap = 0) {
  if (glv && (s.c < 13 || s.c > 17)) return fail(c, SBN_EINVAL, "two-level sort: no GLV instantiation for windows of %d bits", s.c);
  const Sort2Plan p = sort2_plan(n, s, o);
  if (p.status == S2_PLAN_TOO_WIDE) return fail(c, SBN_EINVAL, "two-level sort: window of %d bits is too wide", s.c);
  S2Geom g; g.n = n; g.c = s.c; g.W = s.W; g.half = n / 2; g.gap = glv ? glv_gap : 0;
  g.lo_log = p.lo_log; g.P = p.P; g.K = p.K;
  const size_t LO = (size_t)1 << g.lo_log, WP = (size_t)g.W * g.P;
  int rc;
  if ((rc = ensure(c, c->s2_cnt, WP * g.K * 4)) || (rc = ensure(c, c->s2_part, (3 * WP + 1) * 4))) return rc;
  if ((rc = ensure(c, c->s2_idx, (size_t)g.W * n * 4)) || (rc = ensure(c, c->s2_lo, (size_t)g.W * n * 2)) || (rc = ensure(c, c->blockhist, p.max_sc * LO * 4))) return rc;
  uint32_t* cntA = (uint32_t*)c->s2_cnt.p; uint32_t* part_cnt = (uint32_t*)c->s2_part.p; uint32_t* part_off = part_cnt + WP; uint32_t* sc_off = part_off + WP;
  uint32_t* tmp_idx = (uint32_t*)c->s2_idx.p; uint16_t* tmp_lo = (uint16_t*)c->s2_lo.p; uint32_t* bh = (uint32_t*)c->blockhist.p;
  const size_t lds_a = WP * 4, lds_c = s2_scatter_lds_bytes(g.P, p.spt);
  if (p.status == S2_PLAN_COUNTERS) return fail(c, SBN_EINVAL, "two-level sort: %zu level-1 counters do not fit the LDS granted to k_s2_count", WP);
  const S2Variant* v = sort2_variant(glv, s.c, p.spt);
  if (!v) return fail(c, SBN_EINVAL, "two-level sort: no instantiation for windows of %d bits", s.c);     // not reached: sort2_applies admits S2_C_MIN .. S2_C_MAX only
  {
    ProfScope _ps(c, "k_s2_count");
    hipLaunchKernelGGL(v->count, dim3(g.K), dim3(1024), lds_a, c->stream, scalars, g, cntA, c->d_bad);
  }
  LAUNCH(c, "k_s2_prefix", k_s2_prefix_k, (unsigned)WP, 256, cntA, g.K, part_cnt);
  LAUNCH(c, "k_s2_prefix", k_s2_prefix_hi, 1, 1024, (const uint32_t*)part_cnt, g.W, g.P, part_off, sc_off);
  {
    ProfScope _ps(c, "k_s2_scatter");
    hipLaunchKernelGGL(v->scatter, dim3(g.K), dim3(1024), lds_c, c->stream, scalars, g, (const uint32_t*)cntA, (const uint32_t*)part_off, tmp_idx, tmp_lo);
  }
  const unsigned l2 = s2_level2_blocks(p.max_sc);
  LAUNCH(c, "k_s2_hist", k_s2_hist, l2, 1024, (const uint16_t*)tmp_lo, g, (const uint32_t*)part_off, (const uint32_t*)part_cnt, (const uint32_t*)sc_off, bh);
  LAUNCH(c, "k_s2_prefix", k_s2_prefix2, (unsigned)WP, 1024, bh, g, (const uint32_t*)part_off, (const uint32_t*)sc_off, hist, offs);
  {
    ProfScope _ps(c, "k_s2_place");
    hipLaunchKernelGGL(k_s2_place, dim3(l2), dim3(1024), s2_place_lds_bytes(g.lo_log), c->stream,
                       (const uint16_t*)tmp_lo, (const uint32_t*)tmp_idx, g, (const uint32_t*)part_off, (const uint32_t*)part_cnt, (const uint32_t*)sc_off, (const uint32_t*)bh, (const uint32_t*)offs, sorted, estride);
  }
  LAUNCHCHK(c);            // a refused launch (LDS, grid) is reported here, by the sort, not by whatever runs next
  return SBN_OK;
}

struct BucketJob {
  int mode; DigitArgs da; MsmShape s;
  size_t P;               // problems (windows or rows)
  size_t threads;         // digit-kernel threads
  const uint32_t* points; // Montgomery affine points the entries index
  const uint8_t* skip;    // ROWS: per-row flags, 2 = all-zero row whose stages can be skipped (or null)
  bool glv;               // SINGLE over GLV half-scalars (da.n = 2 x bases, 16-byte records): points = the GLV table, record t >= n/2
  size_t glv_gap;         // indexes point t + glv_gap
};

// ---- the accumulate of a bucket job, shared with the derefs key (abi_derefs_key.inc), whose buckets are its result ----
static const size_t ACC_CTR_BYTES = 64 + (ACC_SEG_MAX + 2) * 4;      // the counters of the accumulate kernels, then the size bins of the bucket ordering: ONE memset clears both
static_assert(sizeof(AccCounters) <= 64, "the size bins follow the counters at byte 64");
// everything launch_accumulate touches but the histogram: NB buckets of a.LPB slots, `entries` sorted entries in all
static int ensure_accumulate(sbn_ctx* c, size_t NB, size_t entries, const AccPlan& a) {
  int rc;
  if ((rc = ensure(c, c->offs, NB * 4)) || (rc = ensure(c, c->sorted, entries * 4)) || (rc = ensure(c, c->buckets, NB * 128 * (size_t)a.LPB)) || (rc = ensure(c, c->acc_ctr, ACC_CTR_BYTES))) return rc;
  if ((rc = ensure(c, c->extra_list, a.max_extra * sizeof(ExtraItem))) || (rc = ensure(c, c->extra_out, a.max_extra * 128)) || (rc = ensure(c, c->big_list, a.max_big * sizeof(BigItem)))) return rc;
  return ensure(c, c->perm, NB * 4);
}
// bucket order by decreasing load (the size bins were cleared with the counters), then the three accumulate kernels: c->buckets holds the sums
static void launch_accumulate(sbn_ctx* c, const uint32_t* points, size_t NB, int nb, size_t estride, const AccPlan& a, const uint32_t* hist) {
  const uint32_t* offs = (const uint32_t*)c->offs.p; const uint32_t* sorted = (const uint32_t*)c->sorted.p; uint32_t* buckets = (uint32_t*)c->buckets.p;
  AccCounters* ctr = (AccCounters*)c->acc_ctr.p;
  uint32_t* size_bins = (uint32_t*)((uint8_t*)c->acc_ctr.p + 64);
  const uint32_t SEG = a.SEG;
  LAUNCH(c, "k_size_sort", k_size_hist, (unsigned)((NB + 1023) / 1024), 1024, hist, NB, SEG, size_bins);
  LAUNCH(c, "k_size_sort", k_size_scan, 1, 64, size_bins, SEG);
  LAUNCH(c, "k_size_sort", k_size_scatter, (unsigned)((NB + 1023) / 1024), 1024, hist, NB, SEG, size_bins, (uint32_t*)c->perm.p);
  const unsigned agrid = (unsigned)((NB * (size_t)a.LPB + 255) / 256);
  LAUNCH(c, "k_acc_first", (a.LPB == 1 ? k_acc_first<1> : k_acc_first<2>), agrid, 256, points, NB, nb, estride, SEG, hist, offs, sorted, (const uint32_t*)c->perm.p, buckets, ctr,
         (ExtraItem*)c->extra_list.p, (BigItem*)c->big_list.p);
  // grid-stride over at most max_extra items (the work list's capacity): no more blocks than that many lanes, 2048 at the most
  const unsigned egrid = (unsigned)std::max<size_t>(1, std::min<size_t>(2048, (a.max_extra + 255) / 256));
  LAUNCH(c, "k_acc_extra", k_acc_extra, egrid, 256, points, nb, estride, SEG, hist, offs, sorted, (const AccCounters*)ctr, (const ExtraItem*)c->extra_list.p, (uint32_t*)c->extra_out.p);
  LAUNCH(c, "k_acc_merge", k_acc_merge, 4096, 64, (const AccCounters*)ctr, (const BigItem*)c->big_list.p, (const uint32_t*)c->extra_out.p, buckets, a.LPB);
}
// weighted sums of the buckets per problem -> c->wsum (P x XYZZ)
static void launch_reduce(sbn_ctx* c, size_t P, int nb, const AccPlan& a, const uint8_t* skip) {
  LAUNCH(c, "k_reduce_l1", k_reduce_l1, (unsigned)(P * a.chunks), 64, (const uint32_t*)c->buckets.p, a.L, nb, (uint32_t*)c->red_a.p, skip, a.chunks, a.LPB);
  uint32_t* in = (uint32_t*)c->red_a.p; uint32_t* outb = (uint32_t*)c->red_b.p;
  int G = a.chunks;
  for (int k64 = 1; k64 <= a.levels; k64++) {
    const int Gout = (G + 63) / 64, final = (k64 == a.levels);
    if (a.quad) LAUNCH(c, "k_reduce_combine", k_reduce_combine_quad, (unsigned)(P * Gout), 256, in, G, Gout, k64, a.L, final, final ? (uint32_t*)c->wsum.p : outb);
    else LAUNCH(c, "k_reduce_combine", k_reduce_combine, (unsigned)(P * Gout), 64, in, G, Gout, k64, a.L, final, final ? (uint32_t*)c->wsum.p : outb);
    std::swap(in, outb); G = Gout;
  }
}
static void store_last_acc(sbn_ctx* c, const AccPlan& a) { const uint64_t v[6] = {a.SEG, (uint64_t)a.LPB, (uint64_t)a.L, (uint64_t)a.chunks, (uint64_t)a.levels, a.quad ? 1u : 0u}; memcpy(c->last_acc, v, sizeof v); }

// digits -> counting sort -> segmented bucket accumulation -> per-problem weighted sums in c->wsum (P x XYZZ)
static int run_bucket_job(sbn_ctx* c, const BucketJob& J, const MsmOverrides& o) {
  const MsmShape& s = J.s;
  const size_t NB = J.P * (size_t)s.nb;
  if (NB > 0xffffffffull) return fail(c, SBN_EINVAL, "bucket space too large");
  const size_t estride = J.da.estride;
  c->last_job[0] = (uint64_t)s.c; c->last_job[1] = (uint64_t)s.W; c->last_job[2] = (uint64_t)(J.P * estride); c->last_job[3] = (uint64_t)NB;
  const AccPlan a = acc_plan(J.mode, J.da.n, J.P, estride, s.nb, o);
  int rc;
  if ((rc = ensure(c, c->hist, NB * 4)) || (rc = ensure_accumulate(c, NB, J.P * estride, a))) return rc;
  if ((rc = ensure(c, c->red_a, J.P * a.chunks * 256)) || (rc = ensure(c, c->red_b, J.P * ((a.chunks + 63) / 64) * 256)) || (rc = ensure(c, c->wsum, J.P * 128))) return rc;
  uint32_t* hist = (uint32_t*)c->hist.p; uint32_t* offs = (uint32_t*)c->offs.p; uint32_t* sorted = (uint32_t*)c->sorted.p;
  HIPCHK(c, hipMemsetAsync(c->acc_ctr.p, 0, ACC_CTR_BYTES, c->stream));
  // digits once, then the LDS counting sort
  const uint8_t* skip = nullptr;
  const bool two_level = sort2_applies(c, J.mode, J.da.n, s.c) && !J.skip;
  if (s.c > MSM_C_MAX && !two_level) return fail(c, SBN_EINVAL, "window of %d bits needs the two-level sort", s.c);
  if (J.glv && !two_level) return fail(c, SBN_EINVAL, "GLV half-scalars need the two-level sort");
  if (two_level) {
    if ((rc = sort2_run(c, o, J.da.scalars, J.da.n, s, estride, hist, offs, sorted, J.glv, J.glv_gap))) return rc;
  } else {
    const Sort1Plan sp = sort1_plan(c->sort_rs_max, J.P, estride, s.nb);
    SortGeom g; memset(&g, 0, sizeof g);
    g.E = estride; g.estride = estride; g.nb = s.nb; g.mode = J.mode; g.ncol = J.da.n; g.tstride = J.da.tstride;
    g.RS = sp.RS; g.logRS = sp.logRS; g.R = sp.R; g.K = sp.K; g.chunk = sp.chunk;
    if (J.P > 65535 || g.R > 65535) return fail(c, SBN_EINVAL, "sort grid too large (P=%zu R=%d)", J.P, g.R);
    if ((rc = ensure(c, c->digits, J.P * estride * sizeof(dig_t)))) return rc;
    if ((rc = ensure(c, c->blockhist, J.P * (size_t)g.R * g.K * g.RS * 4))) return rc;
    dig_t* dig = (dig_t*)c->digits.p; uint32_t* bh = (uint32_t*)c->blockhist.p;
    const unsigned gd = (unsigned)((J.threads + 255) / 256);
    const size_t rows_lds = sort_rows_lds_bytes(s.nb);
    const bool fused_rows = J.mode == MODE_ROWS && c->sort_rows_ok && rows_lds <= 160 * 1024 && estride <= 8 * (size_t)SORT_SL;
    skip = fused_rows ? J.skip : nullptr;    // the generic sort reads every digit, so nothing may be left unwritten there
    if (J.mode == MODE_SINGLE) LAUNCH(c, "k_digits_store", (k_digits_store<MODE_SINGLE>), gd, 256, J.da, s, dig, (const uint8_t*)nullptr);
    else LAUNCH(c, "k_digits_store", (k_digits_store<MODE_ROWS>), gd, 256, J.da, s, dig, skip);
    if (c->z_consumed && J.mode == MODE_ROWS) HIPCHK(c, hipEventRecord(c->z_consumed, c->stream));   // the scalars are not read again
    if (fused_rows) {
      ProfScope _ps(c, "k_sort_rows");
      hipLaunchKernelGGL(k_sort_rows, dim3((unsigned)J.P), dim3(1024), rows_lds, c->stream, (const dig_t*)dig, g, hist, offs, sorted, skip);
    } else {
      {
        ProfScope _ps(c, "k_hist_lds");
        hipLaunchKernelGGL(k_hist_lds, dim3(g.K, g.R, (unsigned)J.P), dim3(1024), (size_t)g.RS * 4, c->stream, (const dig_t*)dig, g, bh);
      }
      LAUNCH(c, "k_block_prefix", k_block_prefix, (unsigned)((NB + 255) / 256), 256, bh, g, NB, hist);
      LAUNCH(c, "k_scan", k_scan, (unsigned)J.P, 1024, hist, offs, s.nb);
      {
        ProfScope _ps(c, "k_scatter_lds");
        hipLaunchKernelGGL(k_scatter_lds, dim3(g.K, g.R, (unsigned)J.P), dim3(1024), (size_t)g.RS * 4, c->stream, (const dig_t*)dig, g, (const uint32_t*)bh, (const uint32_t*)offs, sorted);
      }
    }
  }
  launch_accumulate(c, J.points, NB, s.nb, estride, a, hist);
  store_last_acc(c, a);
  launch_reduce(c, J.P, s.nb, a, skip);
  LAUNCHCHK(c);
  return SBN_OK;
}

// A generator set may be shared by several contexts (one per host thread / stream); its lazily built tables (window, GLV) are guarded by
// one process-wide mutex (taken after the context's own, never the other way round).
static std::mutex g_bases_tables_mu;

// Whether a single MSM of n terms over the generator set b takes the GLV path (glv_kernels.cuh).  It needs the two-level sort for its 2n
// records and a handle (the table of images phi(P) is kept with it).  Automatic rule: glv_pays (msm_plan.hpp).
// SBN_MSM_GLV=0 / 1 (read when the context is created) switches it off / on wherever it can run; with it unset, an SBN_MSM_C experiment
// keeps the plain windows it asks for.
static bool glv_applies(const sbn_ctx* c, const MsmOverrides& o, const sbn_bases* b, size_t n, const MsmShape& plain) {
  if (!b || c->msm_glv == 0 || (c->msm_glv < 0 && o.c_set)) return false;
  const size_t npts = b->n + (b->has_h ? 1 : 0);
  if (2 * npts > 0x7fffffffull || !sort2_applies(c, MODE_SINGLE, 2 * n, S2_C_MIN)) return false;
  if (c->msm_glv == 1) return true;
  return glv_pays(o, n, plain);
}
// the GLV table of a generator set: its npts points, then phi of each (2 x npts x 64 B), built on the first GLV MSM and kept with the
// handle (the contexts that share a handle share one table; derived handles build their own)
static int bases_glv_table(sbn_ctx* c, const sbn_bases* b, const uint32_t** out) {
  std::lock_guard<std::mutex> tg(g_bases_tables_mu);
  if (b->d_glv) { *out = (const uint32_t*)b->d_glv; return SBN_OK; }
  const size_t npts = b->n + (b->has_h ? 1 : 0);
  void* tab = nullptr;
  hipError_t e = hipMalloc(&tab, 2 * npts * 64);
  if (e != hipSuccess) { (void)hipGetLastError(); return fail(c, SBN_ENOMEM, "hipMalloc GLV table (%zu B): %s", 2 * npts * 64, hipGetErrorString(e)); }
  LAUNCH(c, "k_glv_table", k_glv_table, (unsigned)((npts + 255) / 256), 256, (const uint32_t*)b->d_pts, npts, (uint32_t*)tab);
  hipError_t le = hipGetLastError();
  hipError_t se = hipStreamSynchronize(c->stream);
  if (le != hipSuccess || se != hipSuccess) { hipFree(tab); return fail(c, SBN_EHIP, "GLV table build: %s", hipGetErrorString(le != hipSuccess ? le : se)); }
  b->d_glv = tab;
  *out = (const uint32_t*)tab;
  return SBN_OK;
}

// The ONE plan of a single MSM of n terms (1 .. 2^31-1: the callers' check) over device-resident canonical scalars and Montgomery affine bases
// (b: the generator set d_bases belongs to, or null for points staged by the call — only a set keeps a GLV table): the window shape, the
// BucketJob and the GLV switch, with the table and the half-scalar buffer the GLV path allocates.  No launch of the job itself
static int msm_single_plan(sbn_ctx* c, const MsmOverrides& o, const uint32_t* d_scal, const uint32_t* d_bases, size_t n, const sbn_bases* b, BucketJob* out) {
  BucketJob J; memset(&J, 0, sizeof J);
  J.mode = MODE_SINGLE;
  {
    int cm = 1; while ((1 << cm) < c->sort_rs_max) cm++;
    const bool s2 = sort2_applies(c, MODE_SINGLE, n, S2_C_MIN);
    J.s = choose_shape(o, n, false, s2 ? S2_C_MAX : cm + 1, 1, s2 ? S2_C_MAX : MSM_C_MAX);
  }
  J.P = (size_t)J.s.W; J.threads = n; J.points = d_bases;
  J.da.scalars = d_scal; J.da.n = n; J.da.estride = n; J.da.bad = c->d_bad;
  if (glv_applies(c, o, b, n, J.s)) {
    int rc;
    const uint32_t* tab;
    if ((rc = bases_glv_table(c, b, &tab))) return rc;
    if ((rc = ensure(c, c->glv_scal, 2 * n * 16))) return rc;
    J.s = glv_shape(o, n); J.P = (size_t)J.s.W; J.threads = 2 * n; J.points = tab;
    J.da.scalars = (const uint32_t*)c->glv_scal.p; J.da.n = 2 * n; J.da.estride = 2 * n;
    J.glv = true; J.glv_gap = b->n + (b->has_h ? 1 : 0) - n;
  }
  *out = J;
  return SBN_OK;
}
// the planned job, launches only: the J.s.W window sums (XYZZ) stay in c->wsum.  k_glv_split counts scalars >= r into c->d_bad
static int msm_single_run(sbn_ctx* c, const MsmOverrides& o, const BucketJob& J, const uint32_t* d_scal, size_t n) {
  if (J.glv) LAUNCH(c, "k_glv_split", k_glv_split, (unsigned)((n + 255) / 256), 256, d_scal, n, (uint32_t*)c->glv_scal.p, c->d_bad);
  return run_bucket_job(c, J, o);
}
// plan and run, for a caller that hands the window sums over itself (the verifiers: abi_verify_common.inc); *shape: what fold_windows needs
static int msm_single_launch(sbn_ctx* c, const uint32_t* d_scal, const uint32_t* d_bases, size_t n, const sbn_bases* b, MsmShape* shape) {
  if (n == 0 || n > 0x7fffffffull) return fail(c, SBN_EINVAL, "msm: n=%zu is outside 1 .. 2^31-1", n);
  const MsmOverrides o = msm_overrides_read();
  BucketJob J;
  int rc;
  if ((rc = msm_single_plan(c, o, d_scal, d_bases, n, b, &J))) return rc;
  if ((rc = msm_single_run(c, o, J, d_scal, n))) return rc;
  *shape = J.s;
  return SBN_OK;
}
// sum_w 2^(c w) S_w over W window sums as the device left them: the 254-doubling serial chain, on the host.  The one fold of every bucket job's
// and every k_window_sums launch's sums
static sbn_host::Pt fold_windows(const sbn_host::Pt* S, int W, int c) {
  std::vector<sbn_host::Pt> T((size_t)W);
  for (int w = 0; w < W; w++) T[(size_t)w] = sbn_host::pt_from_device(S[w]);
  return sbn_host::combine_windows(T.data(), W, c);
}

// MSM over device-resident canonical scalars and Montgomery affine bases -> canonical affine bytes on the host (b: as msm_single_plan takes it)
static int msm_device(sbn_ctx* c, const uint32_t* d_scal, const uint32_t* d_bases, size_t n, uint8_t out_xy[64], int* out_is_inf, const sbn_bases* b = nullptr) {
  if (n == 0) { memset(out_xy, 0, 64); if (out_is_inf) *out_is_inf = 1; return SBN_OK; }
  if (n > 0x7fffffffull) return fail(c, SBN_EINVAL, "msm: n=%zu exceeds 2^31-1", n);
  const MsmOverrides o = msm_overrides_read();
  BucketJob J;
  int rc;
  if ((rc = msm_single_plan(c, o, d_scal, d_bases, n, b, &J))) return rc;
  if ((rc = ensure_pin(c, std::max<size_t>(4096, J.P * 128)))) return rc;      // sized from the shape the plan ends up with
  if ((rc = input_check_begin(c))) return rc;                                   // ahead of k_glv_split, which counts into c->d_bad
  if ((rc = msm_single_run(c, o, J, d_scal, n))) return rc;
  HIPCHK(c, hipMemcpyAsync(c->pin, c->wsum.p, J.P * 128, hipMemcpyDeviceToHost, c->stream));
  if ((rc = input_check_fetch(c))) return rc;
  HIPCHK(c, hipStreamSynchronize(c->stream));
  if (c->prof) prof_drain(c);
  if ((rc = input_check_end(c))) return rc;
  sbn_host::to_affine_bytes(fold_windows((const sbn_host::Pt*)c->pin, J.s.W, J.s.c), out_xy, out_is_inf);
  return SBN_OK;
}

// window table 2^(c w) * P_j of a generator set, built on first use for a given c and kept with the handle
static int bases_window_table(sbn_ctx* c, const sbn_bases* b, const MsmShape& s, const uint32_t** out) {
  std::lock_guard<std::mutex> tg(g_bases_tables_mu);
  auto it = b->tables.find(s.c);
  if (it != b->tables.end()) { *out = (const uint32_t*)it->second; return SBN_OK; }
  const size_t npts = b->n + (b->has_h ? 1 : 0);
  const size_t tot = npts * (size_t)s.W;
  int rc;
  if ((rc = ensure(c, c->gen_tmp, tot * 128))) return rc;
  void* tab = nullptr;
  hipError_t e = hipMalloc(&tab, tot * 64);
  if (e != hipSuccess) return fail(c, SBN_ENOMEM, "hipMalloc window table (%zu B): %s", tot * 64, hipGetErrorString(e));
  LAUNCH(c, "k_window_table", k_window_table, (unsigned)((npts + 63) / 64), 64, (const uint32_t*)b->d_pts, npts, s.c, s.W, (uint32_t*)c->gen_tmp.p);
  LAUNCH(c, "k_xyzz_to_affine", k_xyzz_to_affine, (unsigned)((tot + 63) / 64), 64, (const uint32_t*)c->gen_tmp.p, (uint32_t*)tab, (uint32_t*)nullptr, (uint8_t*)nullptr, tot);
  LAUNCHCHK(c);
  HIPCHK(c, hipStreamSynchronize(c->stream));
  b->tables[s.c] = tab;
  *out = (const uint32_t*)tab;
  return SBN_OK;
}

// Direct-lookup table of a generator set (comb_kernels.cuh): the largest window c <= COMB_C_MAX (17) whose table fits `max_bytes`.
static int bases_build_comb(sbn_ctx* c, sbn_bases* b, size_t max_bytes) {
  const size_t npts = b->n + (b->has_h ? 1 : 0);
  if (npts == 0) return fail(c, SBN_EINVAL, "precompute: empty generator set");
  int cc = 0; size_t bytes = 0;
  for (int t = COMB_C_MAX; t >= 7; t--) {
    const MsmShape s = make_shape(t);
    const size_t need = npts * (size_t)s.W * (size_t)s.nb * 64;
    if (need <= max_bytes) { cc = t; bytes = need; break; }
  }
  if (!cc) return fail(c, SBN_EINVAL, "precompute: even the c = 7 table (%zu B) exceeds the budget of %zu B", npts * (size_t)make_shape(7).W * 64 * 64, max_bytes);
  {
    std::lock_guard<std::mutex> tg(g_bases_tables_mu);
    if (b->d_comb && b->comb_c == cc) return SBN_OK;
  }
  const MsmShape s = make_shape(cc);
  int rc; const uint32_t* wtab;
  if ((rc = bases_window_table(c, b, s, &wtab))) return rc;
  std::lock_guard<std::mutex> tg(g_bases_tables_mu);
  if (b->d_comb) { HIPCHK(c, hipStreamSynchronize(c->stream)); hipFree(b->d_comb); b->d_comb = nullptr; b->comb_c = 0; }
  void* tab = nullptr;
  hipError_t e = hipMalloc(&tab, bytes);
  if (e != hipSuccess) { (void)hipGetLastError(); return fail(c, SBN_ENOMEM, "hipMalloc lookup table (%zu B): %s", bytes, hipGetErrorString(e)); }
  const size_t slab_lanes = npts * ((size_t)s.nb / COMB_CH);
  const size_t BL = std::min<size_t>(slab_lanes, (size_t)1 << 18);
  void* tx = nullptr; void* tp = nullptr;
  if ((e = hipMalloc(&tx, BL * COMB_CH * 128)) != hipSuccess || (e = hipMalloc(&tp, BL * COMB_CH * 32)) != hipSuccess) {
    (void)hipGetLastError(); hipFree(tab); if (tx) hipFree(tx);
    return fail(c, SBN_ENOMEM, "hipMalloc lookup-table build scratch: %s", hipGetErrorString(e));
  }
  for (int w = 0; w < s.W; w++)
    for (size_t l0 = 0; l0 < slab_lanes; l0 += BL) {
      const size_t lanes = std::min(BL, slab_lanes - l0);
      LAUNCH(c, "k_comb_build", k_comb_build, (unsigned)((lanes + 63) / 64), 64, wtab + 16 * ((size_t)w * npts), npts, cc, l0, lanes, (uint32_t*)tx, (uint32_t*)tp,
             (uint32_t*)tab + 16 * (((size_t)w * npts) << (cc - 1)));
    }
  hipError_t le = hipGetLastError();
  hipError_t se = hipStreamSynchronize(c->stream);
  hipFree(tx); hipFree(tp);
  if (le != hipSuccess || se != hipSuccess) { hipFree(tab); return fail(c, SBN_EHIP, "lookup-table build: %s", hipGetErrorString(le != hipSuccess ? le : se)); }
  if (c->prof) prof_drain(c);
  b->d_comb = tab; b->comb_c = cc; b->comb_bytes = bytes;
  return SBN_OK;
}

// Hyrax row commits on device-resident canonical scalars (hyrax.rs:253-267 -> commitments.rs:144-154)
// launches only (no host synchronisation): row commitments as canonical affine bytes + infinity flags in DEVICE buffers
// (d_xy == nullptr: stop before the conversion and leave the L sums as XYZZ in c->wsum)
// A merged matrix (the recursive call of the duplicate-bases path) comes with per-row flags: 0 ordinary, 1 constant, 2 all-zero.
struct RowInfo {
  const uint8_t* flags = nullptr;   // null: no information
  bool skip_zero = false;           // no blinds: an all-zero row is the identity and needs no work at all
  size_t col_value = ~(size_t)0, col_blind = ~(size_t)0;   // the only columns a flagged row can be non-zero in
  bool internal_rows = false;       // rows written by this library (bullet rounds): canonical and never constant, so the pass that
                                    // classifies rows and checks the caller's scalars is skipped
  bool mont_scalars = false;        // dZ / dBl are table values (Montgomery R = 2^261, lazy): only with merged bases — the merge converts on the way out
};
static int commit_rows_launch(sbn_ctx* c, const sbn_bases* b, const uint32_t* dZ, const uint32_t* dBl, size_t L, size_t R, uint32_t* d_xy, uint8_t* d_inf, const RowInfo& ri = RowInfo()) {
  if (L == 0) return SBN_OK;
  const uint8_t* skip_rows = ri.skip_zero ? ri.flags : nullptr;
  if (b->uniq) {
    // merge the scalars of equal bases, then commit over the unique bases (no blind column: h is merged like any base)
    const size_t U = b->U; int rc;
    if ((rc = ensure(c, c->merged, L * (U + 1) * 32 + L))) return rc;
    uint32_t* m = (uint32_t*)c->merged.p; uint8_t* rowflags = (uint8_t*)c->merged.p + L * (U + 1) * 32;
    if (ri.internal_rows) rowflags = nullptr;          // no classification pass, no flags to clear (a 1-byte fill was a launch of its own)
    else if (R) LAUNCH(c, "k_merge_scalars", k_row_const_flags, (unsigned)L, 256, dZ, dBl, R, rowflags, ri.mont_scalars ? (uint32_t*)nullptr : c->d_bad);
    else HIPCHK(c, hipMemsetAsync(rowflags, 0, L, c->stream));
    {
      const size_t nsmall = (L * (U + 1) + 255) / 256, nbigb = L * (size_t)b->nbig;
      if (nsmall + nbigb > 0x7fffffffull) return fail(c, SBN_EINVAL, "commit: merge grid too large");
      LAUNCH(c, "k_merge_scalars", k_merge, (unsigned)(nsmall + nbigb), 256, dZ, dBl, L, R, U, (const uint32_t*)b->d_csr_off, (const uint32_t*)b->d_csr_cols, MERGE_BIG,
             (const uint32_t*)b->d_big, b->nbig, (const uint8_t*)rowflags, b->hcol, m, ri.mont_scalars ? 1 : 0, (uint32_t)nsmall);
    }
    if (c->z_consumed) HIPCHK(c, hipEventRecord(c->z_consumed, c->stream));      // Z (and the blinds) are not read after this point
    RowInfo info; info.flags = rowflags; info.skip_zero = dBl == nullptr;      // with blinds a zero row still commits to blind*h
    info.col_value = U; info.col_blind = (dBl && b->hcol <= U) ? (size_t)b->hcol : ~(size_t)0;
    return commit_rows_launch(c, b->uniq, m, nullptr, L, U + 1, d_xy, d_inf, info);
  }
  if (ri.mont_scalars) return fail(c, SBN_EINVAL, "commit: internal: Montgomery scalars without merged bases");
  const MsmOverrides o = msm_overrides_read();
  const size_t ncol = R + (dBl ? 1 : 0);
  if (ncol == 0) {
    if (!d_xy) { int rc0; if ((rc0 = ensure(c, c->wsum, L * 128))) return rc0; HIPCHK(c, hipMemsetAsync(c->wsum.p, 0, L * 128, c->stream)); return SBN_OK; }
    HIPCHK(c, hipMemsetAsync(d_xy, 0, 64 * L, c->stream)); HIPCHK(c, hipMemsetAsync(d_inf, 1, L, c->stream)); return SBN_OK;
  }
  const size_t npts = b->n + (b->has_h ? 1 : 0);
  if (b->d_comb) {
    // fixed-base lookup: W mixed additions per scalar, no buckets (comb_kernels.cuh)
    const MsmShape s = make_shape(b->comb_c);
    DigitArgs da; memset(&da, 0, sizeof da);
    da.scalars = dZ; da.blinds = dBl; da.n = ncol; da.R = R; da.L = L; da.tstride = npts; da.bad = c->d_bad;
    const unsigned S = comb_split(L, ncol, s.W, o);       // blocks per row
    int rc;
    if ((rc = ensure(c, c->wsum, L * 128))) return rc;
    if ((rc = ensure(c, c->comb_partial, S > 1 ? L * S * 128 : L * 257 * 128))) return rc;
    if (L > 0x7fffffffull || ncol * (size_t)s.W > 0x7fffffffull) return fail(c, SBN_EINVAL, "commit: too many rows / columns");
    c->last_job[0] = (uint64_t)s.c; c->last_job[1] = (uint64_t)s.W; c->last_job[2] = (uint64_t)(L * ncol * (size_t)s.W); c->last_job[3] = 0;
    if (S > 1) {
      LAUNCH(c, "k_comb_rows", k_comb_rows_flat, dim3((unsigned)L, S), 256, (const uint32_t*)b->d_comb, da, s, skip_rows, (uint32_t*)c->comb_partial.p);
      LAUNCH(c, "k_comb_fold", k_comb_fold, (unsigned)L, S > 64 ? 128 : 64, (const uint32_t*)c->comb_partial.p, S, (uint32_t*)c->wsum.p, (const uint8_t*)nullptr, (const uint32_t*)nullptr);
    } else {
      // ordinary rows: one block each; flagged (constant / zero) rows: one wave each over their one or two live columns
      const uint8_t* fl = (ri.flags && ri.col_value != ~(size_t)0) ? ri.flags : nullptr;
      uint32_t* sparse = (uint32_t*)c->comb_partial.p + (size_t)32 * L * 256;
      LAUNCH(c, "k_comb_rows", k_comb_rows, dim3((unsigned)L, 1), 256, (const uint32_t*)b->d_comb, da, s, fl, (uint32_t*)c->comb_partial.p);
      if (fl) LAUNCH(c, "k_comb_rows_const", k_comb_rows_const, (unsigned)L, 64, (const uint32_t*)b->d_comb, da, s, fl, ri.skip_zero ? 1 : 0, ri.col_value, ri.col_blind, sparse);
      LAUNCH(c, "k_comb_fold", k_comb_fold, (unsigned)L, 64, (const uint32_t*)c->comb_partial.p, 256u, (uint32_t*)c->wsum.p, fl, (const uint32_t*)sparse);
    }
    if (c->z_consumed) HIPCHK(c, hipEventRecord(c->z_consumed, c->stream));
    if (d_xy) LAUNCH(c, "k_xyzz_to_affine", k_xyzz_to_affine, (unsigned)((L + 63) / 64), 64, (const uint32_t*)c->wsum.p, (uint32_t*)nullptr, d_xy, d_inf, L);
    LAUNCHCHK(c);
    return SBN_OK;
  }
  BucketJob J; memset(&J, 0, sizeof J);
  J.mode = MODE_ROWS; J.s = choose_shape(o, ncol, true, 16, L); J.P = L; J.threads = L * ncol;
  if ((size_t)J.s.W * npts > 0x7fffffffull) return fail(c, SBN_EINVAL, "commit: table index overflow");
  int rc; const uint32_t* tab;
  if ((rc = bases_window_table(c, b, J.s, &tab))) return rc;
  J.points = tab;
  J.da.scalars = dZ; J.da.blinds = dBl; J.da.n = ncol; J.da.R = R; J.da.L = L; J.da.tstride = npts; J.da.estride = ncol * (size_t)J.s.W; J.da.bad = c->d_bad;
  J.skip = skip_rows;
  if ((rc = run_bucket_job(c, J, o))) return rc;
  if (d_xy) LAUNCH(c, "k_xyzz_to_affine", k_xyzz_to_affine, (unsigned)((L + 63) / 64), 64, (const uint32_t*)c->wsum.p, (uint32_t*)nullptr, d_xy, d_inf, L);
  LAUNCHCHK(c);
  return SBN_OK;
}
// Hyrax row commits on device-resident canonical scalars (hyrax.rs:253-267 -> commitments.rs:144-154)
static int commit_rows_device(sbn_ctx* c, const sbn_bases* b, const uint32_t* dZ, const uint32_t* dBl, size_t L, size_t R, uint8_t* out_xy, uint8_t* out_inf, const RowInfo& ri = RowInfo()) {
  if (L == 0) return SBN_OK;
  int rc;
  if ((rc = input_check_begin(c))) return rc;
  if (L <= 16) {
    // a handful of rows: the per-row Fermat inversion is a ~0.3 ms single-lane chain on the device and ~15 us on a host core
    // the sums and the input-check counter go straight into the host mailbox, flag behind them (the sumcheck rounds' protocol):
    // one small launch and a poll instead of two copies and a stream synchronisation — a bullet round commits 2 rows at a time
    if ((rc = sc_tickets(c))) return rc;
    if ((rc = commit_rows_launch(c, b, dZ, dBl, L, R, nullptr, nullptr, ri))) return rc;
    const uint32_t seq = ++c->mbox_seq;
    uint32_t* hfin = c->mbox + SC_MBOX_FINALS;
    static_assert(16 * 32 + 1 <= SC_MBOX_WORDS - SC_MBOX_FINALS, "mailbox: 16 XYZZ sums + the counter must fit the final-claims area");
    LAUNCH(c, "k_points_to_host", k_sc_finals_raw, 1, 256, (const uint32_t*)c->wsum.p, (uint32_t)(L * 32), (const uint32_t*)c->d_bad, hfin, c->mbox + SC_MBOX_FLAGS + SC_PACK_MAX, seq);
    LAUNCHCHK(c);
    if ((rc = sc_flag_wait(c, c->mbox + SC_MBOX_FLAGS + SC_PACK_MAX, seq))) return rc;
    *c->h_bad = hfin[L * 32];
    if ((rc = input_check_end(c))) return rc;
    sbn_host::Pt S[16]; memcpy(S, hfin, L * 128);
    for (size_t i = 0; i < L; i++) { int inf = 0; sbn_host::to_affine_bytes(sbn_host::pt_from_device(S[i]), out_xy + 64 * i, &inf); if (out_inf) out_inf[i] = (uint8_t)inf; }
    return SBN_OK;
  }
  if ((rc = ensure(c, c->out_small, L * 65))) return rc;
  if ((rc = ensure_pin(c, std::max<size_t>(4096, L * 65)))) return rc;
  if ((rc = commit_rows_launch(c, b, dZ, dBl, L, R, (uint32_t*)c->out_small.p, (uint8_t*)c->out_small.p + L * 64, ri))) return rc;
  HIPCHK(c, hipMemcpyAsync(c->pin, c->out_small.p, L * 65, hipMemcpyDeviceToHost, c->stream));
  if ((rc = input_check_fetch(c))) return rc;
  HIPCHK(c, hipStreamSynchronize(c->stream));
  if (c->prof) prof_drain(c);
  if ((rc = input_check_end(c))) return rc;
  memcpy(out_xy, c->pin, L * 64);
  if (out_inf) memcpy(out_inf, (uint8_t*)c->pin + L * 64, L);
  return SBN_OK;
}

static int stage_scalars(sbn_ctx* c, const uint8_t* host_scalars, size_t n, uint32_t flags, const uint32_t** d_out) {
  int rc;
  if ((rc = ensure(c, c->stage_scal, n * 32))) return rc;
  HIPCHK(c, hipMemcpyAsync(c->stage_scal.p, host_scalars, n * 32, hipMemcpyHostToDevice, c->stream));
  if (flags & SBN_SCALARS_MONT) {
    if ((rc = ensure(c, c->scal_canon, n * 32))) return rc;
    LAUNCH(c, "k_scalars_from_mont", k_scalars_from_mont, (unsigned)((n + 255) / 256), 256, (const uint32_t*)c->stage_scal.p, (uint32_t*)c->scal_canon.p, n);
    *d_out = (const uint32_t*)c->scal_canon.p;
  } else *d_out = (const uint32_t*)c->stage_scal.p;
  return SBN_OK;
}
static int canon_scalars_dev(sbn_ctx* c, const void* d_scalars, size_t n, uint32_t flags, const uint32_t** d_out) {
  if (flags & SBN_SCALARS_MONT) {
    int rc; if ((rc = ensure(c, c->scal_canon, n * 32))) return rc;
    LAUNCH(c, "k_scalars_from_mont", k_scalars_from_mont, (unsigned)((n + 255) / 256), 256, (const uint32_t*)d_scalars, (uint32_t*)c->scal_canon.p, n);
    *d_out = (const uint32_t*)c->scal_canon.p;
  } else *d_out = (const uint32_t*)d_scalars;
  return SBN_OK;
}

// Detect equal bases (keys: one byte string per point, equal keys <=> equal points) and, when enough of them repeat, attach
// the unique-point table + CSR column lists used by the commit path.
static int bases_build_dedupe(sbn_ctx* c, sbn_bases* b, const std::vector<std::string>& keys) {
  const size_t tot = keys.size();
  std::unordered_map<std::string, uint32_t> idx;
  std::vector<uint32_t> umap(tot);
  std::vector<uint32_t> first_col;
  for (size_t j = 0; j < tot; j++) {
    auto it = idx.find(keys[j]);
    if (it == idx.end()) { uint32_t u = (uint32_t)first_col.size(); idx.emplace(keys[j], u); first_col.push_back((uint32_t)j); umap[j] = u; }
    else umap[j] = it->second;
  }
  const size_t U = first_col.size();
  if (U * 10 > tot * 9) return SBN_OK;         // < 10 % repeats: not worth the extra pass
  std::vector<uint32_t> off(U + 1, 0), cols(tot), big;
  for (size_t j = 0; j < tot; j++) off[umap[j] + 1]++;
  for (size_t u = 0; u < U; u++) off[u + 1] += off[u];
  { std::vector<uint32_t> cur(off.begin(), off.end() - 1); for (size_t j = 0; j < tot; j++) cols[cur[umap[j]]++] = (uint32_t)j; }
  for (size_t u = 0; u < U; u++) if (off[u + 1] - off[u] > MERGE_BIG) big.push_back((uint32_t)u);
  // the unique table carries one extra point: S = sum of the n bases (h excluded), the base of constant rows
  sbn_bases* q = new sbn_bases(); q->n = U + 1; q->has_h = false;
  hipError_t e = hipMalloc(&q->d_pts, (U + 1) * 64);
  if (e != hipSuccess) { delete q; return fail(c, SBN_ENOMEM, "hipMalloc unique bases: %s", hipGetErrorString(e)); }
  for (size_t u = 0; u < U; u++)
    HIPCHK(c, hipMemcpyAsync((uint8_t*)q->d_pts + 64 * u, (const uint8_t*)b->d_pts + 64 * (size_t)first_col[u], 64, hipMemcpyDeviceToDevice, c->stream));
  auto up = [&](void** dst, const std::vector<uint32_t>& v) -> int {
    hipError_t e2 = hipMalloc(dst, std::max<size_t>(4, v.size() * 4)); if (e2 != hipSuccess) return SBN_ENOMEM;
    if (!v.empty() && hipMemcpy(*dst, v.data(), v.size() * 4, hipMemcpyHostToDevice) != hipSuccess) return SBN_EHIP;
    return SBN_OK;
  };
  HIPCHK(c, hipStreamSynchronize(c->stream));
  int rc;
  if ((rc = up(&b->d_csr_off, off)) || (rc = up(&b->d_csr_cols, cols)) || (rc = up(&b->d_big, big))) { sbn_bases_free(c, q); return fail(c, rc, "dedupe tables"); }
  b->uniq = q; b->U = U; b->nbig = (uint32_t)big.size();
  b->hcol = (b->has_h) ? umap[tot - 1] : (uint32_t)(U + 1);
  // S = sum_u mult_u * U_u with mult_u = number of G columns (index < n) that map to u: a U-term MSM with tiny scalars
  {
    const size_t n = b->n;
    std::vector<uint8_t> mult(U * 32, 0);
    for (size_t j = 0; j < n; j++) { uint32_t* m = (uint32_t*)&mult[32 * umap[j]]; m[0] += 1; }
    int rc2;
    if ((rc2 = ensure(c, c->stage_scal, U * 32))) return rc2;
    HIPCHK(c, hipMemcpyAsync(c->stage_scal.p, mult.data(), U * 32, hipMemcpyHostToDevice, c->stream));
    uint8_t sxy[64]; int sinf = 0;
    if ((rc2 = msm_device(c, (const uint32_t*)c->stage_scal.p, (const uint32_t*)q->d_pts, U, sxy, &sinf))) return rc2;
    uint8_t sm[64]; memset(sm, 0, 64);
    if (!sinf) memcpy(sm, sxy, 64);                  // canonical x || y; the device brings it to its Montgomery form (infinity stays all-zero)
    HIPCHK(c, hipMemcpy((uint8_t*)q->d_pts + 64 * U, sm, 64, hipMemcpyHostToDevice));
    LAUNCH(c, "k_points_to_mont", k_points_to_mont, 1, 256, (const uint32_t*)q->d_pts + 16 * U, (uint32_t*)q->d_pts + 16 * U, (size_t)1);
    LAUNCHCHK(c);
    HIPCHK(c, hipStreamSynchronize(c->stream));
  }
  return SBN_OK;
}
