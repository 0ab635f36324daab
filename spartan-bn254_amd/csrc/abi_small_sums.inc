// abi_small_sums.inc — C ABI: many short sums of fresh points in ONE launch (small_sum_kernels.cuh).  sbn_g1_small_sums is what a verifier's
// handful-of-terms equations want in place of one bucket pipeline each (DESIGN §4.5 item 3: any MSM of 2^10 .. 2^15 terms costs the same 0.48 ms,
// and one of 30 terms little less): one upload, one k_window_sums launch over every (sum, window), one hand-over, and the 252-doubling fold of the
// 64 window sums on the host, where the bucket pipeline's fold runs as well (verify_fold_windows).  No table of 2^k P is built (§4.18's costs a
// 253-doubling chain per call and pays when points repeat across sums; here they do not).
// Included by sbn254.hip.

static const size_t SS_SUMS_MAX = 256;
static const uint32_t SBOX_FLAG_WORDS = 256;      // one flag per block of k_sums_to_host, in front of the sums
static_assert(SS_SUMS_MAX * SS_WINDOWS <= (size_t)SBOX_FLAG_WORDS * SS_HANDOVER_POINTS, "a flag for every hand-over block");

// the hand-over area of the window sums, sized on first use and grown when a call brings more: vbox holds 64 points, a call here up to 256 x 64
static int sbox_ensure(sbn_ctx* c, size_t npoints) {
  const size_t words = SBOX_FLAG_WORDS + 32 * npoints;
  if (words <= c->sbox_words) return SBN_OK;
  if (c->sbox) { HIPCHK(c, hipStreamSynchronize(c->stream)); HIPCHK(c, hipHostFree(c->sbox)); c->sbox = nullptr; c->sbox_words = 0; }
  uint32_t* sb = nullptr;
  HIPCHK(c, hipHostMalloc((void**)&sb, words * 4, hipHostMallocMapped | hipHostMallocCoherent));
  memset(sb, 0, words * 4);
  c->sbox = sb; c->sbox_words = words;
  return SBN_OK;
}
// `npoints` XYZZ sums at d_sums to the host in ONE launch (sums_handover_begin) and ONE wait (sums_handover_wait); *out: the sums as the device left
// them, valid until the next hand-over.  Between the two a caller may enqueue work that the host does not wait for
static int sums_handover_begin(sbn_ctx* c, const uint32_t* d_sums, size_t npoints, uint32_t* seq_out) {
  int rc;
  const size_t nblk = (npoints + SS_HANDOVER_POINTS - 1) / SS_HANDOVER_POINTS;
  if (npoints == 0 || nblk > (size_t)SBOX_FLAG_WORDS) return fail(c, SBN_EINVAL, "small sums: %zu points do not fit the hand-over area", npoints);
  if ((rc = sbox_ensure(c, npoints))) return rc;
  const uint32_t seq = ++c->mbox_seq;
  LAUNCH(c, "k_sums_to_host", k_sums_to_host, (unsigned)nblk, 256, (const uint4*)d_sums, (uint32_t)(8 * npoints), (uint4*)(c->sbox + SBOX_FLAG_WORDS), c->sbox, seq);
  LAUNCHCHK(c);
  *seq_out = seq;
  return SBN_OK;
}
static int sums_handover_wait(sbn_ctx* c, size_t npoints, uint32_t seq, const sbn_host::Pt** out) {
  const size_t nblk = (npoints + SS_HANDOVER_POINTS - 1) / SS_HANDOVER_POINTS;
  // a short spin on the flags (a count of polls, not a time: enough for a call of a few sums, whose kernel is tens of microseconds), then the
  // ordinary stream synchronisation, which is the normal path of a large call (256 sums: 2.3 ms of kernel) and of every call with profiling on
  volatile uint32_t* fl = c->sbox;
  bool seen = false;
  if (!c->prof) {
    for (int spin = 0; spin < 200000 && !seen; spin++) {
      size_t done = 0; while (done < nblk && fl[done] == seq) done++;
      if (done == nblk) { std::atomic_thread_fence(std::memory_order_acquire); seen = true; }
    }
  }
  if (!seen) {
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (c->prof) prof_drain(c);
    for (size_t i = 0; i < nblk; i++) if (fl[i] != seq) return fail(c, SBN_EHIP, "small sums: result flag %zu missing after synchronisation", i);
  }
  *out = (const sbn_host::Pt*)(c->sbox + SBOX_FLAG_WORDS);
  return SBN_OK;
}
static int sums_handover(sbn_ctx* c, const uint32_t* d_sums, size_t npoints, const sbn_host::Pt** out) {
  int rc; uint32_t seq = 0;
  if ((rc = sums_handover_begin(c, d_sums, npoints, &seq))) return rc;
  return sums_handover_wait(c, npoints, seq, out);
}
// sum_w 16^w S_w of one sum's 64 window sums as the device left them
static sbn_host::Pt small_sum_fold(const sbn_host::Pt* S) {
  sbn_host::Pt W[SS_WINDOWS];
  for (int w = 0; w < SS_WINDOWS; w++) W[w] = sbn_host::pt_from_device(S[w]);
  return sbn_host::combine_windows(W, SS_WINDOWS, SS_WINDOW_BITS);
}
// a canonical coordinate in the device's Montgomery form (R = 2^261), canonical again: a generator table's entry (k_points_to_mont)
static sbn_host::Fq fq_to_dev_mont(const uint8_t b[32]) {
  sbn_host::Fq x; memcpy(x.v, b, 32);
  const sbn_host::Fq k32 = {{32, 0, 0, 0}};
  return sbn_host::mul(sbn_host::to_mont(x), sbn_host::to_mont(k32));
}

extern "C" {

int sbn_g1_small_sums(sbn_ctx* c, const uint8_t* points_xy, const uint8_t* scalars, const uint32_t* counts, size_t nsums, uint8_t* out_xy, uint8_t* out_is_inf) {
  if (!c) return SBN_EINVAL;
  if (nsums == 0) return SBN_OK;
  if (!points_xy || !scalars || !counts || !out_xy) return fail(c, SBN_EINVAL, "small sums: a null pointer with %zu sums", nsums);
  if (nsums > SS_SUMS_MAX) return fail(c, SBN_EINVAL, "small sums: %zu sums in one call (at most %zu)", nsums, SS_SUMS_MAX);
  size_t total = 0;
  for (size_t i = 0; i < nsums; i++) {
    if (counts[i] > (uint32_t)SS_TERMS_MAX) return fail(c, SBN_EINVAL, "small sums: sum %zu has %u terms (at most %d)", i, counts[i], SS_TERMS_MAX);
    total += counts[i];
  }
  for (size_t j = 0; j < total; j++) {
    if (!fr_canonical(scalars + 32 * j)) return fail(c, SBN_EINVAL, "small sums: scalar %zu is not canonical  [scalar.rs:87-95]", j);
    if (!g1_xy_valid(points_xy + 64 * j)) return fail(c, SBN_EINVAL, "small sums: point %zu is not a canonical point of the curve", j);
  }
  // one staging block, one copy: the descriptors, then the points in table layout.  Built, like the checks above and the folds below, outside the
  // context's mutex: at the cap this host work is nine tenths of the call (DESIGN §4.19) and must not keep other threads off the device
  const size_t desc_bytes = 4 * (size_t)SS_DESC_WORDS * nsums, o_pts = desc_bytes, o_out = (o_pts + 64 * total + 255) / 256 * 256, bytes = o_out + 128 * (size_t)SS_WINDOWS * nsums;
  std::vector<uint32_t> stage((o_pts + 64 * total) / 4, 0u);
  uint32_t* h = stage.data();
  size_t at = 0;
  for (size_t i = 0; i < nsums; i++) {
    uint32_t* d = h + (size_t)SS_DESC_WORDS * i;
    d[0] = counts[i];
    for (uint32_t t = 0; t < counts[i]; t++, at++) {
      d[SS_DESC_IDX + t] = (uint32_t)at;                             // (below `total`, the number of points uploaded)
      memcpy(d + SS_DESC_SCAL + 8 * t, scalars + 32 * at, 32);
      const sbn_host::Fq x = fq_to_dev_mont(points_xy + 64 * at), y = fq_to_dev_mont(points_xy + 64 * at + 32);
      memcpy((uint8_t*)h + o_pts + 64 * at, x.v, 32); memcpy((uint8_t*)h + o_pts + 64 * at + 32, y.v, 32);
    }
  }
  std::vector<sbn_host::Pt> sums(nsums * (size_t)SS_WINDOWS);
  {
    std::lock_guard<std::mutex> g(c->mu); hipSetDevice(c->device);
    int rc;
    if ((rc = ensure_pin(c, 4 * stage.size()))) return rc;
    memcpy(c->pin, h, 4 * stage.size());
    void* slab = nullptr; size_t slab_bytes = 0;
    hipError_t e = pool_get(c, bytes, &slab, &slab_bytes);
    if (e != hipSuccess) return fail(c, SBN_ENOMEM, "hipMalloc small sums state: %s", hipGetErrorString(e));
    struct Drop { sbn_ctx* c; void* p; size_t b; ~Drop() { hipStreamSynchronize(c->stream); pool_put(c, p, b); } } drop{c, slab, slab_bytes};
    uint8_t* p0 = (uint8_t*)slab;
    HIPCHK(c, hipMemcpyAsync(p0, c->pin, 4 * stage.size(), hipMemcpyHostToDevice, c->stream));
    LAUNCH(c, "k_window_sums", k_window_sums, (unsigned)(nsums * SS_WINDOWS), 256, (const uint32_t*)p0, (const uint32_t*)(p0 + o_pts), (uint32_t*)(p0 + o_out));
    const sbn_host::Pt* S = nullptr;
    if ((rc = sums_handover(c, (const uint32_t*)(p0 + o_out), sums.size(), &S))) return rc;
    memcpy(sums.data(), S, sums.size() * sizeof(sbn_host::Pt));     // out of the context's area: the next call may overwrite it once the mutex is free
  }
  for (size_t i = 0; i < nsums; i++) {
    int inf = 0;
    sbn_host::to_affine_bytes(small_sum_fold(sums.data() + (size_t)SS_WINDOWS * i), out_xy + 64 * i, &inf);
    if (out_is_inf) out_is_inf[i] = (uint8_t)inf;
  }
  return SBN_OK;
}

}  // extern "C"
