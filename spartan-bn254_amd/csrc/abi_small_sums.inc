// abi_small_sums.inc — C ABI: many short sums of fresh points in ONE launch (small_sum_kernels.cuh).  sbn_g1_small_sums is what a verifier's
// handful-of-terms equations want in place of one bucket pipeline each (DESIGN §4.5 item 3: any MSM of 2^10 .. 2^15 terms costs the same 0.48 ms,
// and one of 30 terms little less): one upload, one k_window_sums launch over every (sum, window), one hand-over, and the 252-doubling fold of the
// 64 window sums on the host, where the bucket pipeline's fold runs as well (fold_windows, msm_host.hpp).  No table of 2^k P is built (§4.18's costs a
// 253-doubling chain per call and pays when points repeat across sums; here they do not).
// The hand-over (sums_handover) is abi_verify_common.inc, the point checks and fq_to_dev_mont verify_host.hpp.
// Included by sbn254.hip; needs abi_verify_common.inc.

static const size_t SS_SUMS_MAX = 256;
static_assert(SS_SUMS_MAX * SS_WINDOWS <= (size_t)SBOX_FLAG_WORDS * SS_HANDOVER_POINTS, "a flag for every hand-over block");

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
    SlabLease slab(c);
    if ((rc = slab.get(bytes, "small sums state"))) return rc;
    uint8_t* p0 = (uint8_t*)slab.p;
    HIPCHK(c, hipMemcpyAsync(p0, c->pin, 4 * stage.size(), hipMemcpyHostToDevice, c->stream));
    LAUNCH(c, "k_window_sums", k_window_sums, (unsigned)(nsums * SS_WINDOWS), 256, (const uint32_t*)p0, (const uint32_t*)(p0 + o_pts), (uint32_t*)(p0 + o_out));
    const sbn_host::Pt* S = nullptr;
    if ((rc = sums_handover(c, (const uint32_t*)(p0 + o_out), sums.size(), &S))) return rc;
    memcpy(sums.data(), S, sums.size() * sizeof(sbn_host::Pt));     // out of the context's area: the next call may overwrite it once the mutex is free
  }
  for (size_t i = 0; i < nsums; i++) {
    int inf = 0;
    sbn_host::to_affine_bytes(fold_windows(sums.data() + (size_t)SS_WINDOWS * i, SS_WINDOWS, SS_WINDOW_BITS), out_xy + 64 * i, &inf);
    if (out_is_inf) out_is_inf[i] = (uint8_t)inf;
  }
  return SBN_OK;
}

}  // extern "C"
