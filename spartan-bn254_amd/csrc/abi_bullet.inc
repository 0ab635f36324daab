// abi_bullet.inc — the vector / group work of BulletReductionProof::prove (nizk/bullet.rs:41-126) as a device-resident
// state; the transcript (challenge u) stays with the caller: sbn_bullet_cross for the first round's L, R, then ONE call per challenge —
// sbn_bullet_fold_cross folds with u and returns the next round's L, R (sbn_bullet_fold for the last fold).
//
// The reference folds the generators every round, G' = u_inv*G_L + u*G_R (bullet.rs:87-91): n scalar multiplications of
// 254 doublings each, a latency chain the device cannot shorten.  Here the generators are never folded.  Round j's
// generators are fixed combinations of the ORIGINAL ones, G^(j)[i] = sum_{t = i mod m} s_t * G_t (m = n / 2^j, s_t the product
// of the u / u_inv picked by t's bits — the same s the verifier builds in compute_s, bullet.rs:181-199), so
//   MSM(a_L, G^(j)_R) = MSM over the original G_t of  w_t = a_L[(t mod m) - m/2] * s_t  for (t mod m) >= m/2, else 0,
// one elementwise kernel + an MSM, and g_hat = MSM(s, G).  L, R and g_hat are the same group elements.
// Because the bases never change, both MSMs of a round run as ONE two-row shared-base commit (the Hyrax kernel path with its
// cached window table and merged duplicate generators) over the derived set G ‖ Q with h = H (derived_set, abi_msm.inc): row = [w ‖ c], blind = blind.
// Included by sbn254.hip.

static const size_t BULLET_COMB_BYTES = (size_t)3 << 30;
struct sbn_bullet {
  size_t n = 0, m = 0;          // original / current length
  const sbn_bases* ext = nullptr;   // G ‖ Q (Q = infinity when absent) with h = H; owned by the caller's G handle
  void* d_a = nullptr; void* d_b = nullptr; void* d_s = nullptr;   // a, b (m live entries, the CURRENT buffers), s (n), Montgomery Fr
  void* d_a2 = nullptr; void* d_b2 = nullptr;   // the other halves of the a / b ping-pong: the fused fold + cross round writes the folded vectors there
  void* d_dots = nullptr;       // c_L, c_R of the current round (canonical, 2 x 32 B): shipped to the host with the commit's sums
  void* d_w = nullptr;          // canonical commit input: rows [w^L ‖ c_L], [w^R ‖ c_R] of n + 1 scalars, then the two blinds
  void* slab = nullptr; size_t slab_bytes = 0;   // one pooled allocation holding d_a, d_b, d_s, d_w
  bool has_q = false, has_h = false;
  bool q_scaled = false; ScScalar qs;   // Q = q_scale * Q_base (sbn_bullet_begin_scaled): the column of Q_base carries c * q_scale; qs = q_scale in Montgomery form
};

// s_t *= (t mod m) < m/2 ? u_inv : u   (the generator fold of bullet.rs:87-91, applied to the coefficients); u, u_inv: Montgomery form, kernel arguments
__global__ void __launch_bounds__(256) k_bullet_fold_s(uint32_t* __restrict__ s, size_t n, size_t m, ScScalar su, ScScalar si) {
  const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n) return;
  const Fr f = fr_from_words(((t & (m - 1)) < (m >> 1)) ? si : su);
  fe_store_tab<FrP>(s + 8 * t, fe_mul(fe_load<FrP>(s + 8 * t), f));
}
// blockIdx.y = 0: a[i] = u * a[i] + u_inv * a[i + h];  1: b[i] = u_inv * b[i] + u * b[i + h]   (bullet.rs:94-106)
__global__ void __launch_bounds__(256) k_fold_tables(uint32_t* __restrict__ a, uint32_t* __restrict__ b, size_t h, ScScalar su, ScScalar si) {
  uint32_t* Z = blockIdx.y ? b : a;
  const Fr lo = fr_from_words(blockIdx.y ? si : su), hi = fr_from_words(blockIdx.y ? su : si);
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < h; i += (size_t)gridDim.x * blockDim.x)
    fe_store_tab<FrP>(Z + 8 * i, fe_add_lazy(fe_mul(lo, fe_load<FrP>(Z + 8 * i)), fe_mul(hi, fe_load<FrP>(Z + 8 * (i + h)))));
}
// ---- one launch for everything a round does ahead of its commit -----------------------------------------------------------------
// FOLD: first the folds with the PREVIOUS round's challenge u (bullet.rs:86-106: s_t *= u or u_inv, a' = u a_L + u_inv a_R, b' = u_inv b_L + u b_R;
// the folded vectors go to the other half of the ping-pong, every entry written by exactly one thread), then — on the folded vectors of
// length m (m = the length AFTER the fold), h = m / 2 — the cross dot products c_L = <a_L, b_R>, c_R = <a_R, b_L> (bullet.rs:72-73) and the
// two commit rows w^L, w^R (see the file header).  A thread recomputes the folded entries it needs instead of waiting for another block's
// (2 products each).  The dot products' partial sums are written through; the last of the `nbd` blocks that hold dot terms (ticket) folds
// them and writes the rows' tails (column n = Q gets c_L / c_R), the two blinds and the canonical c_L, c_R for the host — the protocol of
// sc_last_block_fold_at, with device memory as the destination (the next kernel of the stream reads it).
struct BulletPrep {
  const uint32_t* a; const uint32_t* b; uint32_t* a_nxt; uint32_t* b_nxt; uint32_t* s;
  uint32_t* wL; uint32_t* wR; uint32_t* blinds; uint32_t* dots; uint32_t* partial; uint32_t* ticket;
};
template <bool FOLD>
__global__ void __launch_bounds__(256) k_bullet_prep(BulletPrep A, size_t n, size_t m, ScScalar su, ScScalar si, int has_q /* 0: no Q term, 1: Q itself, 2: Q = qs * Q_base */, ScScalar qs, ScScalar bl, ScScalar br, uint32_t nbd) {
  const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const size_t h = m >> 1;
  Fr u = fe_zero<FrP>(), ui = u;
  if (FOLD) { u = fr_from_words(su); ui = fr_from_words(si); }
  // entry j (< m) of the vectors this round works on; before the fold they are 2 m long
  auto a_new = [&](size_t j) { return FOLD ? fe_add(fe_mul(u, fe_load<FrP>(A.a + 8 * j)), fe_mul(ui, fe_load<FrP>(A.a + 8 * (j + m)))) : fe_load<FrP>(A.a + 8 * j); };
  auto b_new = [&](size_t j) { return FOLD ? fe_add(fe_mul(ui, fe_load<FrP>(A.b + 8 * j)), fe_mul(u, fe_load<FrP>(A.b + 8 * (j + m)))) : fe_load<FrP>(A.b + 8 * j); };
  if (t < n) {
    Fr st = fe_load<FrP>(A.s + 8 * t);
    if (FOLD) { st = fe_mul(st, ((t & (2 * m - 1)) < m) ? ui : u); fe_store_tab<FrP>(A.s + 8 * t, st); }
    const size_t i = t & (m - 1);
    const bool hi = i >= h;
    const Fr w = fe_from_mont(fe_mul(a_new(hi ? i - h : i + h), st));      // canonical plain integer: the commit cuts digits from it
    const Fr z = fe_zero<FrP>();
    fe_store_packed<FrP>(A.wL + 8 * t, hi ? w : z);
    fe_store_packed<FrP>(A.wR + 8 * t, hi ? z : w);
  }
  if (blockIdx.x >= nbd) return;
  Fr cl = fe_zero<FrP>(), cr = cl;
  if (t < h) {
    const Fr aL = a_new(t), aR = a_new(t + h), bL = b_new(t), bR = b_new(t + h);
    if (FOLD) {
      fe_store_tab<FrP>(A.a_nxt + 8 * t, aL); fe_store_tab<FrP>(A.a_nxt + 8 * (t + h), aR);
      fe_store_tab<FrP>(A.b_nxt + 8 * t, bL); fe_store_tab<FrP>(A.b_nxt + 8 * (t + h), bR);
    }
    cl = fe_mul(aL, bR); cr = fe_mul(aR, bL);
  }
  sc_block_sums_store_slot(cl, cr, cr, false, A.partial, nullptr, 0u, 0u, blockIdx.x, nbd);     // write-through partial sums + the storing wave's vmcnt(0)
  __shared__ uint32_t s_last;
  __syncthreads();
  if (threadIdx.x == 0) s_last = (__hip_atomic_fetch_add(A.ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == nbd - 1) ? 1u : 0u;
  __syncthreads();
  if (!s_last) return;
  if (threadIdx.x == 0) { __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent"); asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); }
  __syncthreads();
  const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
  if (wv < 2) {
    Fr sres = fe_zero<FrP>();
    for (unsigned b = lane; b < nbd; b += 64) sres = fe_add(sres, fr_load_coherent(A.partial + 8 * ((size_t)b * 3 + wv)));
    sres = wave_sum_fr(fe_reduce(sres));
    if (lane == 0) {
      const Fr cv = fe_from_mont(sres);                                   // c_L / c_R for the caller: always the plain dot product
      Fr col = fe_zero<FrP>();
      if (has_q == 1) col = cv; else if (has_q == 2) col = fe_from_mont(fe_mul(fe_reduce(sres), fr_from_words(qs)));   // the scalar on Q_base: c * q_scale
      fe_store_packed<FrP>((wv ? A.wR : A.wL) + 8 * n, col);
      fe_store_packed<FrP>(A.dots + 8 * wv, cv);
    }
  }
  if (threadIdx.x >= 128 && threadIdx.x < 136) { const int k = threadIdx.x - 128; A.blinds[k] = bl.v[k]; A.blinds[8 + k] = br.v[k]; }
  if (threadIdx.x == 0) __hip_atomic_store(A.ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__global__ void __launch_bounds__(256) k_fr_fill_one(uint32_t* __restrict__ out, size_t n) {
  const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t < n) fe_store_packed<FrP>(out + 8 * t, fe_one<FrP>());
}

extern "C" {

void sbn_bullet_free(sbn_ctx* c, sbn_bullet* st) {
  if (!st) return;
  std::unique_lock<std::mutex> g;
  if (c) { g = std::unique_lock<std::mutex>(c->mu); hipSetDevice(c->device); hipStreamSynchronize(c->stream); }
  pool_put(c, st->slab, st->slab_bytes);
  delete st;
}
size_t sbn_bullet_len(const sbn_bullet* st) { return st ? st->m : 0; }

}  // extern "C"
static int bullet_begin_impl(sbn_ctx* c, const sbn_bases* G, const uint8_t* Q_xy, const uint8_t* q_scale, const sbn_table* a, const sbn_table* b, const uint8_t* blind,
                             uint8_t* Gamma_xy, int* Gamma_is_inf, sbn_bullet** out) {
  if (!c || !G || !a || !b || !out) return SBN_EINVAL;
  if (q_scale && (!Q_xy || !fr_canonical(q_scale))) return fail(c, SBN_EINVAL, "bullet: q_scale needs a base point and a canonical scalar");
  const size_t n = a->len;
  if (b->len != n || G->n != n) return fail(c, SBN_EINVAL, "bullet: a (%zu), b (%zu) and G (%zu) differ in length  [bullet.rs:42-43 assert_eq]", n, b->len, G->n);
  if (n == 0 || (n & (n - 1))) return fail(c, SBN_EINVAL, "bullet: n=%zu is not a power of two  [bullet.rs:44]", n);
  if (blind && !fr_canonical(blind)) return fail(c, SBN_EINVAL, "bullet: blind is not canonical");
  if (blind && !G->has_h) return fail(c, SBN_EINVAL, "bullet: blind given but the generator set has no h");
  std::lock_guard<std::mutex> g(c->mu); hipSetDevice(c->device);
  sbn_bullet* st = new sbn_bullet(); st->n = st->m = n; st->has_q = Q_xy != nullptr; st->has_h = G->has_h;
  memset(&st->qs, 0, sizeof st->qs);
  if (q_scale) { st->q_scaled = true; st->qs = scs_from(sbn_host::fr::to_dev_mont(el_from(q_scale))); }
  int rc = SBN_OK;
  auto chk = [&](hipError_t x) { if (x != hipSuccess && rc == SBN_OK) rc = fail(c, SBN_EHIP, "bullet begin: %s", hipGetErrorString(x)); };
  auto drop = [&]() { pool_put(c, st->slab, st->slab_bytes); delete st; };
  if ((rc = ensure_pin(c, 4096))) { drop(); return rc; }
  // the derived generator set for this Q: built once per (G, Q) and kept by G
  rc = derived_set(G, DERIVED_BULLET, Q_xy ? std::string((const char*)Q_xy, 64) : std::string(), [&](sbn_bases** ext) -> int {
    if ((rc = ensure(c, c->stage_pts, (n + 2) * 64))) return rc;
    uint8_t* P = (uint8_t*)c->stage_pts.p;
    chk(hipMemcpyAsync(P, G->d_pts, n * 64, hipMemcpyDeviceToDevice, c->stream));
    chk(hipMemsetAsync(P + 64 * n, 0, 64, c->stream));
    if (Q_xy) {
      memcpy(c->pin, Q_xy, 64);
      chk(hipMemcpyAsync(P + 64 * n, c->pin, 64, hipMemcpyHostToDevice, c->stream));
      LAUNCH(c, "k_points_to_mont", k_points_to_mont, 1, 256, (const uint32_t*)(P + 64 * n), (uint32_t*)(P + 64 * n), (size_t)1);
    }
    if (rc == SBN_OK) rc = bases_from_device(c, P, n + 1, G->has_h ? (const uint8_t*)G->d_pts + 64 * n : nullptr, ext);
    if (rc != SBN_OK) return rc;
    // a small lookup table (comb_kernels.cuh) for the derived set: a round's two-row commit is latency-bound, and the lookup
    // path has no sort / bucket-reduction stages to wait for.  Best effort: without the memory the bucket path serves.
    if (bases_build_comb(c, (*ext)->uniq ? (*ext)->uniq : *ext, BULLET_COMB_BYTES) != SBN_OK) (void)hipGetLastError();
    return SBN_OK;
  }, &st->ext);
  if (rc != SBN_OK) { drop(); return rc; }
  hipError_t e = pool_get(c, (5 * n + 2 * (n + 2) + 2) * 32, &st->slab, &st->slab_bytes);     // from the context's buffer cache: no hipMalloc per proof
  if (e != hipSuccess) { st->slab = nullptr; rc = fail(c, SBN_ENOMEM, "hipMalloc bullet state: %s", hipGetErrorString(e)); }
  else {
    uint8_t* p0 = (uint8_t*)st->slab; st->d_a = p0; st->d_b = p0 + 32 * n; st->d_s = p0 + 64 * n; st->d_a2 = p0 + 96 * n; st->d_b2 = p0 + 128 * n;
    st->d_w = p0 + 160 * n; st->d_dots = p0 + 160 * n + 64 * (n + 2);
  }
  if (rc == SBN_OK) {
    chk(hipMemcpyAsync(st->d_a, a->d, n * 32, hipMemcpyDeviceToDevice, c->stream));      // the reference clones them too (bullet.rs:50-52)
    chk(hipMemcpyAsync(st->d_b, b->d, n * 32, hipMemcpyDeviceToDevice, c->stream));
    LAUNCH(c, "k_fr_fill_one", k_fr_fill_one, (unsigned)((n + 255) / 256), 256, (uint32_t*)st->d_s, n);
  }
  if (rc == SBN_OK && Gamma_xy) {
    // Gamma = MSM(a, G) + <a, b> * Q + blind * H   (bullet.rs:58-60): a one-row commit of [a ‖ <a,b>] with the blind
    uint8_t ab[32];
    rc = table_dot_locked(c, (const uint32_t*)st->d_a, (const uint32_t*)st->d_b, n, ab);
    if (rc == SBN_OK) {
      uint8_t* W = (uint8_t*)st->d_w;
      LAUNCH(c, "k_scalars_from_mont", k_scalars_from_internal, (unsigned)((n + 255) / 256), 256, (const uint32_t*)st->d_a, (uint32_t*)W, n);
      uint8_t* hp = (uint8_t*)c->pin + 1024; memset(hp, 0, 64);
      if (Q_xy) {
        if (q_scale) { const sbn_host::fr::El x = sbn_host::fr::fmul(el_from(ab), el_from(q_scale)); memcpy(hp, x.v, 32); }     // <a, b> * q_scale: the scalar on Q_base
        else memcpy(hp, ab, 32);
      }
      if (blind) memcpy(hp + 32, blind, 32);
      chk(hipMemcpyAsync(W + 32 * n, hp, 64, hipMemcpyHostToDevice, c->stream));
      chk(hipStreamSynchronize(c->stream));
      uint8_t inf = 0;
      if (rc == SBN_OK) rc = commit_rows_device(c, st->ext, (const uint32_t*)W, st->has_h ? (const uint32_t*)(W + 32 * (n + 1)) : nullptr, 1, n + 1, Gamma_xy, &inf);
      if (Gamma_is_inf) *Gamma_is_inf = inf;
    }
  }
  if (rc == SBN_OK) chk(hipStreamSynchronize(c->stream));
  if (rc != SBN_OK) { drop(); return rc; }
  *out = st;
  return SBN_OK;
}
extern "C" {
int sbn_bullet_begin(sbn_ctx* c, const sbn_bases* G, const uint8_t* Q_xy, const sbn_table* a, const sbn_table* b, const uint8_t* blind,
                     uint8_t* Gamma_xy, int* Gamma_is_inf, sbn_bullet** out) {
  return bullet_begin_impl(c, G, Q_xy, nullptr, a, b, blind, Gamma_xy, Gamma_is_inf, out);
}
// Q = q_scale * Q_base.  DotProductProofLog::prove (nizk/mod.rs:478-494) draws r from the transcript and hands the bullet reduction
// Q = gens_1.scale(r).G[0] — a NEW point per proof over a FIXED base: with (Q_base, q_scale) the derived generator set G || Q_base and its
// lookup table are built once per generator set instead of once per proof; the column of Q_base carries c * q_scale.  Same L, R, Gamma.
int sbn_bullet_begin_scaled(sbn_ctx* c, const sbn_bases* G, const uint8_t* Q_base_xy, const uint8_t q_scale[32], const sbn_table* a, const sbn_table* b, const uint8_t* blind,
                            uint8_t* Gamma_xy, int* Gamma_is_inf, sbn_bullet** out) {
  if (!Q_base_xy || !q_scale) return SBN_EINVAL;
  return bullet_begin_impl(c, G, Q_base_xy, q_scale, a, b, blind, Gamma_xy, Gamma_is_inf, out);
}

}  // extern "C"
// A bullet round's hand-over (rows_to_host_launch / _collect; the first words of the mailbox's final-claims area and its flag): the two rows in st->d_w
// (n + 1 canonical scalars each, the two blinds behind them) as ONE two-row commit, the 2 x 8 words of st->d_dots behind its sums — launches only
static const uint32_t BULLET_SLOT_WORD = SC_MBOX_FINALS, BULLET_FLAG_WORD = SC_MBOX_FLAGS + SC_PACK_MAX;
static int bullet_rows_launch(sbn_ctx* c, sbn_bullet* st, uint32_t* seq) {
  const uint32_t* W = (const uint32_t*)st->d_w;
  return rows_to_host_launch(c, st->ext, W, st->has_h ? W + 16 * (st->n + 1) : nullptr, 2, st->n + 1, (const uint32_t*)st->d_dots, 16, BULLET_SLOT_WORD, BULLET_FLAG_WORD, seq);
}
// the one host wait of such a commit: the two points as canonical affine bytes, the two scalars that travelled with them
static int bullet_rows_collect(sbn_ctx* c, uint32_t seq, uint8_t P0_xy[64], int* P0_inf, uint8_t P1_xy[64], int* P1_inf, uint8_t s0[32], uint8_t s1[32]) {
  uint8_t xy[128], s[64]; int inf[2];
  const int rc = rows_to_host_collect(c, BULLET_SLOT_WORD, BULLET_FLAG_WORD, seq, 2, xy, inf, s, 64);
  if (rc) return rc;
  memcpy(P0_xy, xy, 64); memcpy(P1_xy, xy + 64, 64); memcpy(s0, s, 32); memcpy(s1, s + 32, 32);
  if (P0_inf) *P0_inf = inf[0];
  if (P1_inf) *P1_inf = inf[1];
  return SBN_OK;
}
// One round's device work and its one host wait: [FOLD: the folds with the previous challenge] + the cross dot products + the two commit
// rows in ONE launch (k_bullet_prep), the two-row commit over the original generators (bullet.rs:77-78: L = MSM(a_L, G_R) + c_L*Q + blind_L*H,
// R likewise), and the results (two XYZZ sums, c_L, c_R) through the host mailbox — no copy, no stream synchronisation.
static int bullet_round_locked(sbn_ctx* c, sbn_bullet* st, bool fold, const uint8_t* u, const uint8_t* u_inv, const uint8_t* blind_L, const uint8_t* blind_R,
                               uint8_t L_xy[64], int* L_inf, uint8_t R_xy[64], int* R_inf, uint8_t c_L[32], uint8_t c_R[32]) {
  const size_t n = st->n, m = fold ? st->m / 2 : st->m, h = m / 2;       // m: the length this round's cross terms are taken at
  int rc;
  uint8_t* WL = (uint8_t*)st->d_w; uint8_t* WR = WL + 32 * (n + 1); uint8_t* BL = WR + 32 * (n + 1);
  const uint32_t nbd = (uint32_t)std::max<size_t>(1, (h + 255) / 256);
  if ((rc = ensure(c, c->sc_partial, std::max<size_t>(4096, (size_t)nbd * 96)))) return rc;
  if ((rc = ensure(c, c->wsum, 4096))) return rc;                       // (sized ahead of the launches below, so that rows_to_host_launch never reallocates mid-round)
  if ((rc = sc_tickets(c))) return rc;
  ScScalar su, si, sl, sr; memset(&su, 0, sizeof su); memset(&si, 0, sizeof si); memset(&sl, 0, sizeof sl); memset(&sr, 0, sizeof sr);
  if (fold) { su = scs_from(sbn_host::fr::to_dev_mont(el_from(u))); si = scs_from(sbn_host::fr::to_dev_mont(el_from(u_inv))); }
  if (blind_L) memcpy(sl.v, blind_L, 32);
  if (blind_R) memcpy(sr.v, blind_R, 32);
  BulletPrep A;
  A.a = (const uint32_t*)st->d_a; A.b = (const uint32_t*)st->d_b; A.a_nxt = (uint32_t*)st->d_a2; A.b_nxt = (uint32_t*)st->d_b2; A.s = (uint32_t*)st->d_s;
  A.wL = (uint32_t*)WL; A.wR = (uint32_t*)WR; A.blinds = (uint32_t*)BL; A.dots = (uint32_t*)st->d_dots; A.partial = (uint32_t*)c->sc_partial.p;
  A.ticket = (uint32_t*)c->sc_tickets.p + 4000;                         // (slots 0 .. 47 belong to the sumcheck rounds)
  const unsigned gx = (unsigned)((n + 255) / 256);
  const int qmode = st->has_q ? (st->q_scaled ? 2 : 1) : 0;
  if (fold) LAUNCH(c, "k_bullet_prep", k_bullet_prep<true>, gx, 256, A, n, m, su, si, qmode, st->qs, sl, sr, nbd);
  else LAUNCH(c, "k_bullet_prep", k_bullet_prep<false>, gx, 256, A, n, m, su, si, qmode, st->qs, sl, sr, nbd);
  if (fold) { std::swap(st->d_a, st->d_a2); std::swap(st->d_b, st->d_b2); st->m = m; }
  uint32_t seq = 0;
  if ((rc = bullet_rows_launch(c, st, &seq))) return rc;
  return bullet_rows_collect(c, seq, L_xy, L_inf, R_xy, R_inf, c_L, c_R);
}
extern "C" {

int sbn_bullet_cross(sbn_ctx* c, sbn_bullet* st, const uint8_t* blind_L, const uint8_t* blind_R, uint8_t L_xy[64], int* L_inf,
                     uint8_t R_xy[64], int* R_inf, uint8_t c_L[32], uint8_t c_R[32]) {
  if (!c || !st || !L_xy || !R_xy || !c_L || !c_R) return SBN_EINVAL;
  if (st->m < 2) return fail(c, SBN_EINVAL, "bullet: nothing left to fold (length %zu)", st->m);
  if ((blind_L || blind_R) && !st->has_h) return fail(c, SBN_EINVAL, "bullet: blinds given but the generator set has no h");
  if ((blind_L && !fr_canonical(blind_L)) || (blind_R && !fr_canonical(blind_R))) return fail(c, SBN_EINVAL, "bullet: blind is not canonical");
  std::lock_guard<std::mutex> g(c->mu); hipSetDevice(c->device);
  return bullet_round_locked(c, st, false, nullptr, nullptr, blind_L, blind_R, L_xy, L_inf, R_xy, R_inf, c_L, c_R);
}

// fold with u (bullet.rs:86-106), then the NEXT round's cross terms (bullet.rs:72-78) — one call, one launch ahead of the commit, one host wait
int sbn_bullet_fold_cross(sbn_ctx* c, sbn_bullet* st, const uint8_t u[32], const uint8_t u_inv[32], const uint8_t* blind_L, const uint8_t* blind_R,
                          uint8_t L_xy[64], int* L_inf, uint8_t R_xy[64], int* R_inf, uint8_t c_L[32], uint8_t c_R[32]) {
  if (!c || !st || !u || !u_inv || !L_xy || !R_xy || !c_L || !c_R) return SBN_EINVAL;
  if (st->m < 4) return fail(c, SBN_EINVAL, "bullet fold_cross: length %zu leaves no cross terms after the fold (use sbn_bullet_fold for the last one)", st->m);
  if (!fr_canonical(u) || !fr_canonical(u_inv)) return fail(c, SBN_EINVAL, "bullet fold: challenge is not canonical");
  if ((blind_L || blind_R) && !st->has_h) return fail(c, SBN_EINVAL, "bullet: blinds given but the generator set has no h");
  if ((blind_L && !fr_canonical(blind_L)) || (blind_R && !fr_canonical(blind_R))) return fail(c, SBN_EINVAL, "bullet: blind is not canonical");
  std::lock_guard<std::mutex> g(c->mu); hipSetDevice(c->device);
  return bullet_round_locked(c, st, true, u, u_inv, blind_L, blind_R, L_xy, L_inf, R_xy, R_inf, c_L, c_R);
}

int sbn_bullet_fold(sbn_ctx* c, sbn_bullet* st, const uint8_t u[32], const uint8_t u_inv[32]) {
  if (!c || !st || !u || !u_inv) return SBN_EINVAL;
  if (st->m < 2) return fail(c, SBN_EINVAL, "bullet fold: nothing left to fold (length %zu)", st->m);
  if (!fr_canonical(u) || !fr_canonical(u_inv)) return fail(c, SBN_EINVAL, "bullet fold: challenge is not canonical");
  std::lock_guard<std::mutex> g(c->mu); hipSetDevice(c->device);
  const size_t n = st->n, m = st->m, h = m / 2;
  // nothing here is read back: the folded vectors are consumed by the next call on the same stream, so no host wait; the challenge and
  // its inverse travel in Montgomery form as kernel arguments (one host product each)
  const ScScalar su = scs_from(sbn_host::fr::to_dev_mont(el_from(u))), si = scs_from(sbn_host::fr::to_dev_mont(el_from(u_inv)));
  LAUNCH(c, "k_bullet_fold_s", k_bullet_fold_s, (unsigned)((n + 255) / 256), 256, (uint32_t*)st->d_s, n, m, su, si);
  unsigned gx = stream_grid(h); if (gx > 1024) gx = 1024;
  LAUNCH(c, "k_fold_tables", k_fold_tables, dim3(gx, 2), 256, (uint32_t*)st->d_a, (uint32_t*)st->d_b, h, su, si);
  LAUNCHCHK(c);
  if (c->prof) { HIPCHK(c, hipStreamSynchronize(c->stream)); prof_drain(c); }
  st->m = h;
  return SBN_OK;
}

int sbn_bullet_finish(sbn_ctx* c, sbn_bullet* st, uint8_t a_hat[32], uint8_t b_hat[32], uint8_t g_hat_xy[64], int* g_hat_is_inf) {
  if (!c || !st || !a_hat || !b_hat || !g_hat_xy) return SBN_EINVAL;
  if (st->m != 1) return fail(c, SBN_EINVAL, "bullet finish: %zu entries left, fold down to 1 first  [bullet.rs:114-116 assert_eq]", st->m);
  std::lock_guard<std::mutex> g(c->mu); hipSetDevice(c->device);
  int rc;
  if ((rc = ensure(c, c->sc_out, 4096))) return rc;
  if ((rc = ensure_pin(c, 4096))) return rc;
  LAUNCH(c, "k_fr_from_mont", k_fr_from_mont, 1, 256, (const uint32_t*)st->d_a, (uint32_t*)c->sc_out.p, (size_t)1);
  LAUNCH(c, "k_fr_from_mont", k_fr_from_mont, 1, 256, (const uint32_t*)st->d_b, (uint32_t*)c->sc_out.p + 8, (size_t)1);
  // g_hat = MSM(s, G): what the verifier computes (bullet.rs:158) and what the folds of bullet.rs:87-91 end with
  LAUNCH(c, "k_scalars_from_mont", k_scalars_from_internal, (unsigned)((st->n + 255) / 256), 256, (const uint32_t*)st->d_s, (uint32_t*)st->d_w, st->n);
  HIPCHK(c, hipMemsetAsync((uint8_t*)st->d_w + 32 * st->n, 0, 32, c->stream));      // Q's column
  LAUNCHCHK(c);
  HIPCHK(c, hipMemcpyAsync(c->pin, c->sc_out.p, 64, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  memcpy(a_hat, c->pin, 32); memcpy(b_hat, (uint8_t*)c->pin + 32, 32);
  uint8_t inf = 0;
  if ((rc = commit_rows_device(c, st->ext, (const uint32_t*)st->d_w, nullptr, 1, st->n + 1, g_hat_xy, &inf))) return rc;
  if (g_hat_is_inf) *g_hat_is_inf = inf;
  return SBN_OK;
}

}  // extern "C"
