// abi_tables.inc — C ABI: device-resident tables, sumcheck rounds, openings, derefs gather, network pieces (include/sbn254.h, B3 + 8f).
// ---- tables + sumcheck rounds ----
static inline ScScalar scs_from(const sbn_host::fr::El& e) { ScScalar s; memcpy(s.v, e.v, 32); return s; }
// the three constants of a hash layer on the host (a lone GPU lane took 11 us for them, once per call): g R, g^2 R^2 (one Montgomery product with
// the plain integer ts gives ts g^2 R), (r - tau) R — canonical, passed as kernel arguments
struct HashConsts { ScScalar gs, g2s, nts; };
static HashConsts hash_consts(const uint8_t r_hash[32], const uint8_t r_multiset[32]) {
  using namespace sbn_host::fr;
  const El g = el_from(r_hash), tau = el_from(r_multiset), zero = {{0, 0, 0, 0}};
  return {scs_from(to_dev_mont(g)), scs_from(to_dev_mont(to_dev_mont(mmul(to_m(g), g)))), scs_from(to_dev_mont(sub(zero, tau)))};
}
static int eq_evals_locked(sbn_ctx* c, const uint8_t* r, size_t ell, sbn_table** out);
extern "C" {
static unsigned stream_grid(size_t work_items) {
  size_t blocks = (work_items + 255) / 256;
  if (blocks > 2048) blocks = 2048;     // 256 CUs x 8 blocks, grid-stride beyond
  if (blocks < 1) blocks = 1;
  return (unsigned)blocks;
}
static int table_make(sbn_ctx* c, const void* src, bool src_is_host, size_t len, uint32_t flags, sbn_table** out) {
  if (len == 0 || (len & (len - 1))) return fail(c, SBN_EINVAL, "table length %zu is not a power of two", len);
  TableScope S(c); sbn_table* t; int rc;
  if ((rc = S.alloc(len, "table", &t))) return rc;
  HIPCHK(c, hipMemcpyAsync(t->d, src, len * 32, src_is_host ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice, c->stream));
  if (!(flags & SBN_SCALARS_MONT)) LAUNCH(c, "k_fr_to_mont", k_fr_to_mont, stream_grid(len), 256, (const uint32_t*)t->d, (uint32_t*)t->d, len);
  else LAUNCH(c, "k_fr_to_mont", k_fr_from_ark, stream_grid(len), 256, (const uint32_t*)t->d, (uint32_t*)t->d, len);      // ark-ff's R = 2^256 -> R = 2^261
  LAUNCHCHK(c);
  HIPCHK(c, hipStreamSynchronize(c->stream));
  *out = S.give(t);
  return S.done();
}
int sbn_table_upload(sbn_ctx* c, const uint8_t* Z, size_t len, uint32_t flags, sbn_table** out) {
  if (!c || !Z || !out) return SBN_EINVAL;
  std::lock_guard<std::mutex> g(c->mu); hipSetDevice(c->device);
  return table_make(c, Z, true, len, flags, out);
}
int sbn_table_from_dev(sbn_ctx* c, const void* Z_dev, size_t len, uint32_t flags, sbn_table** out) {
  if (!c || !Z_dev || !out) return SBN_EINVAL;
  std::lock_guard<std::mutex> g(c->mu); hipSetDevice(c->device);
  return table_make(c, Z_dev, false, len, flags, out);
}
// No stream wait: the buffers go back to the context's cache, and whatever takes them from there next is enqueued on the same
// stream, behind every kernel that may still be reading them (pool_put's overflow path ends in hipFree, which waits by itself).
void sbn_table_free(sbn_ctx* c, sbn_table* t) {
  if (!t) return;
  std::unique_lock<std::mutex> g;
  if (c) { g = std::unique_lock<std::mutex>(c->mu); hipSetDevice(c->device); }
  table_release(c, t);
}
size_t sbn_table_len(const sbn_table* t) { return t ? t->len : 0; }
int sbn_table_download(sbn_ctx* c, const sbn_table* t, uint8_t* out) {
  if (!c || !t || !out) return SBN_EINVAL;
  std::lock_guard<std::mutex> g(c->mu); hipSetDevice(c->device);
  int rc; if ((rc = ensure(c, c->stage_scal, t->len * 32))) return rc;
  LAUNCH(c, "k_fr_from_mont", k_fr_from_mont, stream_grid(t->len), 256, (const uint32_t*)t->d, (uint32_t*)c->stage_scal.p, t->len);
  LAUNCHCHK(c);
  HIPCHK(c, hipMemcpyAsync(out, c->stage_scal.p, t->len * 32, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return SBN_OK;
}
int sbn_table_read0(sbn_ctx* c, const sbn_table* t, uint8_t out[32]) {
  if (!c || !t || !out) return SBN_EINVAL;
  std::lock_guard<std::mutex> g(c->mu); hipSetDevice(c->device);
  int rc; if ((rc = ensure(c, c->sc_out, 4096))) return rc;
  LAUNCH(c, "k_fr_from_mont", k_fr_from_mont, 1, 256, (const uint32_t*)t->d, (uint32_t*)c->sc_out.p, (size_t)1);
  LAUNCHCHK(c);
  HIPCHK(c, hipMemcpyAsync(out, c->sc_out.p, 32, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return SBN_OK;
}
static int upload_r_mont(sbn_ctx* c, const uint8_t r[32]) {
  int rc; if ((rc = ensure(c, c->sc_r, 64))) return rc;
  if ((rc = ensure_pin(c, 4096))) return rc;
  if (!fr_canonical(r)) return fail(c, SBN_EINVAL, "challenge scalar is not canonical (>= r)");
  memcpy(c->pin, r, 32);
  HIPCHK(c, hipMemcpyAsync(c->sc_r.p, c->pin, 32, hipMemcpyHostToDevice, c->stream));
  LAUNCH(c, "k_fr_to_mont", k_fr_to_mont, 1, 256, (const uint32_t*)c->sc_r.p, (uint32_t*)c->sc_r.p, (size_t)1);
  return SBN_OK;
}
int sbn_bind_top_many(sbn_ctx* c, sbn_table* const* ts, size_t count, const uint8_t r[32]) {
  if (!c || !ts || !r || count == 0) return SBN_EINVAL;
  std::lock_guard<std::mutex> g(c->mu); hipSetDevice(c->device);
  for (size_t i = 0; i < count; i++) { if (!ts[i]) return SBN_EINVAL; if (ts[i]->len != ts[0]->len) return fail(c, SBN_EINVAL, "bind: tables differ in length"); }
  if (ts[0]->len < 2) return fail(c, SBN_EINVAL, "bind: table has no variable left");
  const size_t half = ts[0]->len / 2;
  unsigned gx = stream_grid(half); if (count > 1 && gx > 1024) gx = 1024;
  int rc;
  if (count <= (size_t)BIND_PACK_MAX) {
    // pointers and challenge as kernel arguments; the bound tables are read by later calls on the same stream: no host wait
    if (!fr_canonical(r)) return fail(c, SBN_EINVAL, "challenge scalar is not canonical (>= r)");
    BindPack pack; memset(&pack, 0, sizeof pack);
    for (size_t i = 0; i < count; i++) pack.t[i] = (uint32_t*)ts[i]->d;
    ScScalar rs; memcpy(rs.v, r, 32);
    LAUNCH(c, "k_bind_top", k_bind_top_packed, dim3(gx, (unsigned)count), 256, pack, half, rs);
    LAUNCHCHK(c);
    if (c->prof) { HIPCHK(c, hipStreamSynchronize(c->stream)); prof_drain(c); }
  } else {
    if ((rc = upload_r_mont(c, r))) return rc;
    if ((rc = ensure(c, c->sc_tabs, count * sizeof(void*)))) return rc;
    // pinned staging lives after the 32-byte r slot
    if ((rc = ensure_pin(c, 4096 + count * sizeof(void*)))) return rc;
    void** hp = (void**)((uint8_t*)c->pin + 64);
    for (size_t i = 0; i < count; i++) hp[i] = ts[i]->d;
    HIPCHK(c, hipMemcpyAsync(c->sc_tabs.p, hp, count * sizeof(void*), hipMemcpyHostToDevice, c->stream));
    LAUNCH(c, "k_bind_top", k_bind_top, dim3(gx, (unsigned)count), 256, (uint32_t* const*)c->sc_tabs.p, half, (const uint32_t*)c->sc_r.p);
    LAUNCHCHK(c);
    HIPCHK(c, hipStreamSynchronize(c->stream));      // the pinned staging is reused by the next call
    if (c->prof) prof_drain(c);
  }
  for (size_t i = 0; i < count; i++) ts[i]->len = half;
  return SBN_OK;
}
int sbn_bind_top(sbn_ctx* c, sbn_table* t, const uint8_t r[32]) { sbn_table* one[1] = {t}; return sbn_bind_top_many(c, one, 1, r); }

}  // extern "C" (templates need C++ linkage)
#define SC_SINGLE_LAUNCH_MAX (c->sck.single_max)    // table halves up to this many entries take the single-launch round (SBN_SC_SINGLE_MAX overrides)
// ---- the launch part of a round, shared by sbn_sc_eval_* / sbn_sc_bind_eval_* (results to the host mailbox) and the one-call provers that
// keep a round's sums on the device (abi_zk_sumcheck.inc): grids, kernel-variant thresholds, second buffers.  `res` is where the last block
// of an instance leaves its sums (ticketed fold), `seq` the sequence number written behind them.
static inline unsigned sc_eval_grid(sbn_ctx* c, size_t half, size_t count) {      // a few block rounds over the chip: see sc_fused_grid
  size_t want = (4096 + count - 1) / count, cap = (half + 255) / 256;
  if (c->sck.grid) want = c->sck.grid;
  return (unsigned)std::max<size_t>(1, std::min(std::min(want, cap), (size_t)1024));
}
static inline bool sc_fused_single(sbn_ctx* c, size_t q) { return q <= SC_SINGLE_LAUNCH_MAX / 2; }
// grid: a few block rounds over the chip (256 CUs x 4 blocks), so that each thread runs many indices and the reduction at the
// end of the kernel is amortised; never more blocks than there are groups of 256 indices
static inline unsigned sc_fused_grid(sbn_ctx* c, size_t q, size_t count, bool single) {
  // whole block rounds: count * gx just under a multiple of the resident blocks (256 CUs x waves per SIMD), so that no nearly
  // empty last round is left (4104 blocks on 1024 slots would cost a fifth round for 8 blocks)
  // Four block rounds (interleaved sweep on one box, all six streaming rounds of a 2^21 sumcheck, SBN_SC_BLOCK_ROUNDS = 1 / 2 / 3 /
  // 4 / 6: 2.60-2.63 / 2.50-2.56 / 2.46-2.53 / 2.43-2.44 / 2.56-2.63 ms)
  const size_t br = single ? 4 : c->sck.block_rounds;
  size_t want = std::max<size_t>(1, br * 256 * 2 / count), cap = (q + 255) / 256;
  if (c->sck.grid) want = c->sck.grid;
  return (unsigned)std::max<size_t>(1, std::min(std::min(want, cap), (size_t)1024));
}
// the second buffer of a table about to be bound from `len` to len / 2 entries
static int sc_second_buffer(sbn_ctx* c, sbn_table* t, size_t len) {
  if (t->cap2 >= len / 2) return SBN_OK;
  if (t->d2) { HIPCHK(c, hipStreamSynchronize(c->stream)); if (t->owned2) pool_put(c, t->d2, t->cap2 * 32); t->d2 = nullptr; t->cap2 = 0; }
  t->owned2 = true;
  size_t _gb2 = 0; hipError_t e = pool_get(c, (len / 2) * 32, &t->d2, &_gb2);
  if (e != hipSuccess) return fail(c, SBN_ENOMEM, "hipMalloc second table buffer: %s", hipGetErrorString(e));
  t->cap2 = _gb2 / 32;
  return SBN_OK;
}
static inline void sc_swap_bound(sbn_table* t, size_t len) { std::swap(t->d, t->d2); std::swap(t->cap, t->cap2); std::swap(t->owned, t->owned2); t->len = len / 2; }
// the packed (pointers as kernel arguments) eval round in one launch; c->sc_partial holds count * gx * 96 bytes, the tickets exist
template <int KIND>
static int sc_eval_launch(sbn_ctx* c, const ScArgsPack& pack, size_t count, size_t half, unsigned gx, uint32_t* res, uint32_t seq) {
  const char* nm = KIND == KIND_CUBIC ? "k_sc_eval_cubic" : KIND == KIND_R1CS ? "k_sc_eval_r1cs" : "k_sc_eval_quad";
  LAUNCH(c, nm, k_sc_eval<KIND>, dim3(gx, (unsigned)count), 256, (const ScArgs*)nullptr, pack, half, (uint32_t*)c->sc_partial.p, (uint32_t*)c->sc_tickets.p, res, seq);
  LAUNCHCHK(c);
  return SBN_OK;
}
// the packed fused bind + eval round in one launch: single (sc_fused_single) the four-lanes-per-index kernel up to q = 128 and the
// lane-per-index kernel above, else the streaming kernel (the caller has checked that its table pattern is one it is built for)
template <int KIND>
static int sc_fused_launch(sbn_ctx* c, const ScFusedPack& pack, size_t count, size_t q, unsigned gx, bool single, const ScScalar& rs, uint32_t* res, uint32_t seq) {
  const ScFusedArgs* dargs = nullptr;
  const char* nm = KIND == KIND_CUBIC ? "k_sc_bind_eval_cubic" : KIND == KIND_R1CS ? "k_sc_bind_eval_r1cs" : "k_sc_bind_eval_quad";
  const char* nms = KIND == KIND_CUBIC ? "k_sc_bind_eval_cubic_stream" : KIND == KIND_R1CS ? "k_sc_bind_eval_r1cs_stream" : "k_sc_bind_eval_quad_stream";   // profiled apart from the single-launch rounds
  if (!single)
    LAUNCH(c, nms, (k_sc_bind_eval_pf<KIND>), dim3(gx, (unsigned)count), 256, dargs, pack, q, rs, (uint32_t*)c->sc_partial.p, (uint32_t*)c->sc_tickets.p, res, seq);
  else if (q <= 128) {
    // the last rounds of a sumcheck: four lanes per index (k_sc_bind_eval_tiny), one block of up to 512 lanes per instance
    // (measured per round at 18 instances: 64 / 128 / 256 indices 10.5 / 13.8 / 21.8 us against 16 us for the lane-per-index kernel)
    const unsigned bt = (unsigned)std::max<size_t>(64, (4 * q + 63) / 64 * 64);
    LAUNCH(c, nm, (k_sc_bind_eval_tiny<KIND>), dim3(1, (unsigned)count), bt, dargs, pack, q, rs, res, seq);
  } else
    // (the 2-waves-per-SIMD build: no spills, hence no scratch segment — these launches are latency, not occupancy)
    LAUNCH(c, nm, (k_sc_bind_eval<KIND, 2>), dim3(gx, (unsigned)count), 256, dargs, pack, q, rs, (uint32_t*)c->sc_partial.p, (uint32_t*)c->sc_tickets.p, res, seq);
  LAUNCHCHK(c);
  return SBN_OK;
}
template <int KIND>
static int sc_eval_common(sbn_ctx* c, const sbn_table* const* const* cols, int ncols, size_t count, uint8_t* out) {
  // cols[j][i] = table j of instance i
  const size_t len = cols[0][0]->len;
  for (int j = 0; j < ncols; j++) for (size_t i = 0; i < count; i++) {
    if (!cols[j][i]) return SBN_EINVAL;
    if (cols[j][i]->len != len) return fail(c, SBN_EINVAL, "sumcheck eval: tables differ in length");
  }
  if (len < 2) return fail(c, SBN_EINVAL, "sumcheck eval: no variable left");
  const size_t half = len / 2;
  int rc;
  const unsigned gx = sc_eval_grid(c, half, count);
  if ((rc = ensure(c, c->sc_partial, (size_t)count * gx * 96))) return rc;
  const char* nm = KIND == KIND_CUBIC ? "k_sc_eval_cubic" : KIND == KIND_R1CS ? "k_sc_eval_r1cs" : "k_sc_eval_quad";
  uint8_t* hres;
  const bool packed = count <= (size_t)SC_PACK_MAX;         // pointers travel as kernel arguments
  // One launch whatever the size: the last block of an instance (ticket) folds the blocks' partial sums into the polled host
  // mailbox.  The partial sums are written through the caches (fr_store_coherent), so the hand-over needs no device-scope release
  // fence — the fence is what made this 3.5x slower on large tables in round 1 (it writes back the XCD's whole L2).
  // (more than SC_PACK_MAX instances: k_sc_finish folds them, and the result is copied back)
  ScArgsPack pack; memset(&pack, 0, sizeof pack);
  if (packed) { for (size_t i = 0; i < count; i++) for (int j = 0; j < ncols; j++) pack.a[i].t[j] = (const uint32_t*)cols[j][i]->d; }
  else {
    if ((rc = ensure(c, c->sc_args, count * sizeof(ScArgs)))) return rc;
    if ((rc = ensure_pin(c, 4096 + count * sizeof(ScArgs) + count * 96))) return rc;
    ScArgs* ha = (ScArgs*)((uint8_t*)c->pin + 64);
    for (size_t i = 0; i < count; i++) for (int j = 0; j < 4; j++) ha[i].t[j] = j < ncols ? (const uint32_t*)cols[j][i]->d : nullptr;
    HIPCHK(c, hipMemcpyAsync(c->sc_args.p, ha, count * sizeof(ScArgs), hipMemcpyHostToDevice, c->stream));
  }
  const ScArgs* dargs = packed ? nullptr : (const ScArgs*)c->sc_args.p;
  if (packed) {
    if ((rc = sc_tickets(c))) return rc;
    hres = (uint8_t*)c->mbox;
    const uint32_t seq = ++c->mbox_seq;
    if ((rc = sc_eval_launch<KIND>(c, pack, count, half, gx, c->mbox, seq))) return rc;
    if ((rc = sc_mbox_wait(c, count, seq))) return rc;
  } else {
    if ((rc = ensure(c, c->sc_out, std::max<size_t>(4096, count * 96)))) return rc;
    if ((rc = ensure_pin(c, 4096 + count * sizeof(ScArgs) + count * 96))) return rc;
    LAUNCH(c, nm, k_sc_eval<KIND>, dim3(gx, (unsigned)count), 256, dargs, pack, half, (uint32_t*)c->sc_partial.p, (uint32_t*)nullptr, (uint32_t*)nullptr, 0u);
    LAUNCH(c, "k_sc_finish", k_sc_finish, (unsigned)count, 64, (const uint32_t*)c->sc_partial.p, (int)gx, (uint32_t*)c->sc_out.p);
    LAUNCHCHK(c);
    hres = (uint8_t*)c->pin + 64 + count * sizeof(ScArgs);
    HIPCHK(c, hipMemcpyAsync(hres, c->sc_out.p, count * 96, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (c->prof) prof_drain(c);
  }
  if (KIND == KIND_QUAD) { for (size_t i = 0; i < count; i++) memcpy(out + 64 * i, hres + 96 * i, 64); }
  else memcpy(out, hres, count * 96);
  return SBN_OK;
}
extern "C" {
int sbn_sc_eval_cubic_batched(sbn_ctx* c, const sbn_table* const* A, const sbn_table* const* B, const sbn_table* const* Cc, size_t count, uint8_t* out) {
  if (!c || !A || !B || !Cc || !out || count == 0) return SBN_EINVAL;
  std::lock_guard<std::mutex> g(c->mu); hipSetDevice(c->device);
  const sbn_table* const* cols[3] = {A, B, Cc};
  return sc_eval_common<KIND_CUBIC>(c, cols, 3, count, out);
}
int sbn_sc_eval_cubic(sbn_ctx* c, const sbn_table* A, const sbn_table* B, const sbn_table* Cc, uint8_t out[96]) {
  if (!A || !B || !Cc) return SBN_EINVAL;
  return sbn_sc_eval_cubic_batched(c, &A, &B, &Cc, 1, out);
}
int sbn_sc_eval_r1cs(sbn_ctx* c, const sbn_table* T, const sbn_table* A, const sbn_table* B, const sbn_table* Cc, uint8_t out[96]) {
  if (!c || !T || !A || !B || !Cc || !out) return SBN_EINVAL;
  std::lock_guard<std::mutex> g(c->mu); hipSetDevice(c->device);
  const sbn_table* const* cols[4] = {&T, &A, &B, &Cc};
  return sc_eval_common<KIND_R1CS>(c, cols, 4, 1, out);
}
int sbn_sc_eval_quad(sbn_ctx* c, const sbn_table* Z, const sbn_table* ABC, uint8_t out[64]) {
  if (!c || !Z || !ABC || !out) return SBN_EINVAL;
  std::lock_guard<std::mutex> g(c->mu); hipSetDevice(c->device);
  const sbn_table* const* cols[2] = {&Z, &ABC};
  return sc_eval_common<KIND_QUAD>(c, cols, 2, 1, out);
}
}  // extern "C"
template <int KIND>
static int sc_bind_eval_common(sbn_ctx* c, sbn_table* const* const* cols, int ncols, size_t count, const uint8_t r[32], uint8_t* out) {
  const size_t len = cols[0][0]->len;
  for (int j = 0; j < ncols; j++) for (size_t i = 0; i < count; i++) {
    if (!cols[j][i]) return SBN_EINVAL;
    if (cols[j][i]->len != len) return fail(c, SBN_EINVAL, "sumcheck bind+eval: tables differ in length");
  }
  if (len < 4) return fail(c, SBN_EINVAL, "sumcheck bind+eval needs len >= 4 (use sbn_bind_top for the last round)");
  const size_t q = len / 4;
  int rc;
  if (!fr_canonical(r)) return fail(c, SBN_EINVAL, "challenge scalar is not canonical (>= r)");
  const bool packed = count <= (size_t)SC_PACK_MAX;
  const bool single = packed && sc_fused_single(c, q);
  if ((rc = ensure_pin(c, 4096 + count * sizeof(ScFusedArgs) + count * 96))) return rc;
  // the challenge in Montgomery form, once, on the host (r * 2^261 mod the group order: this library's R)
  ScScalar rs;
  rs = scs_from(sbn_host::fr::to_dev_mont(el_from(r)));
  // every distinct table gets exactly one writer; its second buffer receives the bound half.  A table that several instances
  // share (poly_C_par of prove_cubic_batched, sumcheck.rs:201-235) is bound ONCE ahead of the round and read pre-bound by all of them.
  std::vector<sbn_table*> distinct; std::vector<int> uses;
  for (size_t i = 0; i < count; i++) for (int j = 0; j < ncols; j++) {
    sbn_table* t = cols[j][i];
    auto it = std::find(distinct.begin(), distinct.end(), t);
    if (it == distinct.end()) { distinct.push_back(t); uses.push_back(1); } else uses[(size_t)(it - distinct.begin())]++;
  }
  for (sbn_table* t : distinct) if ((rc = sc_second_buffer(c, t, len))) return rc;
  std::vector<char> prebound(distinct.size(), 0);
  if (!single)
    for (size_t k = 0; k < distinct.size(); k++) if (uses[k] >= 2) {
      prebound[k] = 1;
      LAUNCH(c, "k_bind_oop", k_bind_oop, stream_grid(len / 2), 256, (const uint32_t*)distinct[k]->d, (uint32_t*)distinct[k]->d2, len / 2, rs);
    }
  ScFusedPack pack; memset(&pack, 0, sizeof pack);
  ScFusedArgs* ha = packed ? pack.a : (ScFusedArgs*)((uint8_t*)c->pin + 64);
  std::vector<char> has_writer(distinct.size(), 0);
  for (size_t i = 0; i < count; i++) for (int j = 0; j < 4; j++) {
    ha[i].src[j] = nullptr; ha[i].dst[j] = nullptr; ha[i].pre[j] = 0;
    if (j >= ncols) continue;
    sbn_table* t = cols[j][i];
    const size_t k = (size_t)(std::find(distinct.begin(), distinct.end(), t) - distinct.begin());
    if (prebound[k]) { ha[i].src[j] = (const uint32_t*)t->d2; ha[i].pre[j] = 1; continue; }
    ha[i].src[j] = (const uint32_t*)t->d;
    if (!has_writer[k]) { ha[i].dst[j] = (uint32_t*)t->d2; has_writer[k] = 1; }
  }
  const unsigned gx = sc_fused_grid(c, q, count, single);
  if ((rc = ensure(c, c->sc_partial, (size_t)count * gx * 96))) return rc;
  const char* nm = KIND == KIND_CUBIC ? "k_sc_bind_eval_cubic" : KIND == KIND_R1CS ? "k_sc_bind_eval_r1cs" : "k_sc_bind_eval_quad";
  uint8_t* hres;
  if (!packed) {
    if ((rc = ensure(c, c->sc_args, count * sizeof(ScFusedArgs)))) return rc;
    HIPCHK(c, hipMemcpyAsync(c->sc_args.p, ha, count * sizeof(ScFusedArgs), hipMemcpyHostToDevice, c->stream));
  }
  const ScFusedArgs* dargs = packed ? nullptr : (const ScFusedArgs*)c->sc_args.p;
  if (single) {
    if ((rc = sc_tickets(c))) return rc;
    hres = (uint8_t*)c->mbox;
    const uint32_t seq = ++c->mbox_seq;
    if ((rc = sc_fused_launch<KIND>(c, pack, count, q, gx, true, rs, c->mbox, seq))) return rc;
    if ((rc = sc_mbox_wait(c, count, seq))) return rc;
  } else {
    if ((rc = ensure(c, c->sc_out, std::max<size_t>(4096, count * 96)))) return rc;
    bool pf_ok = true;                          // the software-pipelined kernel is built for the usual patterns only
    for (size_t i = 0; i < count && pf_ok; i++) {
      unsigned mask = 0;
      const int order[4] = {KIND == KIND_R1CS ? 1 : 0, KIND == KIND_R1CS ? 2 : 1, KIND == KIND_R1CS ? 3 : 2, 0};
      for (int t = 0; t < ncols; t++) { const int j = order[t]; if (ha[i].pre[j]) mask |= 1u << t; else if (!ha[i].dst[j]) pf_ok = false; }
      if (!sc_pf_mask_supported(KIND, mask)) pf_ok = false;
    }
    const char* nms = KIND == KIND_CUBIC ? "k_sc_bind_eval_cubic_stream" : KIND == KIND_R1CS ? "k_sc_bind_eval_r1cs_stream" : "k_sc_bind_eval_quad_stream";   // profiled apart from the single-launch rounds
    if (pf_ok && packed) {
      // the streaming round finishes in the kernel too (ticketed fold into the host mailbox): no finishing launch, no copy, no stream wait
      if ((rc = sc_tickets(c))) return rc;
      const uint32_t seq = ++c->mbox_seq;
      if ((rc = sc_fused_launch<KIND>(c, pack, count, q, gx, false, rs, c->mbox, seq))) return rc;
      if ((rc = sc_mbox_wait(c, count, seq))) return rc;
      hres = (uint8_t*)c->mbox;
    } else {
    if (pf_ok) LAUNCH(c, nms, (k_sc_bind_eval_pf<KIND>), dim3(gx, (unsigned)count), 256, dargs, pack, q, rs, (uint32_t*)c->sc_partial.p, (uint32_t*)nullptr, (uint32_t*)nullptr, 0u);
    else LAUNCH(c, nm, (k_sc_bind_eval<KIND, 3>), dim3(gx, (unsigned)count), 256, dargs, pack, q, rs, (uint32_t*)c->sc_partial.p, (uint32_t*)nullptr, (uint32_t*)nullptr, 0u);
    LAUNCH(c, "k_sc_finish", k_sc_finish, (unsigned)count, 64, (const uint32_t*)c->sc_partial.p, (int)gx, (uint32_t*)c->sc_out.p);
    LAUNCHCHK(c);
    hres = (uint8_t*)c->pin + 64 + count * sizeof(ScFusedArgs);
    HIPCHK(c, hipMemcpyAsync(hres, c->sc_out.p, count * 96, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (c->prof) prof_drain(c);
    }
  }
  for (sbn_table* t : distinct) sc_swap_bound(t, len);
  if (KIND == KIND_QUAD) { for (size_t i = 0; i < count; i++) memcpy(out + 64 * i, hres + 96 * i, 64); }
  else memcpy(out, hres, count * 96);
  return SBN_OK;
}
extern "C" {
int sbn_sc_bind_eval_cubic_batched(sbn_ctx* c, sbn_table* const* A, sbn_table* const* B, sbn_table* const* Cc, size_t count, const uint8_t r[32], uint8_t* out) {
  if (!c || !A || !B || !Cc || !r || !out || count == 0) return SBN_EINVAL;
  std::lock_guard<std::mutex> g(c->mu); hipSetDevice(c->device);
  sbn_table* const* cols[3] = {A, B, Cc};
  return sc_bind_eval_common<KIND_CUBIC>(c, cols, 3, count, r, out);
}
int sbn_sc_bind_eval_r1cs(sbn_ctx* c, sbn_table* T, sbn_table* A, sbn_table* B, sbn_table* Cc, const uint8_t r[32], uint8_t out[96]) {
  if (!c || !T || !A || !B || !Cc || !r || !out) return SBN_EINVAL;
  std::lock_guard<std::mutex> g(c->mu); hipSetDevice(c->device);
  sbn_table* const* cols[4] = {&T, &A, &B, &Cc};
  return sc_bind_eval_common<KIND_R1CS>(c, cols, 4, 1, r, out);
}
int sbn_sc_bind_eval_quad(sbn_ctx* c, sbn_table* Z, sbn_table* ABC, const uint8_t r[32], uint8_t out[64]) {
  if (!c || !Z || !ABC || !r || !out) return SBN_EINVAL;
  std::lock_guard<std::mutex> g(c->mu); hipSetDevice(c->device);
  sbn_table* const* cols[2] = {&Z, &ABC};
  return sc_bind_eval_common<KIND_QUAD>(c, cols, 2, 1, r, out);
}
int sbn_hash_layer(sbn_ctx* c, const void* addr_dev, const sbn_table* val, const void* ts_dev, uint32_t ts_add, const uint8_t r_hash[32], const uint8_t r_multiset[32], sbn_table** out) {
  if (!c || !val || !r_hash || !r_multiset || !out) return SBN_EINVAL;
  if (!fr_canonical(r_hash) || !fr_canonical(r_multiset)) return fail(c, SBN_EINVAL, "hash layer: challenges not canonical");
  std::lock_guard<std::mutex> g(c->mu); hipSetDevice(c->device);
  const size_t n = val->len;
  const HashConsts k = hash_consts(r_hash, r_multiset);
  TableScope S(c); sbn_table* t; int rc;
  if ((rc = S.alloc(n, "hash layer", &t))) return rc;
  LAUNCH(c, "k_hash_layer", k_hash_layer, stream_grid(n), 256, (const uint32_t*)addr_dev, (const uint32_t*)val->d, (const uint32_t*)ts_dev, ts_add, k.gs, k.g2s, k.nts, n, (uint32_t*)t->d);
  LAUNCHCHK(c);                              // asynchronous: the table is consumed by later calls on the same stream
  if (c->prof) { HIPCHK(c, hipStreamSynchronize(c->stream)); prof_drain(c); }
  *out = S.give(t);
  return S.done();
}
}  // extern "C"
// (the caller holds the context's mutex and has checked the arguments)
static int hash_layer_pair_locked(sbn_ctx* c, const void* addr_dev, const sbn_table* val, const void* ts_a_dev, uint32_t ts_a_add, const void* ts_b_dev, uint32_t ts_b_add,
                                  const uint8_t r_hash[32], const uint8_t r_multiset[32], sbn_table** out_a, sbn_table** out_b) {
  const size_t n = val->len;
  const HashConsts hc = hash_consts(r_hash, r_multiset);
  TableScope S(c); sbn_table* t[2]; int rc;
  for (int k = 0; k < 2; k++) if ((rc = S.alloc(n, "hash layer", &t[k]))) return rc;
  LAUNCH(c, "k_hash_layer", k_hash_layer_pair, stream_grid(n), 256, (const uint32_t*)addr_dev, (const uint32_t*)val->d, (const uint32_t*)ts_a_dev, ts_a_add, (const uint32_t*)ts_b_dev, ts_b_add,
         hc.gs, hc.g2s, hc.nts, n, (uint32_t*)t[0]->d, (uint32_t*)t[1]->d);
  LAUNCHCHK(c);                              // asynchronous, as sbn_hash_layer
  if (c->prof) { HIPCHK(c, hipStreamSynchronize(c->stream)); prof_drain(c); }
  *out_a = t[0]; *out_b = t[1];
  S.give_all();
  return S.done();
}
// the pair and the first layer of both product circuits in one pass (k_hash_pair_prod); n = val->len is a power of two >= 2; the caller holds
// the context's mutex and has checked the arguments
static int hash_layer_pair_product_locked(sbn_ctx* c, const void* addr_dev, const sbn_table* val, const void* ts_a_dev, uint32_t ts_a_add, const void* ts_b_dev, uint32_t ts_b_add,
                                          const uint8_t r_hash[32], const uint8_t r_multiset[32], sbn_table** out_a, sbn_table** out_b, sbn_table** prod_a, sbn_table** prod_b) {
  const size_t n = val->len, half = n / 2;
  const HashConsts hc = hash_consts(r_hash, r_multiset);
  TableScope S(c); sbn_table* t[4]; int rc;                         // out_a, out_b (n entries), prod_a, prod_b (n / 2)
  for (int k = 0; k < 4; k++) if ((rc = S.alloc(k < 2 ? n : half, "hash layer", &t[k]))) return rc;
  LAUNCH(c, "k_hash_pair_prod", k_hash_pair_prod, stream_grid(half), 256, (const uint32_t*)addr_dev, (const uint32_t*)val->d, (const uint32_t*)ts_a_dev, ts_a_add, (const uint32_t*)ts_b_dev, ts_b_add,
         hc.gs, hc.g2s, hc.nts, half, (uint32_t*)t[0]->d, (uint32_t*)t[1]->d, (uint32_t*)t[2]->d, (uint32_t*)t[3]->d);
  hipError_t le = hipGetLastError();          // asynchronous, as sbn_hash_layer
  if (le == hipSuccess && c->prof) { le = hipStreamSynchronize(c->stream); prof_drain(c); }
  if (le != hipSuccess) return fail(c, SBN_EHIP, "hash layer pair + product: %s", hipGetErrorString(le));
  *out_a = t[0]; *out_b = t[1]; *prod_a = t[2]; *prod_b = t[3];
  S.give_all();
  return S.done();
}
extern "C" {
int sbn_hash_layer_pair_product(sbn_ctx* c, const void* addr_dev, const sbn_table* val, const void* ts_a_dev, uint32_t ts_a_add, const void* ts_b_dev, uint32_t ts_b_add,
                                const uint8_t r_hash[32], const uint8_t r_multiset[32], sbn_table** out_a, sbn_table** out_b, sbn_table** prod_a, sbn_table** prod_b) {
  if (!c || !val || !r_hash || !r_multiset || !out_a || !out_b || !prod_a || !prod_b) return SBN_EINVAL;
  if (!fr_canonical(r_hash) || !fr_canonical(r_multiset)) return fail(c, SBN_EINVAL, "hash layer: challenges not canonical");
  if (val->len < 2 || (val->len & (val->len - 1))) return fail(c, SBN_EINVAL, "hash layer pair + product: %zu entries (a power of two >= 2 is needed: the first product layer halves them)", val->len);
  std::lock_guard<std::mutex> g(c->mu); hipSetDevice(c->device);
  return hash_layer_pair_product_locked(c, addr_dev, val, ts_a_dev, ts_a_add, ts_b_dev, ts_b_add, r_hash, r_multiset, out_a, out_b, prod_a, prod_b);
}
int sbn_hash_layer_pair(sbn_ctx* c, const void* addr_dev, const sbn_table* val, const void* ts_a_dev, uint32_t ts_a_add, const void* ts_b_dev, uint32_t ts_b_add,
                        const uint8_t r_hash[32], const uint8_t r_multiset[32], sbn_table** out_a, sbn_table** out_b) {
  if (!c || !val || !r_hash || !r_multiset || !out_a || !out_b) return SBN_EINVAL;
  if (!fr_canonical(r_hash) || !fr_canonical(r_multiset)) return fail(c, SBN_EINVAL, "hash layer: challenges not canonical");
  std::lock_guard<std::mutex> g(c->mu); hipSetDevice(c->device);
  return hash_layer_pair_locked(c, addr_dev, val, ts_a_dev, ts_a_add, ts_b_dev, ts_b_add, r_hash, r_multiset, out_a, out_b);
}
int sbn_product_layer(sbn_ctx* c, const sbn_table* in, sbn_table** out) {
  if (!c || !in || !out) return SBN_EINVAL;
  if (in->len < 2) return fail(c, SBN_EINVAL, "product layer: nothing left to multiply");
  std::lock_guard<std::mutex> g(c->mu); hipSetDevice(c->device);
  const size_t half = in->len / 2;
  TableScope S(c); sbn_table* t; int rc;
  if ((rc = S.alloc(half, "product layer", &t))) return rc;
  LAUNCH(c, "k_product_layer", k_product_layer, stream_grid(half), 256, (const uint32_t*)in->d, half, (uint32_t*)t->d);
  LAUNCHCHK(c);                              // asynchronous, as sbn_hash_layer
  if (c->prof) { HIPCHK(c, hipStreamSynchronize(c->stream)); prof_drain(c); }
  *out = S.give(t);
  return S.done();
}
int sbn_product_circuit(sbn_ctx* c, const sbn_table* in, sbn_table** layers, size_t cap, size_t* count) {
  if (!c || !in || !layers || !count) return SBN_EINVAL;
  size_t need = 0; for (size_t l = in->len; l > 1; l >>= 1) need++;
  if (need == 0) return fail(c, SBN_EINVAL, "product circuit: nothing to multiply");
  if (cap < need) return fail(c, SBN_EINVAL, "product circuit: %zu layers do not fit the caller's array of %zu", need, cap);
  std::lock_guard<std::mutex> g(c->mu); hipSetDevice(c->device);
  const uint32_t* src = (const uint32_t*)in->d;
  for (size_t k = 0; k < need; k++) layers[k] = nullptr;                // filled at the successful end only
  TableScope S(c); sbn_table* t; int rc;
  for (size_t k = 0; k < need; k++)                                     // the tables first (so that a failed allocation leaves nothing enqueued)
    if ((rc = S.alloc(in->len >> (k + 1), "product layer", &t))) return rc;
  const std::vector<sbn_table*>& made = S.held;
  size_t k = 0, len = in->len;
  for (; k < need && len > 2048; k++, len >>= 1) {                      // large layers: one streaming launch each
    LAUNCH(c, "k_product_layer", k_product_layer, stream_grid(len / 2), 256, src, len / 2, (uint32_t*)made[k]->d);
    src = (const uint32_t*)made[k]->d;
  }
  if (k < need) {                                                       // the rest (<= 2048 entries) in one launch
    ProductTail pt; memset(&pt, 0, sizeof pt);
    for (size_t j = k; j < need; j++) pt.out[j - k] = (uint32_t*)made[j]->d;
    LAUNCH(c, "k_product_layer", k_product_tail, 1, 1024, src, len, pt);
  }
  LAUNCHCHK(c);                              // asynchronous, as sbn_product_layer
  if (c->prof) { HIPCHK(c, hipStreamSynchronize(c->stream)); prof_drain(c); }
  for (size_t j = 0; j < need; j++) layers[j] = made[j];
  S.give_all();
  *count = need;
  return S.done();
}
}  // extern "C"
// (the caller holds the context's mutex and has checked the arguments: n tables of len0 = 2^need entries, need >= 1, cap >= need)
static int product_circuit_many_locked(sbn_ctx* c, const sbn_table* const* ins, size_t n, sbn_table** layers, size_t cap, size_t len0, size_t need) {
  // the tables first (so that a failed allocation leaves nothing enqueued): layer k of circuit i is made[i * need + k] until the successful end
  // fills the caller's layers[i * cap + k]
  for (size_t i = 0; i < n; i++) for (size_t k = 0; k < need; k++) layers[i * cap + k] = nullptr;
  TableScope S(c); sbn_table* t; int rc;
  for (size_t i = 0; i < n; i++)
    for (size_t k = 0; k < need; k++) if ((rc = S.alloc(len0 >> (k + 1), "product layer", &t))) return rc;
  const std::vector<sbn_table*>& made = S.held;
  for (size_t o = 0; o < n; o += PC_MANY_MAX) {
    const size_t m = std::min<size_t>(PC_MANY_MAX, n - o);
    size_t k = 0, len = len0;
    for (; k < need && len > 2048; k++, len >>= 1) {                    // large layers: one streaming launch each, all circuits
      ProductLayerPack pk; memset(&pk, 0, sizeof pk);
      for (size_t i = 0; i < m; i++) { pk.in[i] = (const uint32_t*)(k ? made[(o + i) * need + k - 1]->d : ins[o + i]->d); pk.out[i] = (uint32_t*)made[(o + i) * need + k]->d; }
      unsigned gx = stream_grid(len / 2); gx = std::max(1u, gx / (unsigned)m);
      LAUNCH(c, "k_product_layer", k_product_layer_many, dim3(gx, (unsigned)m), 256, pk, len / 2);
    }
    if (k < need) {                                                     // the rest (<= 2048 entries): one block per circuit
      ProductTailPack pt; memset(&pt, 0, sizeof pt);
      for (size_t i = 0; i < m; i++) {
        pt.in[i] = (const uint32_t*)(k ? made[(o + i) * need + k - 1]->d : ins[o + i]->d);
        for (size_t j = k; j < need; j++) pt.out[i][j - k] = (uint32_t*)made[(o + i) * need + j]->d;
      }
      LAUNCH(c, "k_product_layer", k_product_tail_many, (unsigned)m, 1024, pt, len);
    }
  }
  hipError_t le = hipGetLastError();          // asynchronous, as sbn_product_layer
  if (le == hipSuccess && c->prof) { le = hipStreamSynchronize(c->stream); prof_drain(c); }
  if (le != hipSuccess) return fail(c, SBN_EHIP, "product circuits: %s", hipGetErrorString(le));
  for (size_t i = 0; i < n; i++) for (size_t k = 0; k < need; k++) layers[i * cap + k] = made[i * need + k];
  S.give_all();
  return S.done();
}
extern "C" {
int sbn_product_circuit_many(sbn_ctx* c, const sbn_table* const* ins, size_t n, sbn_table** layers, size_t cap, size_t* count) {
  if (!c || !ins || !layers || !count || n == 0) return SBN_EINVAL;
  for (size_t i = 0; i < n; i++) if (!ins[i]) return SBN_EINVAL;
  const size_t len0 = ins[0]->len;
  for (size_t i = 1; i < n; i++) if (ins[i]->len != len0) return fail(c, SBN_EINVAL, "product circuits: table %zu has %zu entries, table 0 has %zu", i, ins[i]->len, len0);
  size_t need = 0; for (size_t l = len0; l > 1; l >>= 1) need++;
  if (need == 0) return fail(c, SBN_EINVAL, "product circuit: nothing to multiply");
  if (cap < need) return fail(c, SBN_EINVAL, "product circuit: %zu layers do not fit the caller's rows of %zu", need, cap);
  std::lock_guard<std::mutex> g(c->mu); hipSetDevice(c->device);
  const int rc = product_circuit_many_locked(c, ins, n, layers, cap, len0, need);
  if (rc == SBN_OK) *count = need;
  return rc;
}
int sbn_table_halves(sbn_ctx* c, const sbn_table* t, sbn_table** left, sbn_table** right) {
  if (!c || !t || !left || !right) return SBN_EINVAL;
  if (t->len < 2) return fail(c, SBN_EINVAL, "halves: table has one entry");
  const size_t half = t->len / 2;
  *left = table_view(t, 0, half); *right = table_view(t, half, half);
  return SBN_OK;
}
// entries [first, first + len) of t as a view (len a power of two): the polynomials DensePolynomial::merge laid end to end (hyrax.rs:237-247)
// are slices of the merged table — Derefs' row_ops_val / col_ops_val inside `comb` (sparse_mlpoly_full.rs:286-297)
int sbn_table_slice(sbn_ctx* c, const sbn_table* t, size_t first, size_t len, sbn_table** out) {
  if (!c || !t || !out) return SBN_EINVAL;
  if (len == 0 || (len & (len - 1)) || first > t->len || len > t->len - first) return fail(c, SBN_EINVAL, "slice: [%zu, +%zu) of a table of %zu entries (a power-of-two length inside the table is needed)", first, len, t->len);
  *out = table_view(t, first, len);
  return SBN_OK;
}
static int table_dot_locked(sbn_ctx* c, const uint32_t* a, const uint32_t* b, size_t n, uint8_t out[32]) {
  int rc;
  unsigned gx = stream_grid(n); if (gx > 1024) gx = 1024;
  if ((rc = ensure(c, c->sc_partial, (size_t)gx * 96))) return rc;
  if ((rc = ensure(c, c->sc_out, 4096))) return rc;
  if ((rc = ensure_pin(c, 4096))) return rc;
  LAUNCH(c, "k_dot", k_dot, gx, 256, a, b, n, (uint32_t*)c->sc_partial.p);
  LAUNCH(c, "k_sc_finish", k_sc_finish, 1, 64, (const uint32_t*)c->sc_partial.p, (int)gx, (uint32_t*)c->sc_out.p);
  LAUNCHCHK(c);
  HIPCHK(c, hipMemcpyAsync(c->pin, c->sc_out.p, 32, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  if (c->prof) prof_drain(c);
  memcpy(out, c->pin, 32);
  return SBN_OK;
}
int sbn_table_dot(sbn_ctx* c, const sbn_table* a, const sbn_table* b, uint8_t out[32]) {
  if (!c || !a || !b || !out) return SBN_EINVAL;
  if (a->len != b->len) return fail(c, SBN_EINVAL, "dot: lengths differ (hyrax.rs:410 assert_eq)");
  std::lock_guard<std::mutex> g(c->mu); hipSetDevice(c->device);
  return table_dot_locked(c, (const uint32_t*)a->d, (const uint32_t*)b->d, a->len, out);
}
int sbn_table_evaluate(sbn_ctx* c, const sbn_table* Z, const uint8_t* r, size_t ell, uint8_t out[32]) {
  if (!c || !Z || (!r && ell) || !out || ell > 40) return SBN_EINVAL;
  if (((size_t)1 << ell) != Z->len) return fail(c, SBN_EINVAL, "evaluate: r.len() != num_vars (hyrax.rs:218 assert_eq)");
  std::lock_guard<std::mutex> g(c->mu); hipSetDevice(c->device);
  TableScope S(c); sbn_table* chi = nullptr; int rc;
  if ((rc = eq_evals_locked(c, r, ell, &chi))) return rc;
  S.keep(chi);
  if ((rc = table_dot_locked(c, (const uint32_t*)Z->d, (const uint32_t*)chi->d, Z->len, out))) return rc;
  return S.done();
}
}  // extern "C"
// (the caller holds the context's mutex and has checked the arguments)
static int table_evaluate_many_locked(sbn_ctx* c, const sbn_table* const* Z, size_t count, const uint8_t* r, size_t ell, uint8_t* out) {
  TableScope S(c); sbn_table* chi = nullptr;
  int rc = eq_evals_locked(c, r, ell, &chi);       // ONE eq table for all of them (the reference rebuilds it per call, hyrax.rs:217-222)
  if (rc) return rc;
  S.keep(chi);
  {
    const size_t n = chi->len;
    unsigned gx = stream_grid(n); if (gx > 1024) gx = 1024;
    for (size_t i0 = 0; i0 < count && rc == SBN_OK; i0 += SC_PACK_MAX) {
      const size_t m = std::min<size_t>(SC_PACK_MAX, count - i0);
      if ((rc = ensure(c, c->sc_partial, m * gx * 96))) break;
      if ((rc = ensure(c, c->sc_out, std::max<size_t>(4096, m * 96)))) break;
      if ((rc = ensure_pin(c, 4096 + m * 96))) break;
      ScArgsPack pack; memset(&pack, 0, sizeof pack);
      for (size_t i = 0; i < m; i++) pack.a[i].t[0] = (const uint32_t*)Z[i0 + i]->d;
      LAUNCH(c, "k_dot", k_dot_many, dim3(gx, (unsigned)m), 256, pack, (const uint32_t*)chi->d, n, (uint32_t*)c->sc_partial.p);
      LAUNCH(c, "k_sc_finish", k_sc_finish, (unsigned)m, 64, (const uint32_t*)c->sc_partial.p, (int)gx, (uint32_t*)c->sc_out.p);
      hipError_t e = hipGetLastError();
      if (e == hipSuccess) e = hipMemcpyAsync(c->pin, c->sc_out.p, m * 96, hipMemcpyDeviceToHost, c->stream);
      if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
      if (e != hipSuccess) { rc = fail(c, SBN_EHIP, "evaluate_many: %s", hipGetErrorString(e)); break; }
      if (c->prof) prof_drain(c);
      for (size_t i = 0; i < m; i++) memcpy(out + 32 * (i0 + i), (uint8_t*)c->pin + 96 * i, 32);
    }
  }
  return rc ? rc : S.done();
}
extern "C" {
int sbn_table_evaluate_many(sbn_ctx* c, const sbn_table* const* Z, size_t count, const uint8_t* r, size_t ell, uint8_t* out) {
  if (!c || !Z || !out || (!r && ell) || count == 0 || ell > 40) return SBN_EINVAL;
  for (size_t i = 0; i < count; i++) {
    if (!Z[i]) return SBN_EINVAL;
    if (((size_t)1 << ell) != Z[i]->len) return fail(c, SBN_EINVAL, "evaluate: r.len() != num_vars of table %zu (hyrax.rs:218 assert_eq)", i);
  }
  std::lock_guard<std::mutex> g(c->mu); hipSetDevice(c->device);
  return table_evaluate_many_locked(c, Z, count, r, ell, out);
}
int sbn_table_bound(sbn_ctx* c, const sbn_table* Z, const sbn_table* Lv, sbn_table** out) {
  if (!c || !Z || !Lv || !out) return SBN_EINVAL;
  const size_t L_size = Lv->len;
  if (L_size == 0 || Z->len % L_size) return fail(c, SBN_EINVAL, "bound: table length is not a multiple of L.len()");
  const size_t R_size = Z->len / L_size;
  std::lock_guard<std::mutex> g(c->mu); hipSetDevice(c->device);
  // row slices so that ~2048 blocks are in flight
  const size_t col_tiles = (R_size + 63) / 64;
  size_t nslices = (2048 + col_tiles - 1) / col_tiles; if (nslices > L_size) nslices = L_size; if (nslices < 1) nslices = 1;
  const size_t rows_per_slice = (L_size + nslices - 1) / nslices; nslices = (L_size + rows_per_slice - 1) / rows_per_slice;
  if (col_tiles > 0x7fffffff || nslices > 65535) return fail(c, SBN_EINVAL, "bound: grid too large");
  int rc;
  if ((rc = ensure(c, c->sc_partial, nslices * R_size * 32))) return rc;
  TableScope S(c); sbn_table* t;
  if ((rc = S.alloc(R_size, "bound table", &t))) return rc;
  LAUNCH(c, "k_bound_partial", k_bound_partial, dim3((unsigned)col_tiles, (unsigned)nslices), 256, (const uint32_t*)Z->d, (const uint32_t*)Lv->d, L_size, R_size, rows_per_slice, (uint32_t*)c->sc_partial.p);
  LAUNCH(c, "k_bound_fold", k_bound_fold, (unsigned)((R_size + 255) / 256), 256, (const uint32_t*)c->sc_partial.p, nslices, R_size, (uint32_t*)t->d);
  LAUNCHCHK(c);
  HIPCHK(c, hipStreamSynchronize(c->stream));
  if (c->prof) prof_drain(c);
  *out = S.give(t);
  return S.done();
}
}  // extern "C"
// rshift < 0: the whole polynomial (padded to a power of two); else the rows row0, row0 + rstep, ... (nrows of them) of its L x 2^rshift view
// (the caller holds the context's mutex and has checked the pointers)
static int gather_merge_locked(sbn_ctx* c, const sbn_table* const* mem, const void* const* addr_dev, size_t count, size_t n, int rshift, size_t row0, size_t rstep, size_t nrows, sbn_table** out) {
  size_t padded = 1; while (padded < count * n) padded <<= 1;              // Z.resize(len.next_power_of_two()) (hyrax.rs:245)
  size_t out_len = padded;
  if (rshift >= 0) {
    const size_t R = (size_t)1 << rshift;
    if (R > padded || rstep == 0 || nrows == 0 || (row0 + (nrows - 1) * rstep) >= padded / R) return fail(c, SBN_EINVAL, "gather rows: rows %zu + k * %zu (k < %zu) are not all inside the %zu x %zu matrix", row0, rstep, nrows, padded / R, R);
    out_len = nrows * R;
  }
  int rc;
  if ((rc = ensure(c, c->sc_args, count * sizeof(GatherArgs) + 64))) return rc;
  if ((rc = ensure_pin(c, 4096 + count * sizeof(GatherArgs)))) return rc;
  GatherArgs* ha = (GatherArgs*)((uint8_t*)c->pin + 64);
  for (size_t k = 0; k < count; k++) { ha[k].mem = (const uint32_t*)mem[k]->d; ha[k].addr = (const uint32_t*)addr_dev[k]; ha[k].mem_len = mem[k]->len; }
  uint8_t* d_args = (uint8_t*)c->sc_args.p; uint32_t* d_oob = (uint32_t*)(d_args + count * sizeof(GatherArgs));
  HIPCHK(c, hipMemcpyAsync(d_args, ha, count * sizeof(GatherArgs), hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemsetAsync(d_oob, 0, 4, c->stream));
  TableScope S(c); sbn_table* t;
  if ((rc = S.alloc(out_len, "gather table", &t))) return rc;
  LAUNCH(c, "k_gather_merge", k_gather_merge, stream_grid(out_len), 256, (const GatherArgs*)d_args, count, n, out_len, (uint32_t*)t->d, d_oob, rshift, row0, rstep);
  LAUNCHCHK(c);
  uint32_t oob = 0;
  HIPCHK(c, hipMemcpyAsync(c->pin, d_oob, 4, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  if (c->prof) prof_drain(c);
  memcpy(&oob, c->pin, 4);
  if (oob) return fail(c, SBN_EINVAL, "gather: %u addresses are outside their memory table (sparse_mlpoly_full.rs:228 assert)", oob);
  *out = S.give(t);
  return S.done();
}
static int gather_merge_impl(sbn_ctx* c, const sbn_table* const* mem, const void* const* addr_dev, size_t count, size_t n, int rshift, size_t row0, size_t rstep, size_t nrows, sbn_table** out) {
  if (!c || !mem || !addr_dev || !out || count == 0 || n == 0) return SBN_EINVAL;
  for (size_t k = 0; k < count; k++) if (!mem[k] || !addr_dev[k]) return SBN_EINVAL;
  std::lock_guard<std::mutex> g(c->mu); hipSetDevice(c->device);
  return gather_merge_locked(c, mem, addr_dev, count, n, rshift, row0, rstep, nrows, out);
}
extern "C" {
int sbn_gather_merge(sbn_ctx* c, const sbn_table* const* mem, const void* const* addr_dev, size_t count, size_t n, sbn_table** out) {
  return gather_merge_impl(c, mem, addr_dev, count, n, -1, 0, 1, 0, out);
}
int sbn_gather_merge_rows(sbn_ctx* c, const sbn_table* const* mem, const void* const* addr_dev, size_t count, size_t n, size_t R, size_t row0, size_t rstep, size_t nrows, sbn_table** out) {
  if (R == 0 || (R & (R - 1))) return c ? fail(c, SBN_EINVAL, "gather rows: R = %zu is not a power of two (hyrax.rs:371-373 gives powers of two)", R) : SBN_EINVAL;
  int rshift = 0; while (((size_t)1 << rshift) < R) rshift++;
  return gather_merge_impl(c, mem, addr_dev, count, n, rshift, row0, rstep, nrows, out);
}
int sbn_commit_table(sbn_ctx* c, const sbn_bases* b, const sbn_table* t, const uint8_t* blinds, size_t L, size_t R, uint8_t* out_xy, uint8_t* out_inf) {
  if (!c || !b || !t || (!out_xy && L)) return SBN_EINVAL;
  if (L * R != t->len) return fail(c, SBN_EINVAL, "commit_table: L*R (%zu) != table length (%zu)  [hyrax.rs:257 assert_eq]", L * R, t->len);
  void* dB = nullptr; int rc;
  if (blinds) {
    if ((rc = sbn_dev_alloc(c, L * 32, &dB))) return rc;
    if ((rc = sbn_dev_upload(c, dB, blinds, L * 32))) { sbn_dev_free(c, dB); return rc; }
    // blinds arrive canonical while the table is Montgomery: bring the blinds to Montgomery form so one flag covers both
    std::lock_guard<std::mutex> g(c->mu); hipSetDevice(c->device);
    LAUNCH(c, "k_fr_to_mont", k_fr_to_mont, stream_grid(L), 256, (const uint32_t*)dB, (uint32_t*)dB, L);
  }
  rc = commit_rows_dev_impl(c, b, t->d, dB, L, R, SBN_SCALARS_INTERNAL, out_xy, out_inf);
  if (dB) sbn_dev_free(c, dB);
  return rc;
}
}  // extern "C"
// EqPolynomial::evals (hyrax.rs:355-369); the caller holds the context's mutex
static int eq_evals_locked(sbn_ctx* c, const uint8_t* r, size_t ell, sbn_table** out) {
  for (size_t j = 0; j < ell; j++) if (!fr_canonical(r + 32 * j)) return fail(c, SBN_EINVAL, "eq_evals: r[%zu] is not canonical", j);
  const size_t N = (size_t)1 << ell;
  int rc;
  if ((rc = ensure(c, c->stage_scal, std::max<size_t>(N * 32, 64)))) return rc;     // ping-pong partner
  TableScope S(c); sbn_table* t;
  if ((rc = S.alloc(N, "eq table", &t))) return rc;
  // No staging copy, no conversion launch and no host wait: the point travels as kernel arguments in Montgomery form (one host product
  // per coordinate), the table is consumed in stream order.  Levels: the first m <= 12 in one launch (direct product per entry), then
  // two levels per pass.
  std::vector<ScScalar> rm(ell);
  for (size_t j = 0; j < ell; j++) rm[j] = scs_from(sbn_host::fr::to_dev_mont(el_from(r + 32 * j)));
  const size_t m = std::min<size_t>(ell, EQ_DIRECT_MAX);
  EqPoint pt; memset(&pt, 0, sizeof pt);
  for (size_t j = 0; j < m; j++) memcpy(pt.v[j], rm[j].v, 32);
  size_t passes = 0; for (size_t j = m; j < ell; ) { j += (ell - j >= 2) ? 2 : 1; passes++; }
  // ping-pong so that the last pass lands in t->d
  uint32_t* bufA = (uint32_t*)t->d; uint32_t* bufB = (uint32_t*)c->stage_scal.p;
  uint32_t* cur = (passes % 2 == 0) ? bufA : bufB;
  LAUNCH(c, "k_eq_level", k_eq_direct, (unsigned)((((size_t)1 << m) + 255) / 256), 256, pt, (int)m, cur);
  size_t size = (size_t)1 << m;
  for (size_t j = m; j < ell; ) {
    uint32_t* nxt = (cur == bufA) ? bufB : bufA;
    if (ell - j >= 2) { LAUNCH(c, "k_eq_level", k_eq_level2, stream_grid(size), 256, (const uint32_t*)cur, nxt, size, rm[j], rm[j + 1]); size *= 4; j += 2; }
    else { LAUNCH(c, "k_eq_level", k_eq_level, stream_grid(size), 256, (const uint32_t*)cur, nxt, size, rm[j]); size *= 2; j += 1; }
    cur = nxt;
  }
  LAUNCHCHK(c);
  if (c->prof) { HIPCHK(c, hipStreamSynchronize(c->stream)); prof_drain(c); }
  *out = S.give(t);
  return S.done();
}
extern "C" {
int sbn_eq_evals(sbn_ctx* c, const uint8_t* r, size_t ell, sbn_table** out) {
  if (!c || (!r && ell) || !out || ell > 40) return SBN_EINVAL;
  std::lock_guard<std::mutex> g(c->mu); hipSetDevice(c->device);
  return eq_evals_locked(c, r, ell, out);
}

}  // extern "C"
