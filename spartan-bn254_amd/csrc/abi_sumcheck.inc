// abi_sumcheck.inc — C ABI: SumcheckInstanceProof::prove_cubic_batched (sumcheck.rs:165-330) as a device-resident state.
//
// The reference's loop per round: per-instance sums -> coeffs combination (:269-271) -> UniPoly -> transcript -> r_j -> bind every
// table (:289-299).  The transcript only ever sees the combination, so the state returns exactly that: three scalars per round.
// The caller's tables are never written: from the first bind on the state works on its own buffers (one slab, two buffers per
// table of half and a quarter of the length, alternating).  Three modes, chosen when the sumcheck begins:
//   COMB    (tables of >= 2^16 entries = SC_COMB_MIN_LEN, >= 2 "par" instances, no zero coefficient): the "par" group runs on the combined kernels
//           (sumcheck_comb_kernels.cuh: c_i folded into A_i at the first bind, products summed before ONE reduction, C factored out)
//           while a round has >= 2^14 index pairs (SC_COMB_MIN_Q), the "seq" instances on the per-instance kernels; smaller rounds: everything on the
//           per-instance single-launch kernels (A' is already scaled: the host only adds the "par" triples);
//   SCALED  (smaller tables): the "par" A tables are copied scaled when the sumcheck begins (one launch), then the per-instance kernels;
//   PLAIN   (a zero coefficient among the "par" instances): nothing is scaled, the host combines with coeffs.
// In every mode the "seq" instances' triples are weighted on the host (18 products per round at most).
// Final claims (:302-318): A_i[0] = A'_i[0] / c_i — one host inversion per sumcheck (batched), the same field elements bit for bit.
// sbn_sumcheck_prove (end of this file) queues all rounds of such a state at once, with the transcript step on the device between them.

struct sbn_sumcheck {
  size_t n_par = 0, n_seq = 0, ntab = 0;
  size_t len = 0, len0 = 0;                 // current / initial table length
  int binds = 0;                            // rounds bound so far
  int mode = 0;                             // 0 PLAIN, 1 SCALED, 2 COMB
  bool scaled = false;                      // the "par" A tables currently hold c_i * A_i
  std::vector<const uint32_t*> cur;         // current tables, in the order of `finals`: A_par.., B_par.., C_par, A_seq.., B_seq.., C_seq..
  void* slab = nullptr; size_t slab_bytes = 0;
  std::vector<uint32_t*> buf[2];            // per table: buffer of len0 / 2 and of len0 / 4 entries
  std::vector<uint32_t*> scaled_copy;       // SCALED mode: full-length c_i * A_i (inside the slab)
  std::vector<sbn_host::fr::El> co, co_m;   // coeffs canonical / host-Montgomery (all instances)
  std::vector<sbn_host::fr::El> co_inv_m;   // 1 / c_i of the "par" instances, host-Montgomery (modes that scale A; computed while round 0 runs)
  ScCombGroup* d_groups = nullptr;          // device: the groups of the round-0 sums and of every combined round, written once when the sumcheck begins
  size_t eval_groups = 0;                   // groups [0, eval_groups): round-0 sums
  std::vector<size_t> grp_off, grp_cnt;     // combined round j (= binds so far): groups [grp_off[j], + grp_cnt[j])
  sbn_table* owned_c = nullptr;             // sbn_sumcheck_begin_eq: the eq table built for this sumcheck (poly_C_par), released with the state
  uint8_t evals0[96] = {0};                 // round 0's combined sums as sbn_sumcheck_begin returned them (sbn_sumcheck_prove starts from them)
  std::vector<uint8_t> finals_host;         // the final claims as the last round delivered them (canonical, before the division by c_i)
  uint32_t* d_finals = nullptr;             // ntab x 32 B: where the LAST bind puts every table's single entry (sbn_sumcheck_finish reads it in one go)
};
static const size_t SC_COMB_MIN_LEN = (size_t)1 << 16;      // COMB mode from this table length on
// partial sums: [0, 24 x 1024) triples for the per-instance kernels (slot * gridDim.x + block), then 24 x 2048 for the combined kernels
static const size_t SC_PARTIAL_BYTES = (size_t)SC_PACK_MAX * 1024 * 96 * 3;
static const size_t SC_COMB_MIN_Q = (size_t)1 << 14;        // (ScKnobs::comb_min_q's default) ... and its kernels while a round has this many index pairs (tools/sc_minq_sweep.sh:
                                                            // 2^13: 3.81-3.83 ms per 18 x 2^21 sumcheck, 48.0-48.7 ms per prove; 2^14: 3.75 / 47.6-47.7)
// blocks per group / per instance the partial-sum area holds: 24 x 1024 triples for the per-instance kernels, 24 x 2048 behind them for the
// combined kernels (sc_block_sums_store_at writes partial[(slot * nblk + bidx) * 3]); every grid below is clamped to these, whatever the overrides say
static const size_t SC_PART_INST_BLOCKS = 1024, SC_PART_COMB_BLOCKS = 2048;
static_assert(SC_PARTIAL_BYTES == (size_t)SC_PACK_MAX * (SC_PART_INST_BLOCKS + SC_PART_COMB_BLOCKS) * 96, "partial-sum area and the grid clamps disagree");
#define sc_comb_min_q() (c->sck.comb_min_q)
// returns the slab to the context's cache unless released (every error exit of sbn_sumcheck_begin after pool_get)
struct ScSlabGuard { sbn_ctx* c; sbn_sumcheck* st; bool armed = true; ~ScSlabGuard() { if (armed && st->slab) { pool_put(c, st->slab, st->slab_bytes); st->slab = nullptr; } } };
// a round that fails after its first launch leaves tables half bound: the state is marked dead (len = 0) so that later calls return SBN_EINVAL
struct ScRoundGuard { sbn_sumcheck* st; bool ok = false; ~ScRoundGuard() { if (!ok) st->len = 0; } };

template <int N> struct ScScalePack { const uint32_t* src[N]; uint32_t* dst[N]; ScScalar s[N]; };
// dst[x] = s * src[x] for up to SC_PACK_MAX tables (blockIdx.y = table; s in the tables' Montgomery form)
__global__ void __launch_bounds__(256) k_sc_scale(ScScalePack<SC_PACK_MAX> pack, size_t n) {
  const uint32_t* src = nullptr; uint32_t* dst = nullptr; ScScalar ss;
#pragma unroll
  for (int i = 0; i < SC_PACK_MAX; i++) if (i == (int)blockIdx.y) { src = pack.src[i]; dst = pack.dst[i]; ss = pack.s[i]; }
  const Fr s = fr_from_words(ss);
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x)
    fe_gstore_packed<FrP>(dst + 8 * i, fe_mulu(s, fe_gload<FrP>(src + 8 * i)));              // [0, 1.02 r): a table value
}
// The first bind of COMB mode scales A: A'_i = (c_i (1 - r)) z0 + (c_i r) z2.  The groups of that launch are written when the sumcheck begins
// with u = c_i; once the first challenge is known this kernel (one block per group, one lane per instance) replaces u, v by c_i (1 - r), c_i r
// in place — canonical Montgomery words, the same field elements the host used to compute and copy up (a 1.5 KB copy per sumcheck, 13 us of
// blit kernel in the prove's trace).
template <class RS>
__global__ void __launch_bounds__(64) k_sc_first_uv(ScCombGroup* __restrict__ groups, RS rmont) {
  ScCombGroup* g = groups + blockIdx.x;
  const uint32_t k = threadIdx.x;
  if (k >= g->n) return;
  const Fr r = fr_from_words(rmont), ci = fe_unpack<FrP>(g->u[k]);
  const Fr cr = fe_mul(ci, r);
  fe_store<FrP>(g->v[k], cr);                                       // canonical
  fe_store<FrP>(g->u[k], fe_sub(ci, cr));
}
// out-of-place bind of up to 64 tables (the last round of a sumcheck whose tables are still the caller's)
struct BindOopPack { const uint32_t* src[BIND_PACK_MAX]; uint32_t* dst[BIND_PACK_MAX]; };
__global__ void __launch_bounds__(256) k_bind_oop_many(BindOopPack pack, size_t half, ScScalar rmont) {
  const uint32_t* Z = nullptr; uint32_t* D = nullptr;
#pragma unroll
  for (int i = 0; i < BIND_PACK_MAX; i++) if (i == (int)blockIdx.y) { Z = pack.src[i]; D = pack.dst[i]; }
  const Fr r = fr_from_words(rmont);
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < half; i += (size_t)gridDim.x * blockDim.x)
    fe_gstore_packed<FrP>(D + 8 * i, sc_bind1(fe_gload<FrP>(Z + 8 * i), fe_gload<FrP>(Z + 8 * (i + half)), r));
}
// The LAST bind of a sumcheck (two entries per table left) and the final claims in one launch: fin[t] = Z_t[0] + r (Z_t[1] - Z_t[0]) stays on the
// device (table format) and goes to the host mailbox as a canonical integer, flag behind them (sc_flag_store's protocol) — the separate
// k_sc_finals launch and its wait (one host round trip per sumcheck, 43 per prove) disappear.  One block, one lane per table (<= 80).
constexpr int SC_FINAL_MAX = 80;
static_assert(SC_FINAL_MAX >= 3 * SC_PACK_MAX + 1, "one lane per table of the largest sumcheck");
struct ScFinalPack { const uint32_t* src[SC_FINAL_MAX]; };
template <class RS>
__global__ void __launch_bounds__(128) k_sc_bind_finals(ScFinalPack pk, uint32_t count, RS rmont, uint32_t* __restrict__ fin, uint32_t* __restrict__ host_out, uint32_t* __restrict__ flag, uint32_t seq) {
  const uint32_t t = threadIdx.x;
  const uint32_t* z = nullptr;
#pragma unroll
  for (int i = 0; i < SC_FINAL_MAX; i++) if (i == (int)t) z = pk.src[i];
  if (t < count) {
    const Fr v = sc_bind1(fe_load<FrP>(z), fe_load<FrP>(z + 8), fr_from_words(rmont));
    fe_store_packed<FrP>(fin + 8 * t, v);
    fe_store_packed<FrP>(host_out + 8 * t, fe_from_mont(v));
  }
  sc_drain_stores();
  __syncthreads();
  if (t == 0) sc_flag_store(flag, seq);
}
// the same for entry 0 of up to 64 separate tables (sbn_table_read0_many: e.g. the 18 products of the memory-checking circuits)
struct ScRead0Pack { const uint32_t* p[64]; };
__global__ void __launch_bounds__(128) k_sc_finals_gather(ScRead0Pack pk, uint32_t count, uint32_t* __restrict__ host_out, uint32_t* __restrict__ flag, uint32_t seq) {
  const uint32_t t = threadIdx.x;
  if (t < count) fe_store_packed<FrP>(host_out + 8 * t, fe_from_mont(fe_load<FrP>(pk.p[t])));
  sc_drain_stores();
  __syncthreads();
  if (t == 0) sc_flag_store(flag, seq);
}

// ---- the per-instance fused round on raw pointers (what sc_bind_eval_common does for table handles) -----------------------------
// inst[i]: src / dst / pre of A, B, C (dst null: another instance writes that table).  Slots 0 .. count-1 of the mailbox.
// RS: the challenge as a kernel argument (ScScalar) or in device memory (ScScalarDev); mbox: where the sums and their flags go (the host mailbox, or its
// device twin when a transcript step kernel reads them: sbn_sumcheck_prove)
template <class RS>
static int sc_launch_inst_fused(sbn_ctx* c, ScFusedPack& pack, size_t count, size_t q, const RS& rs, uint32_t* mbox, uint32_t seq) {
  int rc;
  const bool single = q <= SC_SINGLE_LAUNCH_MAX / 2;
  unsigned gx;
  {
    const size_t br = 4;
    size_t want = std::max<size_t>(1, br * 256 * 2 / count), cap = (q + 255) / 256;
    gx = (unsigned)std::max<size_t>(1, std::min(std::min(want, cap), SC_PART_INST_BLOCKS));
  }
  if ((rc = ensure(c, c->sc_partial, SC_PARTIAL_BYTES))) return rc;
  const ScFusedArgs* dargs = nullptr;
  if (single) {
    if (q <= 128) {
      const unsigned bt = (unsigned)std::max<size_t>(64, (4 * q + 63) / 64 * 64);
      LAUNCH(c, "k_sc_bind_eval_cubic", (k_sc_bind_eval_tiny<KIND_CUBIC, RS>), dim3(1, (unsigned)count), bt, dargs, pack, q, rs, mbox, seq);
    } else
      LAUNCH(c, "k_sc_bind_eval_cubic", (k_sc_bind_eval<KIND_CUBIC, 2, RS>), dim3(gx, (unsigned)count), 256, dargs, pack, q, rs, (uint32_t*)c->sc_partial.p, (uint32_t*)c->sc_tickets.p, mbox, seq);
  } else {
    // streaming: every table needs its writer in the launch or must arrive bound (the caller pre-binds shared tables)
    bool pf_ok = true;
    for (size_t i = 0; i < count && pf_ok; i++) {
      unsigned mask = 0;
      for (int t = 0; t < 3; t++) { if (pack.a[i].pre[t]) mask |= 1u << t; else if (!pack.a[i].dst[t]) pf_ok = false; }
      if (!sc_pf_mask_supported(KIND_CUBIC, mask)) pf_ok = false;
    }
    if (pf_ok) LAUNCH(c, "k_sc_bind_eval_cubic_stream", (k_sc_bind_eval_pf<KIND_CUBIC, RS>), dim3(gx, (unsigned)count), 256, dargs, pack, q, rs, (uint32_t*)c->sc_partial.p, (uint32_t*)c->sc_tickets.p, mbox, seq);
    else LAUNCH(c, "k_sc_bind_eval_cubic", (k_sc_bind_eval<KIND_CUBIC, 2, RS>), dim3(gx, (unsigned)count), 256, dargs, pack, q, rs, (uint32_t*)c->sc_partial.p, (uint32_t*)c->sc_tickets.p, mbox, seq);
  }
  LAUNCHCHK(c);
  return SBN_OK;
}
// mbox: where the sums and their flags go (null: the host mailbox; sbn_product_proof_prove passes the mailbox's device twin)
static int sc_launch_inst_eval(sbn_ctx* c, ScArgsPack& pack, size_t count, size_t half, uint32_t seq, uint32_t* mbox = nullptr) {
  int rc;
  size_t want = (c->sck.eval_blocks + count - 1) / count, cap = (half + 255) / 256;
  const unsigned gx = (unsigned)std::max<size_t>(1, std::min(std::min(want, cap), SC_PART_INST_BLOCKS));
  if ((rc = ensure(c, c->sc_partial, SC_PARTIAL_BYTES))) return rc;
  LAUNCH(c, "k_sc_eval_cubic", k_sc_eval<KIND_CUBIC>, dim3(gx, (unsigned)count), 256, (const ScArgs*)nullptr, pack, half, (uint32_t*)c->sc_partial.p, (uint32_t*)c->sc_tickets.p, mbox ? mbox : c->mbox, seq);
  LAUNCHCHK(c);
  return SBN_OK;
}

// how many groups the "par" instances are dealt into for a launch over idx_count indices: enough to fill the chip (one index per
// thread, 2 waves per SIMD = 131072 lanes), never more than the instances or the free mailbox slots, never more than 16 instances each
static size_t sc_comb_group_count(const sbn_ctx* c, const sbn_sumcheck* st, size_t idx_count, size_t max_groups, size_t* per_out) {
  const size_t lanes = c->sck.comb_lanes;   // (default 262144: two groups' worth of resident lanes: tools/sc_groups_sweep.sh, 131072 / 262144 / 524288 / 1048576 -> 1.365 / 1.281 / 1.338 / 1.420 ms over the later streaming rounds)
  size_t G = std::max<size_t>(1, (lanes + idx_count - 1) / idx_count);
  G = std::min(std::min(G, st->n_par), max_groups);
  G = std::max(G, (st->n_par + SC_COMB_MAX - 1) / SC_COMB_MAX);
  const size_t per = (st->n_par + G - 1) / G;
  if (per_out) *per_out = per;
  return (st->n_par + per - 1) / per;
}
// c_unbound != nullptr (bind rounds): the round binds the shared C itself — every group reads the unbound table, group 0 also writes the bound one (cptr)
static void sc_comb_groups_fill(const sbn_sumcheck* st, ScCombGroup* hg, size_t G, size_t per, const uint32_t* const* src, uint32_t* const* dst, const uint32_t* cptr,
                                bool scale, const sbn_host::fr::El* u, const sbn_host::fr::El* v, const uint32_t* c_unbound = nullptr) {
  memset(hg, 0, G * sizeof(ScCombGroup));
  for (size_t g = 0; g < G; g++) {
    const size_t i0 = g * per, i1 = std::min(st->n_par, i0 + per);
    hg[g].n = (uint32_t)(i1 - i0); hg[g].scale = scale ? 1u : 0u; hg[g].c = cptr;
    if (c_unbound) { hg[g].c_src = c_unbound; hg[g].c_dst = g == 0 ? const_cast<uint32_t*>(cptr) : nullptr; }
    for (size_t i = i0; i < i1; i++) {
      const size_t k = i - i0;
      hg[g].a_src[k] = src[i]; hg[g].b_src[k] = src[st->n_par + i];
      if (dst) { hg[g].a_dst[k] = dst[i]; hg[g].b_dst[k] = dst[st->n_par + i]; }
      if (scale) { memcpy(hg[g].u[k], u[i].v, 32); if (v) memcpy(hg[g].v[k], v[i].v, 32); }
    }
  }
}

// mailbox slots [0, n_inst) hold per-instance triples (instances listed in inst_ids), slots [n_inst, n_inst + n_comb) combined "par" sums
static void sc_combine_host(const sbn_sumcheck* st, const uint8_t* mbox, const std::vector<size_t>& inst_ids, size_t n_comb, uint8_t out[96]) {
  using namespace sbn_host::fr;
  El acc[3] = {{{0, 0, 0, 0}}, {{0, 0, 0, 0}}, {{0, 0, 0, 0}}};
  for (size_t s = 0; s < inst_ids.size(); s++) {
    const size_t i = inst_ids[s];
    const bool weighted = !(i < st->n_par && st->scaled);          // a scaled "par" instance's sums already carry c_i
    for (int t = 0; t < 3; t++) {
      El x = el_from(mbox + 96 * s + 32 * t);
      if (weighted) x = mmul(st->co_m[i], x);
      acc[t] = add(acc[t], x);
    }
  }
  for (size_t g = 0; g < n_comb; g++)
    for (int t = 0; t < 3; t++) acc[t] = add(acc[t], el_from(mbox + 96 * (inst_ids.size() + g) + 32 * t));
  for (int t = 0; t < 3; t++) memcpy(out + 32 * t, acc[t].v, 32);
}

extern "C" {

void sbn_sumcheck_free(sbn_ctx* c, sbn_sumcheck* st) {
  if (!st) return;
  std::unique_lock<std::mutex> g;
  if (c) { g = std::unique_lock<std::mutex>(c->mu); hipSetDevice(c->device); }
  if (st->slab) pool_put(c, st->slab, st->slab_bytes);                 // recycled in stream order (see sbn_table_free)
  table_release(c, st->owned_c);
  delete st;
}
size_t sbn_sumcheck_len(const sbn_sumcheck* st) { return st ? st->len : 0; }

}  // extern "C"
// the caller holds the context's mutex; owned_c (or null): a C_par this sumcheck owns (sbn_sumcheck_begin_eq) — released here on every error path
static int sumcheck_begin_locked(sbn_ctx* c, const sbn_table* const* A_par, const sbn_table* const* B_par, const sbn_table* C_par, size_t n_par,
                                 const sbn_table* const* A_seq, const sbn_table* const* B_seq, const sbn_table* const* C_seq, size_t n_seq,
                                 const uint8_t* coeffs, uint8_t out_evals[96], sbn_sumcheck** out, sbn_table* owned_c) {
  TableScope own(c); own.keep(owned_c);
  const size_t ninst = n_par + n_seq;
  if (ninst > (size_t)SC_PACK_MAX) return fail(c, SBN_EINVAL, "sumcheck: %zu instances (at most %d)", ninst, SC_PACK_MAX);
  if (!n_par && !C_seq[0]) return SBN_EINVAL;
  const size_t len = n_par ? C_par->len : C_seq[0]->len;
  for (size_t i = 0; i < n_par; i++) { if (!A_par[i] || !B_par[i]) return SBN_EINVAL; if (A_par[i]->len != len || B_par[i]->len != len) return fail(c, SBN_EINVAL, "sumcheck: tables differ in length"); }
  for (size_t i = 0; i < n_seq; i++) { if (!A_seq[i] || !B_seq[i] || !C_seq[i]) return SBN_EINVAL; if (A_seq[i]->len != len || B_seq[i]->len != len || C_seq[i]->len != len) return fail(c, SBN_EINVAL, "sumcheck: tables differ in length"); }
  if (len < 2 || (len & (len - 1))) return fail(c, SBN_EINVAL, "sumcheck: table length %zu (a power of two >= 2 is needed)", len);
  for (size_t i = 0; i < ninst; i++) if (!fr_canonical(coeffs + 32 * i)) return fail(c, SBN_EINVAL, "sumcheck: coeffs[%zu] is not canonical", i);
  int rc;
  if ((rc = sc_tickets(c))) return rc;
  std::unique_ptr<sbn_sumcheck> st(new sbn_sumcheck());
  st->n_par = n_par; st->n_seq = n_seq; st->ntab = 2 * n_par + (n_par ? 1 : 0) + 3 * n_seq; st->len = st->len0 = len;
  for (size_t i = 0; i < n_par; i++) st->cur.push_back((const uint32_t*)A_par[i]->d);
  for (size_t i = 0; i < n_par; i++) st->cur.push_back((const uint32_t*)B_par[i]->d);
  if (n_par) st->cur.push_back((const uint32_t*)C_par->d);
  for (size_t i = 0; i < n_seq; i++) st->cur.push_back((const uint32_t*)A_seq[i]->d);
  for (size_t i = 0; i < n_seq; i++) st->cur.push_back((const uint32_t*)B_seq[i]->d);
  for (size_t i = 0; i < n_seq; i++) st->cur.push_back((const uint32_t*)C_seq[i]->d);
  bool zero_coeff = false;
  for (size_t i = 0; i < ninst; i++) { st->co.push_back(el_from(coeffs + 32 * i)); st->co_m.push_back(sbn_host::fr::to_m(st->co[i])); if (i < n_par && sbn_host::fr::is_zero(st->co[i])) zero_coeff = true; }
  st->mode = (zero_coeff || n_par == 0) ? 0 : (len >= SC_COMB_MIN_LEN && len / 4 >= sc_comb_min_q() && n_par >= 2) ? 2 : 1;   // (the first bind, len / 4 index pairs, is where COMB mode scales A: it must be a combined round)
  // one slab: per table len/2 + len/4 entries, the groups, and (SCALED mode) full-length copies of the "par" A tables
  const size_t half = len / 2, quarter = std::max<size_t>(len / 4, 1);
  const size_t per_tab = (half + quarter) * 32;
  // the combined kernels' launch plan (mode 2): round-0 sums, then one launch per bind while a round has >= sc_comb_min_q() index pairs
  size_t ngroups_total = 0;
  std::vector<size_t> plan_q;
  if (st->mode == 2) {
    ngroups_total = st->eval_groups = sc_comb_group_count(c, st.get(), len / 2, SC_PACK_MAX - n_seq, nullptr);
    for (size_t q = len / 4; q >= sc_comb_min_q() && q >= 1; q /= 2) {
      plan_q.push_back(q); st->grp_off.push_back(ngroups_total);
      st->grp_cnt.push_back(sc_comb_group_count(c, st.get(), q, SC_PACK_MAX - n_seq, nullptr)); ngroups_total += st->grp_cnt.back();
    }
    if ((n_par + SC_COMB_MAX - 1) / SC_COMB_MAX > SC_PACK_MAX - n_seq) return fail(c, SBN_EINVAL, "sumcheck: %zu par instances do not fit the mailbox next to %zu seq instances", n_par, n_seq);
  }
  size_t bytes = st->ntab * per_tab + (ngroups_total + 1) * sizeof(ScCombGroup) + st->ntab * 32 + 4096;
  if (st->mode == 1) bytes += n_par * len * 32;
  { size_t got = 0; hipError_t e = pool_get(c, bytes, &st->slab, &got); if (e != hipSuccess) { st->slab = nullptr; return fail(c, SBN_ENOMEM, "hipMalloc sumcheck state (%zu bytes): %s", bytes, hipGetErrorString(e)); } st->slab_bytes = got; }
  ScSlabGuard slab_guard{c, st.get()};
  uint8_t* p = (uint8_t*)st->slab;
  for (size_t t = 0; t < st->ntab; t++) { st->buf[0].push_back((uint32_t*)p); p += half * 32; st->buf[1].push_back((uint32_t*)p); p += quarter * 32; }
  st->d_groups = (ScCombGroup*)p; p += ((ngroups_total + 1) * sizeof(ScCombGroup) + 255) / 256 * 256;
  st->d_finals = (uint32_t*)p; p += (st->ntab * 32 + 255) / 256 * 256;
  const uint32_t seq = ++c->mbox_seq;
  std::vector<size_t> inst_ids;
  size_t n_comb = 0;
  if (st->mode == 1) {
    ScScalePack<SC_PACK_MAX> sp; memset(&sp, 0, sizeof sp);
    for (size_t i = 0; i < n_par; i++) {
      st->scaled_copy.push_back((uint32_t*)p); p += len * 32;
      sp.src[i] = st->cur[i]; sp.dst[i] = st->scaled_copy[i]; sp.s[i] = scs_from(sbn_host::fr::to_dev_mont(st->co[i]));
    }
    LAUNCH(c, "k_sc_scale", k_sc_scale, dim3(stream_grid(len), (unsigned)n_par), 256, sp, len);
    LAUNCHCHK(c);
    for (size_t i = 0; i < n_par; i++) st->cur[i] = st->scaled_copy[i];
    st->scaled = true;
  }
  if (st->mode == 2) {
    // "par" group: combined kernel, A scaled in registers; "seq": per-instance kernel
    std::vector<sbn_host::fr::El> u(n_par);
    for (size_t i = 0; i < n_par; i++) u[i] = sbn_host::fr::to_dev_mont(st->co[i]);
    if ((rc = ensure(c, c->sc_partial, SC_PARTIAL_BYTES))) return rc;
    {
      // every group of this sumcheck in ONE upload: the round-0 sums (A scaled in registers: u = c_i) and each combined round
      // (bind j reads the caller's tables for j = 0, the state's buffers after that, and writes buf[j & 1]); only the first bind's
      // u, v depend on the challenge: a one-wave kernel derives them on the device when it arrives (k_sc_first_uv)
      if ((rc = ensure_pin(c, 4096 + (ngroups_total + 1) * sizeof(ScCombGroup)))) return rc;
      ScCombGroup* hg = (ScCombGroup*)((uint8_t*)c->pin + 4096);
      size_t per = 0; n_comb = sc_comb_group_count(c, st.get(), half, SC_PACK_MAX - n_seq, &per);
      sc_comb_groups_fill(st.get(), hg, n_comb, per, st->cur.data(), nullptr, st->cur[2 * n_par], true, u.data(), nullptr);
      if (!plan_q.empty()) {     // the first bind (reads the caller's tables, writes buf[0], scales A): u = c_i for now, k_sc_first_uv finishes u, v once r_0 is known
        sc_comb_group_count(c, st.get(), plan_q[0], SC_PACK_MAX - n_seq, &per);
        sc_comb_groups_fill(st.get(), hg + st->grp_off[0], st->grp_cnt[0], per, st->cur.data(), st->buf[0].data(), st->buf[0][2 * n_par], true, u.data(), nullptr);      // (the scaling first bind reads a pre-bound C: its kernel has no register to spare)
      }
      for (size_t j = 1; j < plan_q.size(); j++) {     // the later binds bind the shared C themselves (no k_bind_oop launch per round)
        sc_comb_group_count(c, st.get(), plan_q[j], SC_PACK_MAX - n_seq, &per);
        sc_comb_groups_fill(st.get(), hg + st->grp_off[j], st->grp_cnt[j], per, (const uint32_t* const*)st->buf[(j - 1) & 1].data(), st->buf[j & 1].data(), st->buf[j & 1][2 * n_par], false, nullptr, nullptr,
                            st->buf[(j - 1) & 1][2 * n_par]);
      }
      HIPCHK(c, hipMemcpyAsync(st->d_groups, hg, ngroups_total * sizeof(ScCombGroup), hipMemcpyHostToDevice, c->stream));
    }
    ScArgsPack pack; memset(&pack, 0, sizeof pack);
    {
      const size_t o = 2 * n_par + 1;
      for (size_t j = 0; j < n_seq; j++) { pack.a[j].t[0] = st->cur[o + j]; pack.a[j].t[1] = st->cur[o + n_seq + j]; pack.a[j].t[2] = st->cur[o + 2 * n_seq + j]; inst_ids.push_back(n_par + j); }
    }
    uint32_t* part2 = (uint32_t*)c->sc_partial.p + (size_t)SC_PACK_MAX * 1024 * 24;         // the second half of the partial-sum area
    if (n_seq && half >= ((size_t)1 << 16)) {
      // both kinds in ONE launch: 0.78-0.83 ms against 0.835-0.875 for the two launches on the 2^21 tables (tools/sc_blocks_sweep.sh MODE=begin);
      // 2.9 GB at 3.6 TB/s: round 0 is VALU-bound (6 products per "seq" index, two scalings per "par" instance)
      const size_t mc = c->sck.comb_eval_blocks_mixed, ms = c->sck.eval_blocks_mixed;
      if ((rc = ensure(c, c->sc_partial, SC_PARTIAL_BYTES))) return rc;
      part2 = (uint32_t*)c->sc_partial.p + (size_t)SC_PACK_MAX * 1024 * 24;
      const size_t cap = (half + 255) / 256;
      const unsigned gxc = (unsigned)std::max<size_t>(1, std::min(std::min(cap, std::max<size_t>(1, mc / n_comb)), SC_PART_COMB_BLOCKS));
      const unsigned gxs = (unsigned)std::max<size_t>(1, std::min(std::min(cap, std::max<size_t>(1, ms / n_seq)), SC_PART_INST_BLOCKS));
      LAUNCH(c, "k_sc_eval_mixed", k_sc_eval_mixed, (unsigned)(n_comb * gxc + n_seq * gxs), 256, (const ScCombGroup*)st->d_groups, (uint32_t)n_comb, gxc, pack, (uint32_t)n_seq, gxs, half,
             (uint32_t*)c->sc_partial.p, part2, (uint32_t*)c->sc_tickets.p, c->mbox, seq);
    } else {
      if (n_seq) { if ((rc = sc_launch_inst_eval(c, pack, n_seq, half, seq))) return rc; part2 = (uint32_t*)c->sc_partial.p + (size_t)SC_PACK_MAX * 1024 * 24; }
      const unsigned gx = (unsigned)std::max<size_t>(1, std::min(std::min<size_t>((half + 255) / 256, std::max<size_t>(1, c->sck.comb_eval_blocks / n_comb)), SC_PART_COMB_BLOCKS));
      LAUNCH(c, "k_sc_comb_eval", k_sc_comb_eval, dim3(gx, (unsigned)n_comb), 256, (const ScCombGroup*)st->d_groups, half, part2, (uint32_t*)c->sc_tickets.p, c->mbox, (uint32_t)n_seq, seq);
    }
    LAUNCHCHK(c);
    // (the staging area is reused by the first bind: by then the mailbox wait below has seen this kernel finish, and the copy runs ahead of it in the stream)
  } else {
    ScArgsPack pack; memset(&pack, 0, sizeof pack);
    const size_t oC = 2 * n_par, o = 2 * n_par + (n_par ? 1 : 0);
    for (size_t i = 0; i < n_par; i++) { pack.a[i].t[0] = st->cur[i]; pack.a[i].t[1] = st->cur[n_par + i]; pack.a[i].t[2] = st->cur[oC]; inst_ids.push_back(i); }
    for (size_t j = 0; j < n_seq; j++) { pack.a[n_par + j].t[0] = st->cur[o + j]; pack.a[n_par + j].t[1] = st->cur[o + n_seq + j]; pack.a[n_par + j].t[2] = st->cur[o + 2 * n_seq + j]; inst_ids.push_back(n_par + j); }
    if ((rc = sc_launch_inst_eval(c, pack, ninst, half, seq))) return rc;
  }
  if (st->mode != 0 && n_par) {
    // 1 / c_i for sbn_sumcheck_finish, by Montgomery's trick (one inversion, ~20 us of host time): here, while round 0 runs on the device
    using namespace sbn_host::fr;
    std::vector<El> pre(n_par + 1); pre[0] = from_u64(1);
    for (size_t i = 0; i < n_par; i++) pre[i + 1] = mmul(to_m(pre[i]), st->co[i]);
    El invall = inv(pre[n_par]);
    st->co_inv_m.resize(n_par);
    for (size_t i = n_par; i-- > 0;) {
      st->co_inv_m[i] = to_m(mmul(to_m(invall), pre[i]));
      invall = mmul(to_m(invall), st->co[i]);
    }
  }
  if ((rc = sc_mbox_wait(c, inst_ids.size() + n_comb, seq))) return rc;
  sc_combine_host(st.get(), (const uint8_t*)c->mbox, inst_ids, n_comb, out_evals);
  memcpy(st->evals0, out_evals, 96);
  slab_guard.armed = false;
  if (owned_c) st->owned_c = own.give(owned_c);
  *out = st.release();
  return own.done();
}
// ---- one round's launches, shared by sbn_sumcheck_round (challenge in the kernel arguments, sums to the host mailbox) and
// sbn_sumcheck_prove (challenge in device memory, sums to the mailbox's device twin): the same kernels, grids and order ----
struct ScRoundPlan { std::vector<size_t> inst_ids; size_t n_comb = 0; bool comb = false; };
// the last bind + final claims (two entries per table left): one launch; fin_out / flag: host mailbox or device memory
template <class RS>
static int sc_final_enqueue(sbn_ctx* c, sbn_sumcheck* st, const RS& rs, uint32_t* fin_out, uint32_t* flag, uint32_t fseq) {
  ScFinalPack fp; memset(&fp, 0, sizeof fp);
  for (size_t t = 0; t < st->ntab; t++) fp.src[t] = st->cur[t];
  LAUNCH(c, "k_bind_top", k_sc_bind_finals, 1, 128, fp, (uint32_t)st->ntab, rs, st->d_finals, fin_out, flag, fseq);
  LAUNCHCHK(c);
  return SBN_OK;
}
static void sc_final_advance(sbn_sumcheck* st) {
  for (size_t t = 0; t < st->ntab; t++) st->cur[t] = st->d_finals + 8 * t;
  st->len /= 2; st->binds++;
}
// a bind round with >= 4 entries per table: binds to rs and leaves the next round's sums in mbox slots [0, inst_ids.size() + n_comb)
template <class RS>
static int sc_round_enqueue(sbn_ctx* c, sbn_sumcheck* st, const RS& rs, uint32_t* mbox, uint32_t seq, ScRoundPlan& plan) {
  const size_t n_par = st->n_par, n_seq = st->n_seq, ninst = n_par + n_seq, len = st->len;
  std::vector<uint32_t*>& dst = st->buf[st->binds & 1];
  std::vector<size_t>& inst_ids = plan.inst_ids;
  size_t& n_comb = plan.n_comb;
  int rc;
  const size_t q = len / 4;
  const size_t oC = 2 * n_par, o = 2 * n_par + (n_par ? 1 : 0);
  const bool comb = st->mode == 2 && q >= sc_comb_min_q();
  if (st->mode == 2 && !comb && !st->scaled) return fail(c, SBN_EINVAL, "sumcheck: internal: unscaled tables below the combined kernels' range");
  if (comb) {
    // shared C: bound inside the round kernel (every group binds its entries, group 0 stores them), except by the scaling first bind: once ahead of it
    if (!st->scaled) LAUNCH(c, "k_bind_oop", k_bind_oop, stream_grid(len / 2), 256, st->cur[oC], dst[oC], len / 2, rs);
    const bool scale_now = !st->scaled;
    if ((rc = ensure(c, c->sc_partial, SC_PARTIAL_BYTES))) return rc;
    const size_t jr = (size_t)st->binds;
    if (jr >= st->grp_cnt.size()) return fail(c, SBN_EINVAL, "sumcheck: internal: no group plan for bind %zu", jr);
    n_comb = st->grp_cnt[jr];
    const ScCombGroup* d_grp = st->d_groups + st->grp_off[jr];
    if (scale_now) {
      // the first bind scales A: its groups (uploaded when the sumcheck began, u = c_i) get u = c (1 - r), v = c r on the device
      if (jr != 0) return fail(c, SBN_EINVAL, "sumcheck: internal: unscaled tables after the first bind");
      LAUNCH(c, "k_sc_first_uv", k_sc_first_uv, (unsigned)n_comb, 64, (ScCombGroup*)d_grp, rs);
    }
    ScFusedPack seqpack; memset(&seqpack, 0, sizeof seqpack);
    for (size_t j = 0; j < n_seq; j++) {
      const size_t ids[3] = {o + j, o + n_seq + j, o + 2 * n_seq + j};
      for (int t = 0; t < 3; t++) { seqpack.a[j].src[t] = st->cur[ids[t]]; seqpack.a[j].dst[t] = dst[ids[t]]; }
      inst_ids.push_back(n_par + j);
    }
    // streaming rounds with both kinds of instance: ONE grid, the VALU-bound "seq" blocks interleaved with the memory-bound "par" blocks
    const bool mixed = n_seq > 0 && q > SC_SINGLE_LAUNCH_MAX / 2;
    if (n_seq && !mixed) { if ((rc = sc_launch_inst_fused(c, seqpack, n_seq, q, rs, mbox, seq))) return rc; }
    // grid: 512 blocks for the "par" groups + 512 for the "seq" instances = two block rounds of the 512 resident blocks.  Every block
    // ends in a ~7 us epilogue (three wave sums, write-through stores, the ticket), so the 3070 blocks of the first version cost ~40 us
    // per launch whatever the table size (t = 40 us + bytes / 4.4 TB/s over the six streaming rounds); and EQUAL counts do best
    // (tools/sc_blocks_sweep.sh: 512:512 3.77-3.95 ms per sumcheck, 1024:2048 3.99-4.02, 512:768 4.01, 512:256 4.26).  Both kinds end up
    // evenly spread over the 8 XCDs and finish within 2 % of each other (per-block clocks: 930 / 912 us on the 2^21 tables);
    // forcing one long + one short block per slot, or one kind per XCD, changes nothing (4.04 against 4.01 ms)
    const size_t comb_blocks = c->sck.comb_blocks, seq_blocks = c->sck.seq_blocks;
    size_t want = std::max<size_t>(1, comb_blocks / n_comb), cap = (q + 255) / 256;
    if (c->sck.comb_grid) want = c->sck.comb_grid;
    const unsigned gx = (unsigned)std::max<size_t>(1, std::min(std::min(want, cap), SC_PART_COMB_BLOCKS));
    uint32_t* part2 = (uint32_t*)c->sc_partial.p + (size_t)SC_PACK_MAX * 1024 * 24;
    if (mixed) {
      const size_t capq = (q + 255) / 256;
      const unsigned gx_seq = (unsigned)std::max<size_t>(1, std::min(std::min<size_t>(seq_blocks / n_seq, capq), SC_PART_INST_BLOCKS));
      const unsigned total = (unsigned)(n_comb * gx + n_seq * gx_seq);
      if (scale_now) LAUNCH(c, "k_sc_round_mixed_first", (k_sc_round_mixed<true, RS>), total, 256, d_grp, (uint32_t)n_comb, gx, seqpack, (uint32_t)n_seq, gx_seq, q, rs, (uint32_t*)c->sc_partial.p, part2, (uint32_t*)c->sc_tickets.p, mbox, seq);
      else LAUNCH(c, "k_sc_round_mixed", (k_sc_round_mixed<false, RS>), total, 256, d_grp, (uint32_t)n_comb, gx, seqpack, (uint32_t)n_seq, gx_seq, q, rs, (uint32_t*)c->sc_partial.p, part2, (uint32_t*)c->sc_tickets.p, mbox, seq);
    } else
    if (scale_now) LAUNCH(c, "k_sc_comb_bind_eval_first", (k_sc_comb_bind_eval<true, RS>), dim3(gx, (unsigned)n_comb), 256, d_grp, q, rs, part2, (uint32_t*)c->sc_tickets.p, mbox, (uint32_t)n_seq, seq);
    else LAUNCH(c, "k_sc_comb_bind_eval", (k_sc_comb_bind_eval<false, RS>), dim3(gx, (unsigned)n_comb), 256, d_grp, q, rs, part2, (uint32_t*)c->sc_tickets.p, mbox, (uint32_t)n_seq, seq);
    LAUNCHCHK(c);
  } else {
    // per-instance kernels for everything; a shared C of a streaming round is bound ahead (every table needs a writer there)
    const bool single = q <= SC_SINGLE_LAUNCH_MAX / 2;
    const bool prebind = n_par >= 2 && !single;
    if (prebind) LAUNCH(c, "k_bind_oop", k_bind_oop, stream_grid(len / 2), 256, st->cur[oC], dst[oC], len / 2, rs);
    ScFusedPack pack; memset(&pack, 0, sizeof pack);
    for (size_t i = 0; i < n_par; i++) {
      pack.a[i].src[0] = st->cur[i]; pack.a[i].dst[0] = dst[i];
      pack.a[i].src[1] = st->cur[n_par + i]; pack.a[i].dst[1] = dst[n_par + i];
      if (prebind) { pack.a[i].src[2] = dst[oC]; pack.a[i].pre[2] = 1; }
      else { pack.a[i].src[2] = st->cur[oC]; pack.a[i].dst[2] = i == 0 ? dst[oC] : nullptr; }
      inst_ids.push_back(i);
    }
    for (size_t j = 0; j < n_seq; j++) {
      const size_t ids[3] = {o + j, o + n_seq + j, o + 2 * n_seq + j};
      for (int t = 0; t < 3; t++) { pack.a[n_par + j].src[t] = st->cur[ids[t]]; pack.a[n_par + j].dst[t] = dst[ids[t]]; }
      inst_ids.push_back(n_par + j);
    }
    if ((rc = sc_launch_inst_fused(c, pack, ninst, q, rs, mbox, seq))) return rc;
  }
  plan.comb = comb;
  return SBN_OK;
}
// the state moves on all at once: tables, length, and (a combined round has folded c_i into A_i) the scaled flag
static void sc_round_advance(sbn_sumcheck* st, const ScRoundPlan& plan) {
  std::vector<uint32_t*>& dst = st->buf[st->binds & 1];
  for (size_t t = 0; t < st->ntab; t++) st->cur[t] = dst[t];
  st->len /= 2; st->binds++;
  if (plan.comb) st->scaled = true;
}
// the final claims as the last round delivered them (k_sc_bind_finals), A_i[0] = A'_i[0] / c_i where the state scaled A
static int sc_finals_deliver(sbn_ctx* c, const sbn_sumcheck* st, uint8_t* finals) {
  memcpy(finals, st->finals_host.data(), st->ntab * 32);          // nothing to launch or wait for here
  if (st->scaled) {
    using namespace sbn_host::fr;
    if (st->co_inv_m.size() != st->n_par) return fail(c, SBN_EINVAL, "sumcheck finish: internal: scaled tables without the inverse coefficients");
    for (size_t i = 0; i < st->n_par; i++) { const El a = mmul(st->co_inv_m[i], el_from(finals + 32 * i)); memcpy(finals + 32 * i, a.v, 32); }
  }
  return SBN_OK;
}
extern "C" {
int sbn_sumcheck_begin(sbn_ctx* c, const sbn_table* const* A_par, const sbn_table* const* B_par, const sbn_table* C_par, size_t n_par,
                       const sbn_table* const* A_seq, const sbn_table* const* B_seq, const sbn_table* const* C_seq, size_t n_seq,
                       const uint8_t* coeffs, uint8_t out_evals[96], sbn_sumcheck** out) {
  if (!c || !coeffs || !out_evals || !out || n_par + n_seq == 0) return SBN_EINVAL;
  if ((n_par && (!A_par || !B_par || !C_par)) || (n_seq && (!A_seq || !B_seq || !C_seq))) return SBN_EINVAL;
  std::lock_guard<std::mutex> g(c->mu); hipSetDevice(c->device);
  return sumcheck_begin_locked(c, A_par, B_par, C_par, n_par, A_seq, B_seq, C_seq, n_seq, coeffs, out_evals, out, nullptr);
}
// The same with poly_C_par = EqPolynomial::new(rand).evals() (product_tree.rs:267-275: every layer's sumcheck of
// ProductCircuitEvalProofBatched::prove builds its C this way) built INSIDE the call from the challenge vector: the eq kernels and round 0
// are enqueued back to back, the table belongs to the state.  The final claims list C_par[0] as sbn_sumcheck_begin does.
int sbn_sumcheck_begin_eq(sbn_ctx* c, const sbn_table* const* A_par, const sbn_table* const* B_par, size_t n_par, const uint8_t* rand, size_t ell,
                          const sbn_table* const* A_seq, const sbn_table* const* B_seq, const sbn_table* const* C_seq, size_t n_seq,
                          const uint8_t* coeffs, uint8_t out_evals[96], sbn_sumcheck** out) {
  if (!c || !coeffs || !out_evals || !out || n_par == 0 || !A_par || !B_par || (!rand && ell) || ell > 40) return SBN_EINVAL;
  if (n_seq && (!A_seq || !B_seq || !C_seq)) return SBN_EINVAL;
  std::lock_guard<std::mutex> g(c->mu); hipSetDevice(c->device);
  if (!A_par[0] || A_par[0]->len != ((size_t)1 << ell)) return fail(c, SBN_EINVAL, "sumcheck: rand has %zu entries, the tables 2^%zu are expected to have %zu  [product_tree.rs:268 assert_eq]", ell, ell, (size_t)1 << ell);
  sbn_table* eq = nullptr;
  int rc = eq_evals_locked(c, rand, ell, &eq);
  if (rc) return rc;
  return sumcheck_begin_locked(c, A_par, B_par, eq, n_par, A_seq, B_seq, C_seq, n_seq, coeffs, out_evals, out, eq);
}

int sbn_sumcheck_round(sbn_ctx* c, sbn_sumcheck* st, const uint8_t r[32], uint8_t out_evals[96]) {
  if (!c || !st || !r || !out_evals) return SBN_EINVAL;
  std::lock_guard<std::mutex> g(c->mu); hipSetDevice(c->device);
  if (st->len < 2) return fail(c, SBN_EINVAL, "sumcheck round: no variable left");
  if (!fr_canonical(r)) return fail(c, SBN_EINVAL, "challenge scalar is not canonical (>= r)");
  using namespace sbn_host::fr;
  const size_t len = st->len;
  const El rc_ = el_from(r);
  const ScScalar rs = scs_from(to_dev_mont(rc_));
  int rc;
  memset(out_evals, 0, 96);
  ScRoundGuard round_guard{st};         // from here on an error return leaves the state dead: the arguments were fine, something below failed
  if (len < 4) {
    // last round: bind (out of place: the tables may still be the caller's) and deliver the final claims — one launch, one wait
    if ((rc = sc_tickets(c))) return rc;
    const uint32_t fseq = ++c->mbox_seq;
    uint32_t* hfin = c->mbox + SC_MBOX_FINALS;
    if ((rc = sc_final_enqueue(c, st, rs, hfin, c->mbox + SC_MBOX_FLAGS + SC_PACK_MAX, fseq))) return rc;
    if ((rc = sc_flag_wait(c, c->mbox + SC_MBOX_FLAGS + SC_PACK_MAX, fseq))) return rc;
    st->finals_host.assign((const uint8_t*)hfin, (const uint8_t*)hfin + st->ntab * 32);
    sc_final_advance(st);
    round_guard.ok = true;
    return SBN_OK;
  }
  const uint32_t seq = ++c->mbox_seq;
  ScRoundPlan plan;
  if ((rc = sc_round_enqueue(c, st, rs, c->mbox, seq, plan))) return rc;
  if ((rc = sc_mbox_wait(c, plan.inst_ids.size() + plan.n_comb, seq))) return rc;
  sc_combine_host(st, (const uint8_t*)c->mbox, plan.inst_ids, plan.n_comb, out_evals);
  sc_round_advance(st, plan);
  round_guard.ok = true;
  return SBN_OK;
}

int sbn_sumcheck_finish(sbn_ctx* c, sbn_sumcheck* st, uint8_t* finals) {
  if (!c || !st || !finals) return SBN_EINVAL;
  std::lock_guard<std::mutex> g(c->mu); hipSetDevice(c->device);
  if (st->len != 1) return fail(c, SBN_EINVAL, "sumcheck finish: %zu entries left (bind every variable first)", st->len);
  if (st->finals_host.size() != st->ntab * 32) return fail(c, SBN_EINVAL, "sumcheck finish: internal: the last round left no final claims");
  return sc_finals_deliver(c, st, finals);
}

int sbn_table_read0_many(sbn_ctx* c, const sbn_table* const* ts, size_t count, uint8_t* out) {
  if (!c || !ts || !out) return SBN_EINVAL;
  std::lock_guard<std::mutex> g(c->mu); hipSetDevice(c->device);
  for (size_t i = 0; i < count; i++) if (!ts[i] || ts[i]->len == 0) return fail(c, SBN_EINVAL, "read0_many: table %zu is null or empty", i);
  int rc; if ((rc = sc_tickets(c))) return rc;
  for (size_t o = 0; o < count; o += 64) {
    const size_t m = std::min<size_t>(64, count - o);
    ScRead0Pack pk; memset(&pk, 0, sizeof pk);
    for (size_t i = 0; i < m; i++) pk.p[i] = (const uint32_t*)ts[o + i]->d;
    const uint32_t seq = ++c->mbox_seq;
    uint32_t* hfin = c->mbox + SC_MBOX_FINALS;
    LAUNCH(c, "k_fr_from_mont", k_sc_finals_gather, 1, 128, pk, (uint32_t)m, hfin, c->mbox + SC_MBOX_FLAGS + SC_PACK_MAX, seq);
    LAUNCHCHK(c);
    if ((rc = sc_flag_wait(c, c->mbox + SC_MBOX_FLAGS + SC_PACK_MAX, seq))) return rc;
    memcpy(out + 32 * o, hfin, m * 32);
  }
  return SBN_OK;
}

}  // extern "C"

// ---- the whole sumcheck in one call: every round's kernels and the transcript step between them queued at once ----------------
// which mailbox slots bind round `binds` of a state fills (what sc_round_enqueue will do, known ahead: it depends on lengths only)
static void sc_round_slots(const sbn_ctx* c, const sbn_sumcheck* st, size_t len, size_t binds, std::vector<size_t>& inst_ids, size_t& n_comb, bool& comb) {
  inst_ids.clear(); n_comb = 0;
  comb = st->mode == 2 && len / 4 >= sc_comb_min_q();
  if (comb) { for (size_t j = 0; j < st->n_seq; j++) inst_ids.push_back(st->n_par + j); n_comb = binds < st->grp_cnt.size() ? st->grp_cnt[binds] : 0; }
  else for (size_t i = 0; i < st->n_par + st->n_seq; i++) inst_ids.push_back(i);
}
extern "C" {

int sbn_sumcheck_prove(sbn_ctx* c, sbn_sumcheck* st, sbn_transcript* tr, const uint8_t claim[32], uint8_t* out_polys, uint8_t* out_r, uint8_t* finals) {
  if (!c || !st || !tr || !claim || !out_polys || !out_r || !finals) return SBN_EINVAL;
  std::lock_guard<std::mutex> g(c->mu); hipSetDevice(c->device);
  if (st->len < 2 || st->binds != 0 || st->len != st->len0) return fail(c, SBN_EINVAL, "sumcheck prove: the state has been advanced already (or is dead); it takes a state fresh from sbn_sumcheck_begin");
  if (!fr_canonical(claim)) return fail(c, SBN_EINVAL, "sumcheck prove: the claim is not canonical (>= r)");
  using namespace sbn_host::fr;
  size_t rounds = 0; while (((size_t)1 << rounds) < st->len) rounds++;
  int rc;
  if ((rc = sc_tickets(c))) return rc;
  // the transcript's plan: the first round starts at the caller's phase, every later one behind a PRF (pos 64)
  std::vector<uint8_t> masks_first, masks_next; uint8_t end[3], end2[3];
  transcript_plan_round(tr->t.s.pos, tr->t.s.pos_begin, tr->t.s.cur_flags, masks_first, end);
  transcript_plan_round(end[0], end[1], end[2], masks_next, end2);
  const size_t nblk_first = masks_first.size() / 200, nblk_next = masks_next.size() / 200;
  if (nblk_first < 1 || nblk_first > 3 || nblk_next != 2 || memcmp(end, end2, 3)) return fail(c, SBN_EINVAL, "sumcheck prove: internal: unexpected transcript plan (%zu, %zu blocks)", nblk_first, nblk_next);
  // device layout: [claim, round-0 sums | masks | weights per step] uploaded, [sponge state] both ways, [polys | r | finals | flag] downloaded, then r_j and the mailbox's twin
  const size_t o_claim = 0, o_sums0 = 64, o_masks = 256, o_w = o_masks + 1280, o_strobe = o_w + rounds * SC_PACK_MAX * 32, o_polys = o_strobe + 256,
               o_r = o_polys + rounds * 128, o_fin = o_r + rounds * 32, o_flag = o_fin + (size_t)SC_FINAL_MAX * 32, o_rm = o_flag + 256, o_mbox = o_rm + 256, total = o_mbox + (size_t)SC_MBOX_WORDS * 4;
  if ((rc = ensure(c, c->sc_prove, total))) return rc;
  if ((rc = ensure_pin(c, 4096 + total))) return rc;
  uint8_t* d = (uint8_t*)c->sc_prove.p; uint8_t* h = (uint8_t*)c->pin + 4096;
  memset(h, 0, o_polys);
  {                                       // e travels as fp.cuh's nine 29-bit limbs (the step keeps it lazy between rounds)
    const El cm = to_dev_mont(el_from(claim));
    uint32_t limbs[9];
    for (int k = 0; k < 9; k++) { const int bit = 29 * k, i = bit >> 6, sh = bit & 63; uint64_t x = cm.v[i] >> sh; if (sh > 35 && i + 1 < 4) x |= cm.v[i + 1] << (64 - sh); limbs[k] = (uint32_t)x & 0x1fffffffu; }
    memcpy(h + o_claim, limbs, 36);
  }
  memcpy(h + o_sums0, st->evals0, 96);
  memcpy(h + o_masks, masks_first.data(), masks_first.size());
  memcpy(h + o_masks + 600, masks_next.data(), masks_next.size());
  memcpy(h + o_strobe, tr->t.s.st, 200);
  // weights of step j's slots: c_i R^2 where the host would weight the slot, R^2 where it would only add (the sums arrive as plain integers)
  const El w_one = to_dev_mont(to_dev_mont(from_u64(1)));
  std::vector<uint32_t> nslots(rounds, 1);
  memcpy(h + o_w, w_one.v, 32);
  {
    size_t len = st->len, binds = 0; bool scaled = st->scaled;
    std::vector<size_t> ids; size_t n_comb; bool comb;
    for (size_t j = 1; j < rounds; j++, len /= 2, binds++) {
      sc_round_slots(c, st, len, binds, ids, n_comb, comb);
      uint8_t* w = h + o_w + j * SC_PACK_MAX * 32;
      if (ids.size() + n_comb > (size_t)SC_PACK_MAX) return fail(c, SBN_EINVAL, "sumcheck prove: internal: %zu result slots", ids.size() + n_comb);
      for (size_t s = 0; s < ids.size(); s++) {
        const bool weighted = !(ids[s] < st->n_par && scaled);
        const El x = weighted ? to_dev_mont(to_dev_mont(st->co[ids[s]])) : w_one;
        memcpy(w + 32 * s, x.v, 32);
      }
      for (size_t k = 0; k < n_comb; k++) memcpy(w + 32 * (ids.size() + k), w_one.v, 32);
      nslots[j] = (uint32_t)(ids.size() + n_comb);
      if (comb) scaled = true;
    }
  }
  HIPCHK(c, hipMemcpyAsync(d, h, o_polys, hipMemcpyHostToDevice, c->stream));
  ScRoundGuard round_guard{st};         // from the first launch on a failure leaves tables half bound: the state is dead, the transcript untouched
  const ScScalarDev rs{(const uint32_t*)(d + o_rm)};
  uint32_t* dmbox = (uint32_t*)(d + o_mbox);
  for (size_t j = 0; j < rounds; j++) {
    TrStepArgs a;
    a.sums = j == 0 ? (const uint32_t*)(d + o_sums0) : dmbox;
    a.weights = (const uint32_t*)(d + o_w + j * SC_PACK_MAX * 32); a.nslots = nslots[j];
    a.masks = d + o_masks + (j == 0 ? 0 : 600); a.nblk = (uint32_t)(j == 0 ? nblk_first : nblk_next); a.pos0 = j == 0 ? tr->t.s.pos : end[0];
    a.strobe = d + o_strobe; a.claim = (uint32_t*)(d + o_claim); a.r_mont = (uint32_t*)(d + o_rm);
    a.out_poly = (uint32_t*)(d + o_polys + j * 128); a.out_r = (uint32_t*)(d + o_r + j * 32);
    LAUNCH(c, "k_tr_sumcheck_step", k_tr_sumcheck_step, 1, 64, a);
    if (st->len >= 4) {
      const uint32_t seq = ++c->mbox_seq;
      ScRoundPlan plan;
      if ((rc = sc_round_enqueue(c, st, rs, dmbox, seq, plan))) return rc;
      if (j + 1 < rounds && plan.inst_ids.size() + plan.n_comb != nslots[j + 1]) return fail(c, SBN_EINVAL, "sumcheck prove: internal: round %zu filled %zu slots, %u were planned", j, plan.inst_ids.size() + plan.n_comb, nslots[j + 1]);
      sc_round_advance(st, plan);
    } else {
      const uint32_t fseq = ++c->mbox_seq;
      if ((rc = sc_final_enqueue(c, st, rs, (uint32_t*)(d + o_fin), (uint32_t*)(d + o_flag), fseq))) return rc;
      sc_final_advance(st);
    }
  }
  LAUNCHCHK(c);
  // one copy back, one wait
  HIPCHK(c, hipMemcpyAsync(h + o_strobe, d + o_strobe, o_flag - o_strobe, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  if (c->prof) prof_drain(c);
  st->finals_host.assign(h + o_fin, h + o_fin + st->ntab * 32);
  if ((rc = sc_finals_deliver(c, st, finals))) return rc;
  memcpy(out_polys, h + o_polys, rounds * 128);
  memcpy(out_r, h + o_r, rounds * 32);
  memcpy(tr->t.s.st, h + o_strobe, 200); tr->t.s.pos = end[0]; tr->t.s.pos_begin = end[1]; tr->t.s.cur_flags = end[2];
  round_guard.ok = true;
  return SBN_OK;
}

}  // extern "C"
