// abi_product_proof.inc — C ABI: ProductCircuitEvalProofBatched::prove (product_tree.rs:251-392) as ONE device-resident job.
//
// Per layer (top first) the reference draws coeff_vec and the joint claim (:317-321), runs prove_cubic_batched on the layer's halves
// with poly_C_par = eq(rand) (:271, :323-332), appends the final claims (:352-365), draws r_layer and folds the claims (:368-376).
// Here every value that flows from one layer into the next stays on the device:
//   k_tr_layer_step (transcript_kernels.cuh)   close of layer j+1 and open of layer j in one one-wave launch
//   k_eq_*_dev                                 EqPolynomial::evals from the point the steps left in memory (canonical integers)
//   k_sc_eval / the round kernels / k_tr_sumcheck_step / k_sc_bind_finals   exactly what sbn_sumcheck_prove queues, on a PLAIN-mode state
// Modes (abi_sumcheck.inc).  A layer whose tables have >= 2^16 entries (and >= PP_COMB_MIN_CIRC circuits) runs in COMB mode, as sbn_sumcheck_begin would
// choose: the combined kernels, c_i folded into A_i.  Its groups are planned on the host and uploaded with the job; the c_i they scale by
// are copied in on the device from what the open step left in memory (k_pp_fill_u), k_sc_first_uv finishes the first bind's u, v as before.
// The final claims then hold c_i A_i[0]: 1 / c_i comes from Montgomery's trick with ONE Fermat inversion on a lone wave (k_pp_inv, ~0.2 ms),
// launched on a second stream of the context as soon as the coefficients exist and joined by an event before k_pp_unscale and the close
// step — such a layer's sumcheck takes longer than the inversion.  Every shorter layer runs in PLAIN mode (nothing scaled, the step weights
// every instance's sums): too short to hide an inversion.  The outputs are the same field elements either way.
// A zero coefficient cannot be divided out.  The host never sees c_i, so k_pp_inv raises a flag that is read after the one wait, and the
// job is run again with every layer in PLAIN mode (which needs no division).  Probability 2^-254 per coefficient; a real transcript cannot
// be steered there, so this path is REVIEWED, NOT TESTED.
// Buffers (one sumcheck slab and one eq table sized by the largest layer, the plan records, the outputs) are taken before the first launch.

// COMB layers from this many circuits on.  Measured (DESIGN 4.10): with 12 circuits the combined kernels win back 0.3 ms of a 17.8 ms proof; with 4
// the per-instance kernels cost the same and the COMB layer's extra launches and the two cross-stream events cost 0.15 ms per layer.
static const size_t PP_COMB_MIN_CIRC = 8;
struct PpRead0Pack { const uint32_t* p[SC_FINAL_MAX]; };
// the zero-round layer's "final claims": entry 0 of every table, as canonical integers in the order of a sumcheck's finals (null: the shared eq table, 1)
__global__ void __launch_bounds__(128) k_pp_read0(PpRead0Pack pk, uint32_t count, uint32_t* __restrict__ out) {
  const uint32_t t = threadIdx.x;
  const uint32_t* z = nullptr;
#pragma unroll
  for (int i = 0; i < SC_FINAL_MAX; i++) if (i == (int)t) z = pk.p[i];
  if (t < count) fe_store_packed<FrP>(out + 8 * t, z ? fe_from_mont(fe_load<FrP>(z)) : fe_small<FrP>(1u));
}
// DotProductCircuit::evaluate (product_tree.rs:99-103): partial[(circuit * gridDim.x + block)] = sum over the block's indices of left * right * weight
__global__ void __launch_bounds__(256) k_pp_dotp(ScArgsPack pack, size_t n, uint32_t* __restrict__ partial) {
  __shared__ uint32_t sm[4][NL];
  ScArgs a;
#pragma unroll
  for (int i = 0; i < SC_PACK_MAX; i++) if (i == (int)blockIdx.y) a = pack.a[i];
  Fr acc = fe_zero<FrP>();
  uint32_t cnt = 0;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x)
    fr_acc(acc, fe_mul(fe_mul(fe_gload<FrP>(a.t[0] + 8 * i), fe_gload<FrP>(a.t[1] + 8 * i)), fe_gload<FrP>(a.t[2] + 8 * i)), cnt);
  acc = wave_sum_fr(fe_reduce(acc));
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  if (lane == 0) for (int k = 0; k < NL; k++) sm[wv][k] = acc.v[k];
  __syncthreads();
  if (threadIdx.x == 0) {
    Fr s = fe_zero<FrP>();
    for (int w = 0; w < 4; w++) { Fr x; for (int k = 0; k < NL; k++) x.v[k] = sm[w][k]; s = fe_add(s, x); }
    fe_store_tab<FrP>(partial + 8 * ((size_t)blockIdx.y * gridDim.x + blockIdx.x), fe_reduce(s));
  }
}
// claims_to_verify before the first layer (product_tree.rs:262-264, :296-299), table format: block i < n_circ: ProductCircuit::evaluate =
// the product of the top layer's two entries; block n_circ + k: the fold of dot-product circuit k's partial sums
__global__ void __launch_bounds__(64) k_pp_claims0(PpRead0Pack top, uint32_t n_circ, const uint32_t* __restrict__ partial, uint32_t nblk, uint32_t* __restrict__ claims) {
  const uint32_t i = blockIdx.x, lane = threadIdx.x;
  if (i < n_circ) {
    const uint32_t* z = nullptr;
#pragma unroll
    for (int k = 0; k < SC_PACK_MAX; k++) if (k == (int)i) z = top.p[k];
    if (lane == 0) fe_store_tab<FrP>(claims + 8 * i, fe_mul(fe_load<FrP>(z), fe_load<FrP>(z + 8)));
    return;
  }
  Fr s = fe_zero<FrP>();
  for (uint32_t b = lane; b < nblk; b += 64) s = fe_add(s, fe_load<FrP>(partial + 8 * ((size_t)(i - n_circ) * nblk + b)));     // <= 16 terms below 2.5 r
  s = wave_sum_fr(fe_reduce(s));
  if (lane == 0) fe_store_tab<FrP>(claims + 8 * i, fe_reduce(s));
}
// EqPolynomial::evals (hyrax.rs:355-369) from a point in device memory: r[j] = 8 words, canonical integers (what the step kernels
// write as out_r).  The kernels are k_eq_direct / k_eq_level / k_eq_level2 with the point read and brought to Montgomery form per thread.
__device__ __forceinline__ Fr eq_point_dev(const uint32_t* r, int j) { return fe_to_mont(fe_load<FrP>(r + 8 * j)); }
__global__ void __launch_bounds__(256) k_eq_direct_dev(const uint32_t* __restrict__ r, int m, uint32_t* __restrict__ out) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= ((size_t)1 << m)) return;
  const Fr one = fe_one<FrP>();
  Fr acc = one;
  for (int j = 0; j < m; j++) {
    const Fr rj = eq_point_dev(r, j);
    acc = fe_mul(acc, ((i >> (m - 1 - j)) & 1) ? rj : fe_sub(one, rj));
  }
  fe_store_tab<FrP>(out + 8 * i, acc);
}
__global__ void __launch_bounds__(256) k_eq_level_dev(const uint32_t* __restrict__ in, uint32_t* __restrict__ out, size_t size_in, const uint32_t* __restrict__ r, int j) {
  const Fr rj = eq_point_dev(r, j);
  for (size_t k = (size_t)blockIdx.x * blockDim.x + threadIdx.x; k < size_in; k += (size_t)gridDim.x * blockDim.x) {
    const Fr s = fe_load<FrP>(in + 8 * k);
    const Fr hi = fe_mul(s, rj);
    fe_store_tab<FrP>(out + 8 * (2 * k + 1), hi);
    fe_store_tab<FrP>(out + 8 * (2 * k), fe_sub_lazy(s, hi));
  }
}
__global__ void __launch_bounds__(256) k_eq_level2_dev(const uint32_t* __restrict__ in, uint32_t* __restrict__ out, size_t size_in, const uint32_t* __restrict__ r, int j) {
  const Fr r0 = eq_point_dev(r, j), r1 = eq_point_dev(r, j + 1);
  for (size_t k = (size_t)blockIdx.x * blockDim.x + threadIdx.x; k < size_in; k += (size_t)gridDim.x * blockDim.x) {
    const Fr s = fe_load<FrP>(in + 8 * k);
    const Fr h = fe_mul(s, r0), l = fe_sub(s, h);
    const Fr hh = fe_mul(h, r1), lh = fe_mul(l, r1);
    fe_store_tab<FrP>(out + 8 * (4 * k), fe_sub_lazy(l, lh));
    fe_store_tab<FrP>(out + 8 * (4 * k + 1), lh);
    fe_store_tab<FrP>(out + 8 * (4 * k + 2), fe_sub_lazy(h, hh));
    fe_store_tab<FrP>(out + 8 * (4 * k + 3), hh);
  }
}
// the eq table of r[0 .. ell) into `dst` (2^ell entries), `tmp` the ping-pong partner of the same size; the caller holds the mutex
static int eq_evals_dev_enqueue(sbn_ctx* c, const uint32_t* r, size_t ell, uint32_t* dst, uint32_t* tmp) {
  const size_t m = std::min<size_t>(ell, EQ_DIRECT_MAX);
  size_t passes = 0; for (size_t j = m; j < ell; ) { j += (ell - j >= 2) ? 2 : 1; passes++; }
  uint32_t* cur = (passes % 2 == 0) ? dst : tmp;
  LAUNCH(c, "k_eq_level", k_eq_direct_dev, (unsigned)((((size_t)1 << m) + 255) / 256), 256, r, (int)m, cur);
  size_t size = (size_t)1 << m;
  for (size_t j = m; j < ell; ) {
    uint32_t* nxt = (cur == dst) ? tmp : dst;
    if (ell - j >= 2) { LAUNCH(c, "k_eq_level", k_eq_level2_dev, stream_grid(size), 256, (const uint32_t*)cur, nxt, size, r, (int)j); size *= 4; j += 2; }
    else { LAUNCH(c, "k_eq_level", k_eq_level_dev, stream_grid(size), 256, (const uint32_t*)cur, nxt, size, r, (int)j); size *= 2; j += 1; }
    cur = nxt;
  }
  LAUNCHCHK(c);
  return SBN_OK;
}

// u[k] = c_{first + k} for the groups that scale A by c_i (the round-0 sums and the first bind): group g of the launch covers the instances
// [g * per, g * per + n); the host wrote everything else of the group
__global__ void __launch_bounds__(64) k_pp_fill_u(ScCombGroup* __restrict__ groups, uint32_t per, const uint32_t* __restrict__ coeffs_mont) {
  ScCombGroup* g = groups + blockIdx.x;
  const uint32_t k = threadIdx.x;
  if (k >= g->n || k >= (uint32_t)SC_COMB_MAX) return;
  const uint4* src = reinterpret_cast<const uint4*>(coeffs_mont + 8 * ((size_t)blockIdx.x * per + k));
  uint4* dst = reinterpret_cast<uint4*>(g->u[k]);
  dst[0] = src[0]; dst[1] = src[1];
}
// 1 / c_i for i < n by Montgomery's trick: prefix products, one Fermat inversion, back-substitution.  One lane.  flag = 1 when a c_i is zero
// (the product is zero): the inverses are meaningless then and the host runs the job again without them.
__global__ void __launch_bounds__(64) k_pp_inv(const uint32_t* __restrict__ coeffs_mont, uint32_t n, uint32_t* __restrict__ inv_out, uint32_t* __restrict__ flag) {
  __shared__ uint32_t pre[SC_PACK_MAX + 1][NL];
  if (threadIdx.x != 0 || n == 0 || n > (uint32_t)SC_PACK_MAX) return;
  Fr acc = fe_one<FrP>();
  for (uint32_t i = 0; i < n; i++) {
    for (int k = 0; k < NL; k++) pre[i][k] = acc.v[k];
    acc = fe_mul(acc, fe_load<FrP>(coeffs_mont + 8 * i));
  }
  if (fe_is_zero(acc)) { *flag = 1u; return; }
  Fr inv = fe_inv(acc);
  for (uint32_t i = n; i-- > 0;) {
    Fr p; for (int k = 0; k < NL; k++) p.v[k] = pre[i][k];
    fe_store_tab<FrP>(inv_out + 8 * i, fe_mul(inv, p));
    inv = fe_mul(inv, fe_load<FrP>(coeffs_mont + 8 * i));
  }
}
// the final claims of a COMB layer hold c_i A_i[0] for the "par" A tables: fin[i] <- fin[i] / c_i (canonical integers in and out)
__global__ void __launch_bounds__(64) k_pp_unscale(uint32_t* __restrict__ fin, const uint32_t* __restrict__ inv, uint32_t n) {
  const uint32_t i = threadIdx.x;
  if (i >= n) return;
  const Fr x = fe_to_mont(fe_load<FrP>(fin + 8 * i));
  fe_store_packed<FrP>(fin + 8 * i, fe_from_mont(fe_mul(x, fe_load<FrP>(inv + 8 * i))));
}

// blocks per dot-product circuit of k_pp_dotp over tables of `len` entries; the partial sums need SC_PACK_MAX * pp_dotp_grid(len) * 32 bytes of c->sc_partial
static inline size_t pp_dotp_grid(size_t len) { return std::min<size_t>(std::max<size_t>(1, (len + 255) / 256), 1024); }

#include "transcript_plan.hpp"      // transcript_plan_boundary: the records k_tr_layer_step executes, one boundary's transcript work

// the job itself; the caller holds the mutex and has checked the arguments.  dotp_partials_present: the caller has just run k_pp_dotp over these
// dot-product circuits with this job's grid (dotp_grid) into c->sc_partial and nothing has written there since: the pass is not repeated.  force_plain: every layer in PLAIN mode (the rerun behind a zero
// coefficient).  *zero_coeff: a COMB layer met c_i = 0 — the outputs are not valid and nothing was written to them or to the transcript.
static int product_proof_run(sbn_ctx* c, const sbn_table* const* layers, size_t n_circ, size_t n_layers,
                             const sbn_table* const* dotp_left, const sbn_table* const* dotp_right, const sbn_table* const* dotp_weight, size_t n_dotp,
                             sbn_transcript* tr, uint8_t* out_polys, uint8_t* out_claims, uint8_t* out_rand, uint8_t* out_claims_final, bool force_plain, bool* zero_coeff,
                             bool dotp_partials_present = false) {
  *zero_coeff = false;
  using namespace sbn_host::fr;
  int rc;
  if ((rc = sc_tickets(c))) return rc;
  // ---- the transcript's plan.  Step s (s = 0 .. n_layers) closes layer n_layers - s (s > 0) and opens layer n_layers - 1 - s (s < n_layers);
  // a step starts behind a PRF (pos 64) except the first, which starts at the caller's phase.  Four distinct plans at most.
  const size_t L = n_layers;
  auto n_open_of = [&](size_t s) { return s == L ? (size_t)0 : n_circ + (s == L - 1 ? n_dotp : 0); };
  std::vector<uint8_t> masks_round; uint8_t prf_end[3], end[3], end2[3];
  std::vector<std::vector<uint8_t>> plan(L + 1);
  std::vector<size_t> plan_of(L + 1);                   // step -> the step whose plan it shares
  if ((rc = transcript_plan_boundary(tr->t.s.pos, tr->t.s.pos_begin, tr->t.s.cur_flags, 0, 0, n_open_of(0), plan[0], prf_end))) return fail(c, SBN_EINVAL, "product proof: internal: unexpected transcript plan (first step)");
  plan_of[0] = 0;
  transcript_plan_round(prf_end[0], prf_end[1], prf_end[2], masks_round, end);
  if (masks_round.size() != 400 || memcmp(end, prf_end, 3)) return fail(c, SBN_EINVAL, "product proof: internal: unexpected transcript plan (%zu round blocks)", masks_round.size() / 200);
  for (size_t s = 1; s <= L; s++) {
    const size_t same = (s >= 2 && n_open_of(s) == n_open_of(s - 1) && s != L) ? plan_of[s - 1] : s;
    plan_of[s] = same;
    if (same != s) continue;
    if ((rc = transcript_plan_boundary(prf_end[0], prf_end[1], prf_end[2], n_circ, s == L ? n_dotp : 0, n_open_of(s), plan[s], end2)) || memcmp(end2, prf_end, 3))
      return fail(c, SBN_EINVAL, "product proof: internal: unexpected transcript plan (step %zu)", s);
  }
  // ---- the layers' sumcheck states, planned before anything is uploaded: tables, bind buffers, mode, and (COMB) the groups of every launch
  const size_t ntab_max = 2 * n_circ + 1 + 3 * n_dotp;
  size_t rounds_total = 0; for (size_t s = 0; s < L; s++) rounds_total += s;
  auto al = [](size_t x) { return (x + 255) / 256 * 256; };
  const size_t len_max = (size_t)1 << (L - 1);          // the longest sumcheck table (layer 0's halves)
  const size_t half_max = std::max<size_t>(len_max / 2, 1), quarter_max = std::max<size_t>(len_max / 4, 1);
  const size_t slab_bytes_want = len_max * 32 + ntab_max * (half_max + quarter_max) * 32 + 4096;
  void* slab = nullptr; size_t slab_bytes = 0;
  { hipError_t e = pool_get(c, slab_bytes_want, &slab, &slab_bytes); if (e != hipSuccess) return fail(c, SBN_ENOMEM, "hipMalloc product proof state (%zu bytes): %s", slab_bytes_want, hipGetErrorString(e)); }
  struct SlabGuard { sbn_ctx* c; void* p; size_t n; ~SlabGuard() { pool_put(c, p, n); } } slab_guard{c, slab, slab_bytes};      // recycled in stream order (see sbn_table_free)
  uint32_t* d_eq = (uint32_t*)slab;                     // one slab: the eq table, then per table of the largest sumcheck len/2 + len/4 entries
  uint8_t* d_bufs = (uint8_t*)slab + len_max * 32;
  auto left_of = [&](size_t i, size_t layer) { return (const uint32_t*)layers[i * L + layer]->d; };
  auto right_of = [&](size_t i, size_t layer) { return (const uint32_t*)layers[i * L + layer]->d + 8 * (layers[i * L + layer]->len / 2); };
  struct LayerPlan { std::unique_ptr<sbn_sumcheck> st; std::vector<ScCombGroup> hg; size_t per_eval = 0, per_first = 0, o_groups = 0; };
  std::vector<LayerPlan> lp(L);
  size_t groups_total = 0; bool any_comb = false;
  for (size_t s = 1; s < L; s++) {
    const size_t layer = L - 1 - s, len = (size_t)1 << s, n_seq = layer == 0 ? n_dotp : 0;
    lp[s].st.reset(new sbn_sumcheck());
    sbn_sumcheck& st = *lp[s].st;
    st.n_par = n_circ; st.n_seq = n_seq; st.ntab = 2 * n_circ + 1 + 3 * n_seq; st.len = st.len0 = len;
    for (size_t i = 0; i < n_circ; i++) st.cur.push_back(left_of(i, layer));
    for (size_t i = 0; i < n_circ; i++) st.cur.push_back(right_of(i, layer));
    st.cur.push_back(d_eq);
    for (size_t k = 0; k < n_seq; k++) st.cur.push_back((const uint32_t*)dotp_left[k]->d);
    for (size_t k = 0; k < n_seq; k++) st.cur.push_back((const uint32_t*)dotp_right[k]->d);
    for (size_t k = 0; k < n_seq; k++) st.cur.push_back((const uint32_t*)dotp_weight[k]->d);
    {
      const size_t half = len / 2, quarter = std::max<size_t>(len / 4, 1);
      uint8_t* p = d_bufs;
      for (size_t t = 0; t < st.ntab; t++) { st.buf[0].push_back((uint32_t*)p); p += std::max<size_t>(half, 1) * 32; st.buf[1].push_back((uint32_t*)p); p += quarter * 32; }
    }
    // the mode sbn_sumcheck_begin would choose, except that SCALED layers (too short to hide the inversion) run PLAIN
    st.mode = (!force_plain && len >= SC_COMB_MIN_LEN && len / 4 >= sc_comb_min_q() && n_circ >= PP_COMB_MIN_CIRC && (n_circ + SC_COMB_MAX - 1) / SC_COMB_MAX <= SC_PACK_MAX - n_seq) ? 2 : 0;
    if (st.mode != 2) continue;
    any_comb = true;
    // the groups of the round-0 sums and of every combined bind (what sumcheck_begin_locked uploads), u left zero: k_pp_fill_u copies c_i in
    size_t ng = st.eval_groups = sc_comb_group_count(c, &st, len / 2, SC_PACK_MAX - n_seq, &lp[s].per_eval);
    std::vector<size_t> plan_q;
    for (size_t q = len / 4; q >= sc_comb_min_q() && q >= 1; q /= 2) { plan_q.push_back(q); st.grp_off.push_back(ng); st.grp_cnt.push_back(sc_comb_group_count(c, &st, q, SC_PACK_MAX - n_seq, nullptr)); ng += st.grp_cnt.back(); }
    lp[s].hg.resize(ng);
    const std::vector<sbn_host::fr::El> u0(n_circ, sbn_host::fr::El{{0, 0, 0, 0}});
    size_t per = lp[s].per_eval;
    sc_comb_groups_fill(&st, lp[s].hg.data(), st.eval_groups, per, st.cur.data(), nullptr, st.cur[2 * n_circ], true, u0.data(), nullptr);
    sc_comb_group_count(c, &st, plan_q[0], SC_PACK_MAX - n_seq, &lp[s].per_first);
    sc_comb_groups_fill(&st, lp[s].hg.data() + st.grp_off[0], st.grp_cnt[0], lp[s].per_first, st.cur.data(), st.buf[0].data(), st.buf[0][2 * n_circ], true, u0.data(), nullptr);
    for (size_t j = 1; j < plan_q.size(); j++) {
      sc_comb_group_count(c, &st, plan_q[j], SC_PACK_MAX - n_seq, &per);
      sc_comb_groups_fill(&st, lp[s].hg.data() + st.grp_off[j], st.grp_cnt[j], per, (const uint32_t* const*)st.buf[(j - 1) & 1].data(), st.buf[j & 1].data(), st.buf[j & 1][2 * n_circ], false, nullptr, nullptr,
                          st.buf[(j - 1) & 1][2 * n_circ]);
    }
    lp[s].o_groups = groups_total; groups_total += ng;
  }
  // ---- buffers, all before the first launch
  std::vector<size_t> o_plan(L + 1, 0);
  size_t off = 0;
  const size_t o_strobe = off; off += 256;
  const size_t o_mround = off; off += 512;
  for (size_t s = 0; s <= L; s++) if (plan_of[s] == s) { o_plan[s] = off; off += al(plan[s].size()); }
  const size_t o_zflag = off; off += 256;               // (uploaded as zero) a COMB layer met c_i = 0
  const size_t o_groups = off; off += al(groups_total * sizeof(ScCombGroup));
  const size_t up_bytes = off;                          // [0, up_bytes): uploaded
  const size_t o_polys = off; off += al(std::max<size_t>(rounds_total, 1) * 128);
  const size_t o_r = off; off += al(L * L * 32);       // one row per layer, the top layer first: r_layer, then the r_j of its sumcheck (= the `rand` of the layer below)
  const size_t o_fin = off; off += L * (size_t)SC_FINAL_MAX * 32;
  const size_t o_cfinal = off; off += al((size_t)SC_PACK_MAX * 32);
  const size_t down_end = off;                          // [o_strobe, + 256), the flag and [o_polys, down_end): downloaded
  const size_t o_claims = off; off += al((size_t)SC_PACK_MAX * 32);
  const size_t o_w = off; off += al((size_t)SC_PACK_MAX * 32);
  const size_t o_wc = off; off += al((size_t)SC_PACK_MAX * 32);
  const size_t o_wi = off; off += al((size_t)SC_PACK_MAX * 32);
  const size_t o_cm = off; off += al((size_t)SC_PACK_MAX * 32);
  const size_t o_inv = off; off += al((size_t)SC_PACK_MAX * 32);
  const size_t o_claim = off; off += 256;
  const size_t o_rm = off; off += 256;
  const size_t o_flag = off; off += 256;
  const size_t o_tfin = off; off += al((size_t)SC_FINAL_MAX * 32);       // the sumcheck state's d_finals (table format)
  const size_t o_mbox = off; off += al((size_t)SC_MBOX_WORDS * 4);
  const size_t total = off;
  const size_t gx_dot = pp_dotp_grid(len_max);
  if ((rc = ensure(c, c->sc_prove, total))) return rc;
  if ((rc = ensure_pin(c, 4096 + total))) return rc;
  if ((rc = ensure(c, c->sc_partial, std::max(SC_PARTIAL_BYTES, (size_t)SC_PACK_MAX * gx_dot * 32)))) return rc;
  if ((rc = ensure(c, c->stage_scal, std::max<size_t>(len_max * 32, 64)))) return rc;     // the eq build's ping-pong partner
  if (any_comb && !c->pp_stream) HIPCHK(c, hipStreamCreateWithFlags(&c->pp_stream, hipStreamNonBlocking));
  std::vector<hipEvent_t> events;                       // two per COMB layer, back to the context's pool when the job is over
  struct EventGuard { sbn_ctx* c; std::vector<hipEvent_t>* v; ~EventGuard() { for (hipEvent_t e : *v) c->evt_pool.push_back(e); } } event_guard{c, &events};
  uint8_t* d = (uint8_t*)c->sc_prove.p; uint8_t* h = (uint8_t*)c->pin + 4096;
  memset(h, 0, up_bytes);
  memcpy(h + o_strobe, tr->t.s.st, 200);
  memcpy(h + o_mround, masks_round.data(), 400);
  for (size_t s = 0; s <= L; s++) if (plan_of[s] == s) memcpy(h + o_plan[s], plan[s].data(), plan[s].size());
  for (size_t s = 1; s < L; s++) if (lp[s].st && lp[s].st->mode == 2) {
    memcpy(h + o_groups + lp[s].o_groups * sizeof(ScCombGroup), lp[s].hg.data(), lp[s].hg.size() * sizeof(ScCombGroup));
    lp[s].st->d_groups = (ScCombGroup*)(d + o_groups) + lp[s].o_groups;
  }
  HIPCHK(c, hipMemcpyAsync(d, h, up_bytes, hipMemcpyHostToDevice, c->stream));
  uint32_t* d_claims = (uint32_t*)(d + o_claims); uint32_t* dmbox = (uint32_t*)(d + o_mbox);
  const ScScalarDev rs{(const uint32_t*)(d + o_rm)};
  auto d_r_row = [&](size_t layer) { return (uint32_t*)(d + o_r + (L - 1 - layer) * L * 32); };      // rows in proof order: the top layer first
  auto d_fin_row = [&](size_t layer) { return (uint32_t*)(d + o_fin + (L - 1 - layer) * (size_t)SC_FINAL_MAX * 32); };
  // ---- claims_to_verify: ProductCircuit::evaluate of every circuit, DotProductCircuit::evaluate behind them (:262-264, :296-299)
  {
    PpRead0Pack top; memset(&top, 0, sizeof top);
    for (size_t i = 0; i < n_circ; i++) top.p[i] = left_of(i, L - 1);
    if (n_dotp && !dotp_partials_present) {
      ScArgsPack pack; memset(&pack, 0, sizeof pack);
      for (size_t k = 0; k < n_dotp; k++) { pack.a[k].t[0] = (const uint32_t*)dotp_left[k]->d; pack.a[k].t[1] = (const uint32_t*)dotp_right[k]->d; pack.a[k].t[2] = (const uint32_t*)dotp_weight[k]->d; }
      LAUNCH(c, "k_pp_dotp", k_pp_dotp, dim3((unsigned)gx_dot, (unsigned)n_dotp), 256, pack, len_max, (uint32_t*)c->sc_partial.p);
    }
    LAUNCH(c, "k_pp_claims0", k_pp_claims0, (unsigned)(n_circ + n_dotp), 64, top, (uint32_t)n_circ, (const uint32_t*)c->sc_partial.p, (uint32_t)gx_dot, d_claims);
    LAUNCHCHK(c);
  }
  auto step = [&](size_t s) {                           // close layer L - s (s > 0), open layer L - 1 - s (s < L)
    TrLayerArgs a; memset(&a, 0, sizeof a);
    a.recs = d + o_plan[plan_of[s]]; a.nblk = (uint32_t)(plan[plan_of[s]].size() / TR_REC_BYTES); a.strobe = d + o_strobe;
    if (s > 0) {
      const size_t closed = L - s;
      a.data = d_fin_row(closed); a.ndata = (uint32_t)(2 * n_circ + 1 + (closed == 0 ? 3 * n_dotp : 0)); a.n_close = (uint32_t)n_circ;
      a.out_r = d_r_row(closed);
    }
    a.n_open = (uint32_t)n_open_of(s);
    a.claims = d_claims; a.out_claims = (uint32_t*)(d + o_cfinal); a.weights = (uint32_t*)(d + o_w); a.claim = (uint32_t*)(d + o_claim);
    if (s < L && lp[s].st && lp[s].st->mode == 2) { a.n_par_open = (uint32_t)n_circ; a.coeffs_mont = (uint32_t*)(d + o_cm); a.weights_comb = (uint32_t*)(d + o_wc); a.weights_inst = (uint32_t*)(d + o_wi); }
    LAUNCH(c, "k_tr_layer_step", k_tr_layer_step, 1, 64, a);
  };
  // ---- the layers, top first; nothing below waits for the host
  size_t poly_off = 0;
  for (size_t s = 0; s < L; s++) {
    const size_t layer = L - 1 - s, rounds = s, len = (size_t)1 << rounds;      // this layer's halves: `len` entries, `rounds` sumcheck rounds
    const size_t n_seq = layer == 0 ? n_dotp : 0, ninst = n_circ + n_seq;
    step(s);
    if (rounds == 0) {
      // the zero-round layer (:323-332 with num_rounds_prod = 0): the claims are the entries themselves, eq of the empty point is 1
      PpRead0Pack pk; memset(&pk, 0, sizeof pk);
      for (size_t i = 0; i < n_circ; i++) { pk.p[i] = left_of(i, layer); pk.p[n_circ + i] = right_of(i, layer); }
      const size_t o = 2 * n_circ + 1;
      for (size_t k = 0; k < n_seq; k++) { pk.p[o + k] = (const uint32_t*)dotp_left[k]->d; pk.p[o + n_seq + k] = (const uint32_t*)dotp_right[k]->d; pk.p[o + 2 * n_seq + k] = (const uint32_t*)dotp_weight[k]->d; }
      LAUNCH(c, "k_pp_read0", k_pp_read0, 1, 128, pk, (uint32_t)(o + 3 * n_seq), d_fin_row(layer));
      LAUNCHCHK(c);
      continue;
    }
    // poly_C_par = eq(rand), rand = r_layer ‖ rand_prod of the layer above (:271, :374-376): its row of challenges
    if ((rc = eq_evals_dev_enqueue(c, d_r_row(layer + 1), rounds, d_eq, (uint32_t*)c->stage_scal.p))) return rc;
    sbn_sumcheck& st = *lp[s].st;                        // planned above: PLAIN, or COMB with its groups already in device memory
    st.d_finals = (uint32_t*)(d + o_tfin);
    const bool comb_layer = st.mode == 2;
    hipEvent_t ev_inv = nullptr;
    if (comb_layer) {
      // the coefficients exist: 1 / c_i on the second stream, beside this layer's sumcheck; c_i into the groups that scale A
      hipEvent_t ev_open = evt_get(c); events.push_back(ev_open); ev_inv = evt_get(c); events.push_back(ev_inv);
      HIPCHK(c, hipEventRecord(ev_open, c->stream));
      HIPCHK(c, hipStreamWaitEvent(c->pp_stream, ev_open, 0));
      hipLaunchKernelGGL(k_pp_inv, dim3(1), dim3(64), 0, c->pp_stream, (const uint32_t*)(d + o_cm), (uint32_t)n_circ, (uint32_t*)(d + o_inv), (uint32_t*)(d + o_zflag));
      HIPCHK(c, hipEventRecord(ev_inv, c->pp_stream));
      LAUNCH(c, "k_pp_fill_u", k_pp_fill_u, (unsigned)st.eval_groups, 64, st.d_groups, (uint32_t)lp[s].per_eval, (const uint32_t*)(d + o_cm));
      LAUNCH(c, "k_pp_fill_u", k_pp_fill_u, (unsigned)st.grp_cnt[0], 64, st.d_groups + st.grp_off[0], (uint32_t)lp[s].per_first, (const uint32_t*)(d + o_cm));
    }
    std::vector<uint32_t> nslots(rounds, (uint32_t)ninst); std::vector<bool> comb_round(rounds, false);
    {                                                   // round 0's sums into the mailbox's device twin
      ScArgsPack pack; memset(&pack, 0, sizeof pack);
      const size_t o = 2 * n_circ + 1, half = len / 2;
      if (!comb_layer) {
        for (size_t i = 0; i < n_circ; i++) { pack.a[i].t[0] = st.cur[i]; pack.a[i].t[1] = st.cur[n_circ + i]; pack.a[i].t[2] = st.cur[2 * n_circ]; }
        for (size_t k = 0; k < n_seq; k++) { pack.a[n_circ + k].t[0] = st.cur[o + k]; pack.a[n_circ + k].t[1] = st.cur[o + n_seq + k]; pack.a[n_circ + k].t[2] = st.cur[o + 2 * n_seq + k]; }
        if ((rc = sc_launch_inst_eval(c, pack, ninst, half, ++c->mbox_seq, dmbox))) return rc;
      } else {
        // the "par" group on the combined kernel (A scaled in registers), the "seq" instances per instance: sumcheck_begin_locked's launches
        const size_t n_comb = st.eval_groups;
        for (size_t k = 0; k < n_seq; k++) { pack.a[k].t[0] = st.cur[o + k]; pack.a[k].t[1] = st.cur[o + n_seq + k]; pack.a[k].t[2] = st.cur[o + 2 * n_seq + k]; }
        const uint32_t seq = ++c->mbox_seq;
        uint32_t* part2 = (uint32_t*)c->sc_partial.p + (size_t)SC_PACK_MAX * 1024 * 24;
        if (n_seq && half >= ((size_t)1 << 16)) {
          const size_t mc = c->sck.comb_eval_blocks_mixed, ms = c->sck.eval_blocks_mixed, cap = (half + 255) / 256;
          const unsigned gxc = (unsigned)std::max<size_t>(1, std::min(std::min(cap, std::max<size_t>(1, mc / n_comb)), SC_PART_COMB_BLOCKS));
          const unsigned gxs = (unsigned)std::max<size_t>(1, std::min(std::min(cap, std::max<size_t>(1, ms / n_seq)), SC_PART_INST_BLOCKS));
          LAUNCH(c, "k_sc_eval_mixed", k_sc_eval_mixed, (unsigned)(n_comb * gxc + n_seq * gxs), 256, (const ScCombGroup*)st.d_groups, (uint32_t)n_comb, gxc, pack, (uint32_t)n_seq, gxs, half,
                 (uint32_t*)c->sc_partial.p, part2, (uint32_t*)c->sc_tickets.p, dmbox, seq);
        } else {
          if (n_seq) { if ((rc = sc_launch_inst_eval(c, pack, n_seq, half, seq, dmbox))) return rc; }
          const unsigned gx = (unsigned)std::max<size_t>(1, std::min(std::min<size_t>((half + 255) / 256, std::max<size_t>(1, c->sck.comb_eval_blocks / n_comb)), SC_PART_COMB_BLOCKS));
          LAUNCH(c, "k_sc_comb_eval", k_sc_comb_eval, dim3(gx, (unsigned)n_comb), 256, (const ScCombGroup*)st.d_groups, half, part2, (uint32_t*)c->sc_tickets.p, dmbox, (uint32_t)n_seq, seq);
        }
        LAUNCHCHK(c);
        nslots[0] = (uint32_t)(n_seq + n_comb); comb_round[0] = true;
        // which slots each later round fills (sc_round_slots: lengths only)
        size_t l2 = len, binds = 0; std::vector<size_t> ids; size_t nc; bool cb;
        for (size_t j = 1; j < rounds; j++, l2 /= 2, binds++) { sc_round_slots(c, &st, l2, binds, ids, nc, cb); nslots[j] = (uint32_t)(ids.size() + nc); comb_round[j] = cb; }
      }
    }
    for (size_t j = 0; j < rounds; j++) {
      TrStepArgs a;
      a.sums = dmbox; a.weights = (const uint32_t*)(d + (!comb_layer ? o_w : comb_round[j] ? o_wc : o_wi)); a.nslots = nslots[j];
      a.masks = d + o_mround; a.nblk = 2; a.pos0 = prf_end[0];
      a.strobe = d + o_strobe; a.claim = (uint32_t*)(d + o_claim); a.r_mont = (uint32_t*)(d + o_rm);
      a.out_poly = (uint32_t*)(d + o_polys + (poly_off + j) * 128); a.out_r = d_r_row(layer) + 8 * (1 + j);
      LAUNCH(c, "k_tr_sumcheck_step", k_tr_sumcheck_step, 1, 64, a);
      if (st.len >= 4) {
        const uint32_t seq = ++c->mbox_seq;
        ScRoundPlan rp;
        if ((rc = sc_round_enqueue(c, &st, rs, dmbox, seq, rp))) return rc;
        if (j + 1 < rounds && (rp.inst_ids.size() + rp.n_comb != nslots[j + 1] || rp.comb != comb_round[j + 1]))
          return fail(c, SBN_EINVAL, "product proof: internal: round %zu of layer %zu filled %zu slots, %u were planned", j, layer, rp.inst_ids.size() + rp.n_comb, nslots[j + 1]);
        sc_round_advance(&st, rp);
      } else {
        const uint32_t fseq = ++c->mbox_seq;
        if ((rc = sc_final_enqueue(c, &st, rs, d_fin_row(layer), (uint32_t*)(d + o_flag), fseq))) return rc;
        sc_final_advance(&st);
      }
    }
    if (comb_layer) {                                   // the claims the close step appends: A_i[0] = A'_i[0] / c_i
      if (!st.scaled) return fail(c, SBN_EINVAL, "product proof: internal: a COMB layer ended unscaled");
      HIPCHK(c, hipStreamWaitEvent(c->stream, ev_inv, 0));
      LAUNCH(c, "k_pp_unscale", k_pp_unscale, 1, 64, d_fin_row(layer), (const uint32_t*)(d + o_inv), (uint32_t)n_circ);
    }
    poly_off += rounds;
  }
  step(L);
  LAUNCHCHK(c);
  // one copy back (ranges of one buffer), one wait
  HIPCHK(c, hipMemcpyAsync(h + o_strobe, d + o_strobe, 256, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipMemcpyAsync(h + o_zflag, d + o_zflag, 4, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipMemcpyAsync(h + o_polys, d + o_polys, down_end - o_polys, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  if (c->prof) prof_drain(c);
  { uint32_t z; memcpy(&z, h + o_zflag, 4); if (z) { *zero_coeff = true; return SBN_OK; } }      // (reviewed, not tested: see the head of this file)
  memcpy(out_polys, h + o_polys, rounds_total * 128);
  {
    uint8_t* oc = out_claims;
    for (size_t s = 0; s < L; s++) { memcpy(oc, h + o_fin + s * (size_t)SC_FINAL_MAX * 32, 2 * n_circ * 32); oc += 2 * n_circ * 32; }
    memcpy(oc, h + o_fin + (L - 1) * (size_t)SC_FINAL_MAX * 32 + (2 * n_circ + 1) * 32, 3 * n_dotp * 32);
  }
  memcpy(out_rand, h + o_r + (L - 1) * L * 32, L * 32);
  memcpy(out_claims_final, h + o_cfinal, n_circ * 32);
  memcpy(tr->t.s.st, h + o_strobe, 200); tr->t.s.pos = prf_end[0]; tr->t.s.pos_begin = prf_end[1]; tr->t.s.cur_flags = prf_end[2];
  return SBN_OK;
}

// the job, and the rerun behind a zero coefficient; the caller holds the mutex and has checked the arguments
static int product_proof_locked(sbn_ctx* c, const sbn_table* const* layers, size_t n_circ, size_t n_layers,
                                const sbn_table* const* dotp_left, const sbn_table* const* dotp_right, const sbn_table* const* dotp_weight, size_t n_dotp,
                                sbn_transcript* tr, uint8_t* out_polys, uint8_t* out_claims, uint8_t* out_rand, uint8_t* out_claims_final,
                                bool dotp_partials_present = false) {
  bool zero_coeff = false;
  int rc = product_proof_run(c, layers, n_circ, n_layers, dotp_left, dotp_right, dotp_weight, n_dotp, tr, out_polys, out_claims, out_rand, out_claims_final, false, &zero_coeff,
                             dotp_partials_present);
  // a coefficient was zero in a layer that divides by it: the same job with every layer in PLAIN mode (reviewed, not tested: 2^-254); the first
  // run's sumchecks have used c->sc_partial, so the dot-product pass runs again
  if (rc == SBN_OK && zero_coeff) rc = product_proof_run(c, layers, n_circ, n_layers, dotp_left, dotp_right, dotp_weight, n_dotp, tr, out_polys, out_claims, out_rand, out_claims_final, true, &zero_coeff);
  if (rc == SBN_OK && zero_coeff) return fail(c, SBN_EHIP, "product proof: internal: zero-coefficient flag raised in PLAIN mode");
  return rc;
}

extern "C" {

int sbn_product_proof_prove(sbn_ctx* c, const sbn_table* const* layers, size_t n_circ, size_t n_layers,
                            const sbn_table* const* dotp_left, const sbn_table* const* dotp_right, const sbn_table* const* dotp_weight, size_t n_dotp,
                            sbn_transcript* tr, uint8_t* out_polys, uint8_t* out_claims, uint8_t* out_rand, uint8_t* out_claims_final) {
  if (!c || !layers || !tr || !out_polys || !out_claims || !out_rand || !out_claims_final || n_circ == 0 || n_layers == 0 || n_layers > (size_t)EQ_MAX_VARS) return SBN_EINVAL;
  if (n_dotp && (!dotp_left || !dotp_right || !dotp_weight)) return SBN_EINVAL;
  std::lock_guard<std::mutex> g(c->mu); hipSetDevice(c->device);
  if (n_circ + n_dotp > (size_t)SC_PACK_MAX) return fail(c, SBN_EINVAL, "product proof: %zu instances (at most %d)", n_circ + n_dotp, SC_PACK_MAX);
  for (size_t i = 0; i < n_circ; i++)
    for (size_t j = 0; j < n_layers; j++) {
      const sbn_table* t = layers[i * n_layers + j];
      if (!t) return SBN_EINVAL;
      if (t->len != ((size_t)1 << (n_layers - j))) return fail(c, SBN_EINVAL, "product proof: layer %zu of circuit %zu has %zu entries, 2^%zu are expected  [product_tree.rs:272 assert_eq]", j, i, t->len, n_layers - j);
    }
  for (size_t k = 0; k < n_dotp; k++) {
    if (!dotp_left[k] || !dotp_right[k] || !dotp_weight[k]) return SBN_EINVAL;
    const size_t want = (size_t)1 << (n_layers - 1);
    if (dotp_left[k]->len != want || dotp_right[k]->len != want || dotp_weight[k]->len != want) return fail(c, SBN_EINVAL, "product proof: dot-product circuit %zu does not have 2^%zu entries  [product_tree.rs:299-301 assert_eq]", k, n_layers - 1);
  }
  return product_proof_locked(c, layers, n_circ, n_layers, dotp_left, dotp_right, dotp_weight, n_dotp, tr, out_polys, out_claims, out_rand, out_claims_final);
}

}  // extern "C"
