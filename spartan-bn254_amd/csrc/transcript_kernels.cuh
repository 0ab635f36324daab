// transcript_kernels.cuh — the Merlin / STROBE-128 transcript step of a sumcheck round on the device (sbn_sumcheck_prove).
//
// One wavefront does, between two round kernels, what the host does between two sbn_sumcheck_round calls: combine the round's
// sums (sumcheck.rs:269-271), UniPoly::from_evals (unipoly.rs:28-59), append the polynomial (unipoly.rs:117-122), draw
// challenge_scalar("challenge_nextround") (transcript.rs:56-67), e = poly(r_j) (sumcheck.rs:301).  It is latency, not throughput:
//   * Keccak-f[1600] runs with ONE 64-bit state lane per SIMD lane (25 of 64 active): theta's column parities, pi and chi's row
//     neighbours are wave shuffles (ds_bpermute through __shfl, nine 64-bit exchanges per round in three dependent steps), rho a per-lane rotate count.
//   * STROBE's bookkeeping (operation headers, lengths, labels, the run_f padding bytes, where the blocks end) depends on the
//     phase `pos` alone, never on a value, so the host plans it with its own Strobe code (transcript_plan.hpp over host_strobe.hpp's StrobePlan) as
//     one 200-byte XOR mask per block; the step XORs mask and coefficient bytes into the state, eight bytes per lane, at
//     whatever phase the round starts.  A round is two blocks (three when the first round starts at pos >= 78).
//   * field work is laid out so that independent products share one instruction stream: different lanes, same fe_mul.
// The state between steps is the 200 sponge bytes in device memory; pos / pos_begin / cur_flags are the plan's.
#pragma once
#include "fp.cuh"
#include "sumcheck_kernels.cuh"
#include "transcript_plan.hpp"      // TR_RATE, TR_COEFF_*, TR_REC_*: the layout the host plans and the steps execute

namespace sbn {

struct TrConst { uint32_t rho[25]; uint32_t rc[24][2]; };
__host__ __device__ constexpr TrConst tr_make_const() {
  TrConst t{};
  int x = 1, y = 0;
  for (int k = 0; k < 24; k++) { t.rho[x + 5 * y] = (uint32_t)(((k + 1) * (k + 2) / 2) % 64); const int nx = y, ny = (2 * x + 3 * y) % 5; x = nx; y = ny; }
  uint32_t lfsr = 1;
  for (int r = 0; r < 24; r++) {
    uint64_t c = 0;
    for (int j = 0; j < 7; j++) { if (lfsr & 1) c |= (uint64_t)1 << ((1 << j) - 1); lfsr = ((lfsr << 1) ^ ((lfsr & 0x80) ? 0x71 : 0)) & 0xff; }
    t.rc[r][0] = (uint32_t)c; t.rc[r][1] = (uint32_t)(c >> 32);
  }
  return t;
}
__device__ const TrConst TR_CONST = tr_make_const();

__device__ __forceinline__ uint64_t tr_shfl64(uint64_t v, int src) {
  const uint32_t lo = (uint32_t)__shfl((int)(uint32_t)v, src, 64), hi = (uint32_t)__shfl((int)(uint32_t)(v >> 32), src, 64);
  return ((uint64_t)hi << 32) | lo;
}
__device__ __forceinline__ uint64_t tr_rol64(uint64_t x, uint32_t n) { return (x << n) | (x >> ((64u - n) & 63u)); }   // n in [0, 64)

// per-lane indices of the permutation (lane i = state lane x + 5 y; lanes >= 25 mirror lane 0 and are ignored)
struct TrLanes { int th1, th2, th3, th4, src, dm, dp, c1, c2; uint32_t rot; uint32_t rc_lo, rc_hi; };
__device__ __forceinline__ TrLanes tr_lanes(int lane) {
  const int i = lane < 25 ? lane : 0, x = i % 5, y = i / 5;
  TrLanes L;
  L.th1 = (i + 5) % 25; L.th2 = (i + 10) % 25; L.th3 = (i + 15) % 25; L.th4 = (i + 20) % 25;
  L.src = (x + 3 * y) % 5 + 5 * x;                 // pi: (x', y') -> (y', 2 x' + 3 y'), read backwards
  L.dm = (L.src % 5 + 4) % 5; L.dp = (L.src % 5 + 1) % 5;     // theta's two columns for the SOURCE lane (row 0 holds every column's parity)
  L.rot = TR_CONST.rho[L.src];
  L.c1 = 5 * y + (x + 1) % 5; L.c2 = 5 * y + (x + 2) % 5;
  L.rc_lo = lane < 24 ? TR_CONST.rc[lane][0] : 0u; L.rc_hi = lane < 24 ? TR_CONST.rc[lane][1] : 0u;   // lane r keeps round r's constant
  return L;
}
// Keccak-f[1600], `a` = this lane's 64-bit state lane.  Three dependent exchanges per round: (column parities, and the lane pi will
// move here, fetched before theta); (theta's two parities for that source lane: theta is applied on arrival, fused with rho); (chi's neighbours).
__device__ __forceinline__ uint64_t tr_keccak_f(uint64_t a, const TrLanes& L, int lane) {
#pragma unroll 1
  for (int r = 0; r < 24; r++) {
    const uint64_t as = tr_shfl64(a, L.src);
    const uint64_t c = a ^ tr_shfl64(a, L.th1) ^ tr_shfl64(a, L.th2) ^ tr_shfl64(a, L.th3) ^ tr_shfl64(a, L.th4);    // parity of this lane's column
    const uint64_t b = tr_rol64(as ^ tr_shfl64(c, L.dm) ^ tr_rol64(tr_shfl64(c, L.dp), 1), L.rot);
    a = b ^ (~tr_shfl64(b, L.c1) & tr_shfl64(b, L.c2));
    const uint32_t klo = (uint32_t)__builtin_amdgcn_readlane((int)L.rc_lo, r), khi = (uint32_t)__builtin_amdgcn_readlane((int)L.rc_hi, r);
    if (lane == 0) a ^= ((uint64_t)khi << 32) | klo;
  }
  return a;
}

// constants in fp.cuh's Montgomery domain (R = 2^261), 29-bit limbs
struct TrFrC {
  static constexpr uint32_t K778[9] = {0x1c00feeeu, 0x1c5573e0u, 0x18197feau, 0x08b5c34cu, 0x120f41aeu, 0x1a97f167u, 0x15f6b4bbu, 0x01454f10u, 0x00160937u};   // 2^256 R^2 = 2^778 mod r
  static constexpr uint32_t INV2[9] = {0x1fffffacu, 0x0edb5ba9u, 0x09c4156eu, 0x0f90701eu, 0x1016ecefu, 0x100ec0c7u, 0x093e16a4u, 0x09c376eeu, 0x001f1642u};   // R / 2
  static constexpr uint32_t INV6[9] = {0x1555553au, 0x0efe3c4du, 0x177eca05u, 0x15108601u, 0x090b85fcu, 0x1c971618u, 0x0383f30cu, 0x177e9672u, 0x002a9f9fu};   // R / 6
};
__device__ __forceinline__ Fr tr_fr_k778() { Fr r; for (int i = 0; i < NL; i++) r.v[i] = SBN_C9(TrFrC::K778, i); return r; }
__device__ __forceinline__ Fr tr_fr_inv2() { Fr r; for (int i = 0; i < NL; i++) r.v[i] = SBN_C9(TrFrC::INV2, i); return r; }
__device__ __forceinline__ Fr tr_fr_inv6() { Fr r; for (int i = 0; i < NL; i++) r.v[i] = SBN_C9(TrFrC::INV6, i); return r; }
__device__ __forceinline__ Fr tr_shfl(const Fr& a, int src) { Fr r;
#pragma unroll
  for (int i = 0; i < NL; i++) r.v[i] = (uint32_t)__shfl((int)a.v[i], src, 64);
  return r; }

struct TrStepArgs {
  const uint32_t* sums;       // the round kernel's results: nslots x 3 canonical integers (device copy of the mailbox layout)
  const uint32_t* weights;    // nslots x 8 words: c_i R^2 for a slot the combination weights, R^2 otherwise (canonical)
  uint32_t nslots;            // <= SC_PACK_MAX
  const uint8_t* masks;       // nblk x 200 bytes: the host's plan of this round's STROBE blocks
  uint32_t nblk, pos0;        // blocks of this round (each ends in a permutation); pos when the round starts
  uint8_t* strobe;            // 200 bytes, 8-byte aligned: the sponge state, read and written
  uint32_t* claim;            // e as its nine 29-bit limbs (Montgomery domain, lazy: no canonical form is needed between steps), read and written
  uint32_t* r_mont;           // out: r_j for the launches behind this one (canonical Montgomery words)
  uint32_t* out_poly;         // out: c0..c3 of this round, canonical integers
  uint32_t* out_r;            // out: r_j, canonical integer
};

__global__ void __launch_bounds__(64) k_tr_sumcheck_step(TrStepArgs A) {
  __shared__ uint32_t s_prod[3][SC_PACK_MAX][NL];
  __shared__ uint32_t s_e[3][NL];
  __shared__ __attribute__((aligned(16))) uint8_t s_cb[128];      // the four coefficients as the transcript reads them
  __shared__ __attribute__((aligned(16))) uint32_t s_ch[16];      // the 64 challenge bytes
  const int lane = threadIdx.x;
  const TrLanes L = tr_lanes(lane);
  // everything the step reads from memory is requested here, ahead of the first use: each dependent global load is a microsecond
  uint64_t a = lane < 25 ? reinterpret_cast<const uint64_t*>(A.strobe)[lane] : 0;
  uint64_t mk[3];
#pragma unroll
  for (int b = 0; b < 3; b++) mk[b] = (lane < 25 && b < (int)A.nblk) ? reinterpret_cast<const uint64_t*>(A.masks + 200 * b)[lane] : 0;
  Fr e;
#pragma unroll
  for (int k = 0; k < NL; k++) e.v[k] = A.claim[k];

  // 1. the combination: slot s, value t in lane 21 t + s (slots 21 .. 23 in a second pass), weights bring the sums into Montgomery form
  {
    const int t = lane / 21, s0 = lane % 21;
    for (int s = s0; t < 3 && s < (int)A.nslots; s += 21) {
      const Fr x = fe_load<FrP>(A.sums + 8 * (3 * s + t)), w = fe_load<FrP>(A.weights + 8 * s);
      const Fr p = fe_mul(x, w);                                                         // (-r, 2r)
#pragma unroll
      for (int k = 0; k < NL; k++) s_prod[t][s][k] = p.v[k];
    }
  }
  __syncthreads();
  Fr acc = fe_zero<FrP>();
  if (lane < 3) {
    for (uint32_t s = 0; s < A.nslots; s++) { Fr x; for (int k = 0; k < NL; k++) x.v[k] = s_prod[lane][s][k]; acc = fe_add(acc, x); }      // within (-24 r, 48 r)
  }
  acc = fe_reduce(acc);                                                                  // lanes 0..2: e0, e2, e3 in (-r, 2r)
  if (lane < 3) for (int k = 0; k < NL; k++) s_e[lane][k] = acc.v[k];
  __syncthreads();
  Fr e0, e2, e3;
  for (int k = 0; k < NL; k++) { e0.v[k] = s_e[0][k]; e2.v[k] = s_e[1][k]; e3.v[k] = s_e[2][k]; }
  const Fr e1 = fe_sub(e, e0);                                                           // sumcheck.rs:274; e within (-3 r, 6 r)
  // 2. UniPoly::from_evals: lane 0: a = (e3 - 3 e2 + 3 e1 - e0) / 6, lane 1: b = (2 e0 - 5 e1 + 4 e2 - e3) / 2 — one product for both
  Fr xa = fe_sub(e3, e0), d21 = fe_sub(e1, e2);
  xa = fe_add(xa, fe_add(fe_dbl(d21), d21));                                             // |.| < 20 r
  Fr xb = fe_sub(fe_dbl(fe_sub(e0, e1)), e3);                                            // 2 e0 - 2 e1 - e3
  xb = fe_add(xb, fe_add(fe_dbl(fe_dbl(fe_sub(e2, e1))), e1));                           // + 4 e2 - 4 e1 + e1;  |.| < 30 r
  const Fr ab = fe_mul(fe_sel2(lane == 1, xa, xb), fe_sel2(lane == 1, tr_fr_inv6(), tr_fr_inv2()));
  const Fr ca = tr_shfl(ab, 0), cb = tr_shfl(ab, 1);
  const Fr cc = fe_sub(fe_sub(e1, e0), fe_add(ca, cb));                                  // c = e1 - d - a - b
  // lane k: coefficient k (d, c, b, a), canonical for the transcript and the proof
  const Fr mine = fe_sel4(lane & 3, e0, cc, cb, ca);
  const Fr plain = fe_from_mont(mine);
  if (lane < 4) {
    uint32_t w[8]; fe_pack<FrP>(plain, w);
    uint4* o = reinterpret_cast<uint4*>(A.out_poly + 8 * lane);
    o[0] = make_uint4(w[0], w[1], w[2], w[3]); o[1] = make_uint4(w[4], w[5], w[6], w[7]);
    uint4* sc = reinterpret_cast<uint4*>(s_cb + 32 * lane);
    sc[0] = make_uint4(w[0], w[1], w[2], w[3]); sc[1] = make_uint4(w[4], w[5], w[6], w[7]);
  }
  __syncthreads();

  // 3. the transcript: every block = mask (labels, lengths, operation headers, run_f's padding) ^ coefficient bytes, then Keccak-f
#pragma unroll
  for (int b = 0; b < 3; b++) {
    if (b >= (int)A.nblk) break;
    uint64_t m = mk[b];
#pragma unroll
    for (int q = 0; q < 8; q++) {
      const int p = 8 * lane + q;                                      // position in the block
      const int t = (int)(TR_RATE * b) + p - (int)A.pos0 - TR_COEFF_FIRST;      // offset from the first coefficient byte in the round's stream
      const int k = t / TR_COEFF_STRIDE, o = t - k * TR_COEFF_STRIDE;
      if (p < TR_RATE && t >= 0 && k < 4 && o < 32) m ^= (uint64_t)s_cb[32 * k + o] << (8 * q);
    }
    a = tr_keccak_f(a ^ m, L, lane);
  }
  // the PRF's 64 bytes: positions 0 .. 63 of the fresh block, read and cleared
  if (lane < 8) { s_ch[2 * lane] = (uint32_t)a; s_ch[2 * lane + 1] = (uint32_t)(a >> 32); a = 0; }
  if (lane < 25) reinterpret_cast<uint64_t*>(A.strobe)[lane] = a;
  __syncthreads();

  // 4. challenge_scalar: lo + hi 2^256 mod r, straight into Montgomery form: lane 0: lo R^2 / R, lane 1: hi (2^256 R^2) / R
  uint32_t w[8];
#pragma unroll
  for (int k = 0; k < 8; k++) w[k] = s_ch[8 * (lane & 1) + k];
  const Fr half = fe_mul(fe_unpack<FrP>(w), fe_sel2((lane & 1) != 0, fe_const_r2<FrP>(), tr_fr_k778()));        // inputs < 2^256 = 5.3 r
  const Fr r = fe_add(tr_shfl(half, 0), tr_shfl(half, 1));                               // (-2 r, 4 r), every lane
  // 5. one product in five lanes: r^2, c r, a r (for e = d + c r + r^2 (b + a r)), r canonical in both domains
  const Fr op = fe_sel4(lane & 3, r, cc, ca, fe_small<FrP>(1u));
  const Fr p1 = fe_mul(r, fe_sel2(lane == 4, op, fe_one<FrP>()));
  const Fr canon = fe_canon_small(p1);                                                   // lane 3: r as an integer, lane 4: r R
  if (lane == 3) fe_store_packed<FrP>(A.out_r, canon);
  if (lane == 4) fe_store_packed<FrP>(A.r_mont, canon);
  const Fr r2 = tr_shfl(p1, 0), cr = tr_shfl(p1, 1), ar = tr_shfl(p1, 2);
  const Fr hi = fe_mul(r2, fe_add(cb, ar));
  const Fr en = fe_add(fe_add(e0, cr), hi);                                              // (-3 r, 6 r), normalised
  if (lane == 0) for (int k = 0; k < NL; k++) A.claim[k] = en.v[k];
}

// ---- the layer-boundary step of ProductCircuitEvalProofBatched::prove (product_tree.rs:316-376), sbn_product_proof_prove -------
// Between two layers' sumchecks the reference appends the final claims (:352-365), draws challenge_scalar("challenge_r_layer"),
// folds claims_to_verify[i] = l_i + r_layer (r_i - l_i) (:370-372), then opens the next layer: n challenge_scalar("rand_coeffs_next_layer")
// and the joint claim sum_i claims_to_verify[i] c_i (:317-321).  One wavefront does "close" and/or "open" in ONE launch.  No appended value
// depends on a challenge of the same step, so the step runs the whole sponge first and does the field work behind it.
// The host plans every block as one record (transcript_plan.hpp, transcript_plan_boundary): the XOR mask (labels, lengths, headers,
// padding), a flag "a 64-byte challenge is read behind this block's permutation", and for each of the 166 rate bytes the index of the
// data byte XORed there (the closing layer's final claims, canonical, 32 bytes each) or 0xffff.  Keccak-f and the lane layout are
// k_tr_sumcheck_step's.
constexpr int TR_LAYER_DATA_MAX = 80;        // scalars staged for the appends (SC_FINAL_MAX: one per table of the largest sumcheck)
constexpr int TR_LAYER_CHAL_MAX = SC_PACK_MAX + 1;
struct TrLayerArgs {
  const uint8_t* recs; uint32_t nblk;       // the host's plan of this step's STROBE blocks
  uint8_t* strobe;                           // 200 sponge bytes, read and written
  const uint32_t* data; uint32_t ndata;      // close: the closing layer's final claims as canonical integers (A_par.., B_par.., C_par, A_seq.., B_seq.., C_seq..)
  uint32_t n_close;                          // close: the number of product circuits (0: this step closes nothing)
  uint32_t n_open;                           // open: coefficients to draw (0: this step opens nothing)
  uint32_t* claims;                          // claims_to_verify, table format (Montgomery): close writes [0, n_close), open reads [0, n_open)
  uint32_t* out_r;                           // close: r_layer, canonical integer
  uint32_t* out_claims;                      // close: the folded claims_to_verify, canonical integers
  uint32_t* weights;                         // open: c_i R^2 (canonical words), what k_tr_sumcheck_step weights slot i's sums with
  uint32_t* claim;                           // open: the joint claim as nine 29-bit limbs (Montgomery, lazy), k_tr_sumcheck_step's `claim`
  // open of a layer whose sumcheck folds c_i into A_i (the combined kernels, abi_sumcheck.inc mode COMB); null otherwise
  uint32_t n_par_open;                       //   the first n_par_open coefficients belong to the "par" instances, the rest to the "seq" instances
  uint32_t* coeffs_mont;                     //   c_i in Montgomery form (canonical words): the groups' u and the inversion read them
  uint32_t* weights_comb;                    //   SC_PACK_MAX slots of a combined round: the "seq" instances' c_i R^2, then R^2 (the groups' sums carry c_i)
  uint32_t* weights_inst;                    //   the slots of a per-instance round on scaled tables: R^2 for the "par" instances, c_i R^2 for the "seq" ones
};
// lo + hi 2^256 mod r in Montgomery form from 64 challenge bytes (transcript.rs:56-67); (-2 r, 4 r), normalised
__device__ __forceinline__ Fr tr_wide_mont(const uint32_t* ch) {
  uint32_t lo[8], hi[8];
#pragma unroll
  for (int k = 0; k < 8; k++) { lo[k] = ch[k]; hi[k] = ch[8 + k]; }
  return fe_add(fe_mul(fe_unpack<FrP>(lo), fe_const_r2<FrP>()), fe_mul(fe_unpack<FrP>(hi), tr_fr_k778()));
}
__global__ void __launch_bounds__(64) k_tr_layer_step(TrLayerArgs A) {
  __shared__ __attribute__((aligned(16))) uint8_t s_data[TR_LAYER_DATA_MAX * 32];
  __shared__ __attribute__((aligned(16))) uint32_t s_ch[TR_LAYER_CHAL_MAX][16];
  const int lane = threadIdx.x;
  const TrLanes L = tr_lanes(lane);
  uint64_t a = lane < 25 ? reinterpret_cast<const uint64_t*>(A.strobe)[lane] : 0;
  const uint32_t ndata = A.ndata < (uint32_t)TR_LAYER_DATA_MAX ? A.ndata : (uint32_t)TR_LAYER_DATA_MAX;
  for (uint32_t i = lane; i < ndata * 2; i += 64) reinterpret_cast<uint4*>(s_data)[i] = reinterpret_cast<const uint4*>(A.data)[i];
  __syncthreads();
  // 1. the sponge: every block = mask ^ data bytes, then Keccak-f; the next record is requested before the permutation runs
  uint32_t nch = 0;
  const uint8_t* rec = A.recs;
  uint64_t mk = (lane < 25 && A.nblk) ? reinterpret_cast<const uint64_t*>(rec)[lane] : 0;
  uint64_t fl = A.nblk ? *reinterpret_cast<const uint64_t*>(rec + TR_REC_FLAGS) : 0;
  uint4 sr = (lane < 21 && A.nblk) ? reinterpret_cast<const uint4*>(rec + TR_REC_SRC)[lane] : make_uint4(~0u, ~0u, ~0u, ~0u);
  for (uint32_t b = 0; b < A.nblk; b++) {
    uint64_t m = mk; const uint64_t f = fl; const uint4 s = sr;
    if (b + 1 < A.nblk) {
      rec += TR_REC_BYTES;
      mk = lane < 25 ? reinterpret_cast<const uint64_t*>(rec)[lane] : 0;
      fl = *reinterpret_cast<const uint64_t*>(rec + TR_REC_FLAGS);
      sr = lane < 21 ? reinterpret_cast<const uint4*>(rec + TR_REC_SRC)[lane] : make_uint4(~0u, ~0u, ~0u, ~0u);
    }
    const uint32_t sw[4] = {s.x, s.y, s.z, s.w};
#pragma unroll
    for (int q = 0; q < 8; q++) {
      const uint32_t idx = (sw[q >> 1] >> (16 * (q & 1))) & 0xffffu;
      if (idx < ndata * 32u) m ^= (uint64_t)s_data[idx] << (8 * q);
    }
    a = tr_keccak_f(a ^ m, L, lane);
    if ((f & 1) && nch < (uint32_t)TR_LAYER_CHAL_MAX) {        // the PRF's 64 bytes: positions 0 .. 63 of the fresh block, read and cleared
      if (lane < 8) { s_ch[nch][2 * lane] = (uint32_t)a; s_ch[nch][2 * lane + 1] = (uint32_t)(a >> 32); a = 0; }
      nch++;
    }
  }
  if (lane < 25) reinterpret_cast<uint64_t*>(A.strobe)[lane] = a;
  __syncthreads();
  // 2. close: lane i folds circuit i's two claims with r_layer (the first challenge of the step)
  const uint32_t first_coeff = A.n_close ? 1u : 0u;
  Fr cv = fe_zero<FrP>();
  if (A.n_close) {
    const Fr rl = tr_wide_mont(s_ch[0]);
    if (lane == 0) fe_store_packed<FrP>(A.out_r, fe_from_mont(rl));
    if ((uint32_t)lane < A.n_close) {
      const Fr l = fe_to_mont(fe_load<FrP>(s_data + 32 * lane)), r = fe_to_mont(fe_load<FrP>(s_data + 32 * (A.n_close + lane)));
      cv = fe_add(l, fe_mul(rl, fe_sub(r, l)));                                          // (-2 r, 4 r)
      fe_store_tab<FrP>(A.claims + 8 * lane, cv);
      fe_store_packed<FrP>(A.out_claims + 8 * lane, fe_from_mont(cv));
    }
  }
  // 3. open: lane i draws c_i; the joint claim is the wave's sum of claims_to_verify[i] c_i
  if (A.n_open) {
    Fr term = fe_zero<FrP>();
    if ((uint32_t)lane < A.n_open) {
      if ((uint32_t)lane >= A.n_close) cv = fe_load<FrP>(A.claims + 8 * lane);           // not folded by this step: first layer, dot-product circuits
      const Fr ci = tr_wide_mont(s_ch[first_coeff + lane]);
      fe_store<FrP>(A.weights + 8 * lane, fe_mul(ci, fe_const_r2<FrP>()));
      term = fe_mul(cv, ci);                                                             // (-r, 2 r)
      if (A.coeffs_mont) fe_store<FrP>(A.coeffs_mont + 8 * lane, ci);
    }
    if (A.weights_comb) {                                                                // (uniform branch: every lane takes part in the exchange)
      const Fr ci = (uint32_t)lane < A.n_open ? tr_wide_mont(s_ch[first_coeff + lane]) : fe_one<FrP>();
      const Fr w = fe_mul(ci, fe_const_r2<FrP>());
      const uint32_t n_seq = A.n_open - A.n_par_open;
      const Fr ws = tr_shfl(w, (int)((A.n_par_open + (uint32_t)lane) & 63u));           // the "seq" instance that owns combined-round slot `lane`
      if (lane < SC_PACK_MAX) {
        fe_store<FrP>(A.weights_comb + 8 * lane, (uint32_t)lane < n_seq ? ws : fe_const_r2<FrP>());
        fe_store<FrP>(A.weights_inst + 8 * lane, ((uint32_t)lane < A.n_par_open || (uint32_t)lane >= A.n_open) ? fe_const_r2<FrP>() : w);
      }
    }
    const Fr sum = fe_reduce(wave_sum_fr(term));                                         // at most 24 terms: (-24 r, 48 r) -> (-r, 2 r)
    if (lane == 0) for (int k = 0; k < NL; k++) A.claim[k] = sum.v[k];
  }
}

}  // namespace sbn
