// kzg_kernels.cuh — KZG openings on device tables (reference src/kzg.rs): evaluate-and-divide by (X - z), the gamma combination of
// a batched opening and the powers of tau of an SRS.
//
// Division.  With r_n = 0 and r_i = p_i + z r_{i+1}, p(z) = r_0 and the quotient (p - p(z)) / (X - z) has q_i = r_{i+1}
// (evaluate_poly + compute_quotient, kzg.rs:220-260).  The recurrence runs from the top coefficient down; it is cut into tiles of
// KZG_TILE coefficients, one block each:
//   k_kzg_div_tiles  pass 1: h_t = sum_j p_{tT+j} z^j, the tile's Horner value with a zero carry in
//   (recursion)      the carry INTO tile t is sum_{s>t} h_s (z^T)^(s-t-1): the quotient of the h vector at z^T — the same problem,
//                    1024 times smaller, solved by the same two kernels (its eval is p(z))
//   k_kzg_div_quot   pass 3: the tile again from its carry, writing q; a single tile (the last level) also writes p(z)
// Inside a block each lane owns KZG_E consecutive coefficients (staged through LDS so that global accesses stay coalesced);
// the lanes' Horner values are joined by a suffix scan over the block with the multipliers z^(E 2^s).
// Inputs are any non-negative representatives below 2^256 (the lazy ranges other kernels leave in tables); every stored value is
// brought below 1.0001 r by kzg_shrink.  No inter-block waiting anywhere.
#pragma once
#include "sumcheck_kernels.cuh"

namespace sbn {

constexpr int KZG_E = 4, KZG_THREADS = 256, KZG_TILE = KZG_E * KZG_THREADS, KZG_TILE_LOG = 10, KZG_SCAN_STEPS = 8;
constexpr int KZG_LDS_U4 = 2 * KZG_TILE + KZG_THREADS;     // 16-byte slots: two per coefficient + one pad per lane (bank spread)
// the multipliers of one level: z itself and w[s] = z^(E 2^s), all in Montgomery form
struct KzgPow { ScScalar z; ScScalar w[KZG_SCAN_STEPS]; };

// x normalised, non-negative, value below 8r  ->  the same value minus k r, in [0, 1.0001 r).  k = floor(top / (P8 + 1)) never
// overshoots (r > P8 2^232 and the low limbs are below 2^232) and leaves less than (P8 + k + 1) 2^232.
__device__ __forceinline__ Fr kzg_shrink(const Fr& x) {
  constexpr uint32_t P8 = FrP::P29[8];
  const uint32_t k = x.v[NL - 1] / (P8 + 1u);
  Fr r; int64_t carry = 0;
#pragma unroll
  for (int i = 0; i < NL; i++) {
    const int64_t t = (int64_t)x.v[i] - (int64_t)k * (int64_t)p29<FrP>(i) + carry;
    if (i < NL - 1) { r.v[i] = (uint32_t)t & LMASK; carry = t >> 29; } else r.v[i] = (uint32_t)t;
  }
  return r;
}
// a + b * m with a below 2^256 (5.3 r), b below 8 r, m canonical: below 6.4 r
__device__ __forceinline__ Fr kzg_madd(const Fr& a, const Fr& b, const Fr& m) { return fe_normu(fe_add_lazy(a, fe_mulu(b, m))); }

__device__ __forceinline__ int kzg_slot(int e) { return 2 * e + e / KZG_E; }     // LDS slot of tile coefficient e

// the tile's coefficients [t T, t T + T) into LDS (zero at and above n), coalesced 16-byte loads
__device__ __forceinline__ void kzg_stage_in(const uint32_t* __restrict__ p, size_t n, size_t base, sbn_u32x4* lds) {
  const sbn_g_u32x4* g = (const sbn_g_u32x4*)(p + 8 * base);
#pragma unroll
  for (int m = 0; m < 2 * KZG_E; m++) {
    const int idx = m * KZG_THREADS + (int)threadIdx.x, e = idx >> 1;
    sbn_u32x4 v = {0u, 0u, 0u, 0u};
    if (base + (size_t)e < n) v = g[idx];
    lds[kzg_slot(e) + (idx & 1)] = v;
  }
}
__device__ __forceinline__ Fr kzg_lds_get(const sbn_u32x4* lds, int e) {
  const sbn_u32x4 lo = lds[kzg_slot(e)], hi = lds[kzg_slot(e) + 1];
  const uint32_t w[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
  return fe_unpack<FrP>(w);
}
__device__ __forceinline__ void kzg_lds_put(sbn_u32x4* lds, int e, const Fr& a /* normalised, below 2^256 */) {
  uint32_t w[8]; fe_pack<FrP>(a, w);
  sbn_u32x4 lo, hi;
  lo.x = w[0]; lo.y = w[1]; lo.z = w[2]; lo.w = w[3]; hi.x = w[4]; hi.y = w[5]; hi.z = w[6]; hi.w = w[7];
  lds[kzg_slot(e)] = lo; lds[kzg_slot(e) + 1] = hi;
}
// S_i = sum_{k >= i} l_k W^(k - i) over the block's lanes (W = z^E): Kogge-Stone, 8 steps through LDS
__device__ __forceinline__ Fr kzg_block_suffix(Fr l, const KzgPow& pw, Fr* sh) {
  const int i = (int)threadIdx.x;
#pragma unroll
  for (int s = 0; s < KZG_SCAN_STEPS; s++) {
    sh[i] = l;
    __syncthreads();
    if (i + (1 << s) < KZG_THREADS) l = kzg_shrink(kzg_madd(l, sh[i + (1 << s)], fr_from_words(pw.w[s])));
    __syncthreads();
  }
  return l;
}

// pass 1: h[t] = the Horner value of tile t with a zero carry in
__global__ void __launch_bounds__(KZG_THREADS) k_kzg_div_tiles(const uint32_t* __restrict__ p, size_t n, KzgPow pw, uint32_t* __restrict__ h) {
  __shared__ sbn_u32x4 lds[KZG_LDS_U4];
  __shared__ Fr sh[KZG_THREADS];
  const size_t base = (size_t)blockIdx.x * KZG_TILE;
  kzg_stage_in(p, n, base, lds);
  __syncthreads();
  const Fr z = fr_from_words(pw.z);
  const int i = (int)threadIdx.x;
  Fr r = fe_zero<FrP>();
#pragma unroll
  for (int e = KZG_E - 1; e >= 0; e--) r = kzg_madd(kzg_lds_get(lds, i * KZG_E + e), r, z);
  r = kzg_block_suffix(kzg_shrink(r), pw, sh);
  if (i == 0) fe_gstore_packed<FrP>(h + 8 * blockIdx.x, r);
}

// pass 3: tile t again from its carry (carry[t]; null = zero), q_j = r_{j+1} for j < qlen (coalesced through LDS); with eval != null
// (a single tile) also p(z) = r_0 as a canonical integer
__global__ void __launch_bounds__(KZG_THREADS) k_kzg_div_quot(const uint32_t* __restrict__ p, size_t n, const uint32_t* __restrict__ carry, KzgPow pw,
                                                          uint32_t* __restrict__ q, size_t qlen, uint32_t* __restrict__ eval) {
  __shared__ sbn_u32x4 lds[KZG_LDS_U4];
  __shared__ Fr sh[KZG_THREADS];
  const size_t base = (size_t)blockIdx.x * KZG_TILE;
  kzg_stage_in(p, n, base, lds);
  const Fr z = fr_from_words(pw.z), w0 = fr_from_words(pw.w[0]);
  const Fr cin = carry ? fe_gload<FrP>(carry + 8 * blockIdx.x) : fe_zero<FrP>();
  __syncthreads();
  const int i = (int)threadIdx.x;
  Fr pe[KZG_E];
#pragma unroll
  for (int e = 0; e < KZG_E; e++) pe[e] = kzg_lds_get(lds, i * KZG_E + e);
  Fr l = fe_zero<FrP>();
#pragma unroll
  for (int e = KZG_E - 1; e >= 0; e--) l = kzg_madd(pe[e], l, z);
  if (i == KZG_THREADS - 1) l = kzg_madd(kzg_shrink(l), cin, w0);     // the last lane also carries the tile's carry: S_i = r_{iE}
  const Fr S = kzg_block_suffix(kzg_shrink(l), pw, sh);
  sh[i] = S;                                                          // (kzg_block_suffix ends on a barrier)
  __syncthreads();
  Fr r = i + 1 < KZG_THREADS ? sh[i + 1] : cin;                       // r at the lane's top coefficient + 1
  if (eval && blockIdx.x == 0 && i == 0) fe_gstore_packed<FrP>(eval, fe_from_mont(S));
#pragma unroll
  for (int e = KZG_E - 1; e >= 0; e--) {
    r = kzg_shrink(r);
    kzg_lds_put(lds, i * KZG_E + e, r);                             // q_{iE+e} = r_{iE+e+1}; only this lane touches these slots
    r = kzg_madd(pe[e], r, z);
  }
  __syncthreads();
  sbn_g_u32x4* g = (sbn_g_u32x4*)(q + 8 * base);
#pragma unroll
  for (int m = 0; m < 2 * KZG_E; m++) {
    const int idx = m * KZG_THREADS + i, e = idx >> 1;
    if (base + (size_t)e < qlen) g[idx] = lds[kzg_slot(e) + (idx & 1)];
  }
}

// batched openings (kzg.rs:278-288): out[i] = sum_k gamma^k p_k[i] over i < n, p_k[i] = 0 from ns[k] on; gpow: K Montgomery powers
__global__ void __launch_bounds__(256) k_kzg_combine(const uint32_t* const* __restrict__ tabs, const size_t* __restrict__ ns, const uint32_t* __restrict__ gpow, size_t K,
                                                     size_t n, uint32_t* __restrict__ out) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    Fr acc = fe_zero<FrP>();
    for (size_t k = 0; k < K; k++) {
      if (i >= ns[k]) continue;
      acc = kzg_shrink(kzg_madd(acc, fe_gload<FrP>(tabs[k] + 8 * i), fe_gload<FrP>(gpow + 8 * k)));
    }
    fe_gstore_packed<FrP>(out + 8 * i, acc);
  }
}

// tau^i for i < n as canonical integers (the scalars of an SRS: KZGSrs::setup, kzg.rs:37-56): lane t takes 16 consecutive powers, its
// first one assembled from pw2[k] = tau^(2^k) (Montgomery form)
constexpr int KZG_POW_RUN = 16, KZG_POW_BITS = 40;
struct KzgPow2 { ScScalar v[KZG_POW_BITS]; };
__global__ void __launch_bounds__(256) k_fr_powers(KzgPow2 pw2, size_t n, uint32_t* __restrict__ out) {
  const size_t base = ((size_t)blockIdx.x * blockDim.x + threadIdx.x) * KZG_POW_RUN;
  if (base >= n) return;
  Fr acc = fe_one<FrP>();
#pragma unroll
  for (int k = 4; k < KZG_POW_BITS; k++)                              // base is a multiple of 16
    if ((base >> k) & 1) acc = fe_mulu(acc, fr_from_words(pw2.v[k]));
  const Fr t = fr_from_words(pw2.v[0]);
  for (int e = 0; e < KZG_POW_RUN && base + e < n; e++) {
    fe_gstore_packed<FrP>(out + 8 * (base + e), fe_from_mont(acc));
    acc = fe_mulu(acc, t);
  }
}

}  // namespace sbn
