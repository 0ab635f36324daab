// small_sum_kernels.cuh — many short sums of FRESH points in one launch (abi_small_sums.inc: sbn_g1_small_sums).
// k_select_sum (r1cs_verify_kernels.cuh) reads a table 2^k P that costs a 253-doubling chain per call; it pays when the same points enter
// many sums.  Here every point enters one sum, so nothing is tabulated: the scalars are cut into 4-bit windows and
//   k_window_sums   one block of 256 lanes per (sum, window) adds digit * P over the sum's at most 64 terms.  Lane t holds bit k = t & 3 of the
//                   window's digit of term t >> 2: 2^k P when the bit is set (at most three doublings in a row), the identity otherwise;
//                   block_sum_quad (g1.cuh) adds the lanes.  The 64 window sums of a sum are folded on the host (252 doublings: the chain
//                   the bucket pipeline leaves to the host as well, host_field.hpp: combine_windows).
//   k_sums_to_host  the hand-over of up to 256 x 64 such sums: k_points_to_host's protocol (zk_sumcheck_kernels.cuh) with one flag per block,
//                   so that 2 MiB do not cross the bus through one block's 256 lanes and no block waits for another.
#pragma once
#include "g1.cuh"
#include "sumcheck_kernels.cuh"

namespace sbn {

constexpr int SS_TERMS_MAX = 64;               // 2 lg n + 4 points of an opening's final equation up to PE_SIDE_MAX = 20
constexpr int SS_WINDOW_BITS = 4;
constexpr int SS_WINDOWS = 64;                 // window 63 holds bits 252 and 253 of a canonical scalar (r < 2^254), and two zero bits
constexpr int SS_DESC_IDX = 64, SS_DESC_SCAL = 128;
constexpr int SS_DESC_WORDS = SS_DESC_SCAL + 8 * SS_TERMS_MAX;      // word 0: the number of terms; 64 + t: the point index of term t; 128 + 8 t ..: its scalar, canonical
constexpr int SS_HANDOVER_POINTS = 64;         // XYZZ sums per block of k_sums_to_host

static_assert(SS_WINDOW_BITS * SS_WINDOWS >= 254 && 4 * SS_TERMS_MAX == 256 && SS_WINDOW_BITS == 4, "one lane per (term, bit of the window)");

// descs: gridDim.x / 64 descriptors.  points: Montgomery affine points in a generator table's layout (all-zero: the identity); the host has
// checked every index against their number.  out: gridDim.x XYZZ sums, out[sum * 64 + window].
__global__ void __launch_bounds__(256) k_window_sums(const uint32_t* __restrict__ descs, const uint32_t* __restrict__ points, uint32_t* __restrict__ out) {
  __shared__ uint32_t sm[4][32];
  wave_prio_helper();
  const uint32_t* d = descs + SS_DESC_WORDS * (size_t)(blockIdx.x / SS_WINDOWS);
  const uint32_t nt = min(d[0], (uint32_t)SS_TERMS_MAX), term = threadIdx.x >> 2, k = threadIdx.x & 3, bit = SS_WINDOW_BITS * (blockIdx.x % SS_WINDOWS) + k;
  XYZZ v = xyzz_inf();
  if (term < nt && ((d[SS_DESC_SCAL + 8 * term + (bit >> 5)] >> (bit & 31)) & 1u)) {
    const Affine p = aff_load(points + 16 * (size_t)d[SS_DESC_IDX + term]);
    if (k == 0) v = xyzz_from_affine(p);
    else if (!aff_is_inf(p)) {
      v = xyzz_dbl_affine(p);
#pragma unroll 1
      for (uint32_t j = 1; j < k; j++) v = xyzz_dbl(v);
    }
  }
  const XYZZ s = block_sum_quad(v, sm);
  if (threadIdx.x == 0) xyzz_store(out + 32 * (size_t)blockIdx.x, s);
}

// nquads 16-byte pieces of XYZZ sums to the host's hand-over area; block b takes the pieces of points [64 b, 64 b + 64) and raises flags[b]
__global__ void __launch_bounds__(256) k_sums_to_host(const uint4* __restrict__ sums, uint32_t nquads, uint4* __restrict__ host_out, uint32_t* __restrict__ flags, uint32_t seq) {
  wave_prio_helper();
  const uint32_t lo = blockIdx.x * (8 * SS_HANDOVER_POINTS), hi = min(lo + 8 * SS_HANDOVER_POINTS, nquads);
  for (uint32_t t = lo + threadIdx.x; t < hi; t += blockDim.x) host_out[t] = sums[t];
  sc_drain_stores();
  __syncthreads();
  if (threadIdx.x == 0) sc_flag_store(flags + blockIdx.x, seq);
}

}  // namespace sbn
