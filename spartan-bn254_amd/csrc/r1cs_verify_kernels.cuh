// r1cs_verify_kernels.cuh — the group work of sbn_r1cs_proof_verify / sbn_zk_sumcheck_verify (abi_r1cs_verify.inc): R1CSProof::verify
// (r1csproof.rs:463-619) and ZKSumcheckInstanceProof::verify (sumcheck.rs:366-457).
// Every point that enters one of the verifier's checks is a point of the proof or a generator, and every coefficient is a scalar the host
// derives from the transcript, so every check is a sum of entries of ONE table, selected by scalar bits:
//   k_pow2_table   T[p][k] = 2^k P_p for k < 254, XYZZ, one lane per point (the proof's decompressed points, then the generators, read from
//                  their handles); once per call.  The 253 doublings of a point are a serial chain in one lane; all points run side by side.
//   k_select_sum   one block per sum of at most 8 terms (point index, canonical scalar): each lane adds the table entries of its share of the
//                  (term, bit) pairs whose bit is set, block_sum_quad (g1.cuh) adds the lanes: a tree of depth ~10 in place of a 254-step
//                  double-and-add.  A single sum goes straight to the host's hand-over area (the transcript needs its bytes); the last launch
//                  of a call takes every equation, moved to one side, and sends back "the sum is the identity" as packed bits.
#pragma once
#include "decompress_kernels.cuh"

namespace sbn {

constexpr int POW2_BITS = 254;                 // a canonical scalar is below r < 2^254
constexpr int SEL_TERMS_MAX = 8;
constexpr int SEL_DESC_WORDS = 80;             // word 0: the number of terms; 1 .. 8: point indices; 16 + 8 t ..: the scalar of term t, canonical
constexpr int POW2_SRC_MAX = 4;

// the points of the table in order: n[s] Montgomery affine points (a generator table's layout) at p[s]
struct Pow2Src { const uint32_t* p[POW2_SRC_MAX]; uint32_t n[POW2_SRC_MAX]; };

__global__ void __launch_bounds__(64) k_pow2_table(Pow2Src S, uint32_t total, uint32_t* __restrict__ table) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  uint32_t j = i; const uint32_t* src = nullptr;
#pragma unroll
  for (int s = 0; s < POW2_SRC_MAX; s++)
    if (!src) { if (j < S.n[s]) src = S.p[s] + 16 * (size_t)j; else j -= S.n[s]; }
  XYZZ v = xyzz_from_affine(aff_load(src));
  uint32_t* o = table + 32 * (size_t)i * POW2_BITS;
#pragma unroll 1
  for (int k = 0; k < POW2_BITS; k++) {
    xyzz_store(o + 32 * k, v);
    if (k + 1 < POW2_BITS) v = xyzz_dbl(v);
  }
}

// descs: gridDim.x descriptors.  out: gridDim.x XYZZ sums, or null.  bits: bit b of the packed words is set when sum b is the identity (the
// words are zero before the launch), or null.  host_out (one block only), or null: the sum, then the na words at ea and the nb words at eb
// that travel with it, to the host's hand-over area, the flag behind them.
__global__ void __launch_bounds__(256) k_select_sum(const uint32_t* __restrict__ descs, const uint32_t* __restrict__ table, uint32_t* __restrict__ out,
                                                    uint32_t* __restrict__ bits, const uint32_t* __restrict__ ea, uint32_t na, const uint32_t* __restrict__ eb, uint32_t nb,
                                                    uint32_t* __restrict__ host_out, uint32_t* __restrict__ flag, uint32_t seq) {
  __shared__ uint32_t sm[4][32];
  const uint32_t* d = descs + SEL_DESC_WORDS * (size_t)blockIdx.x;
  const uint32_t nt = min(d[0], (uint32_t)SEL_TERMS_MAX), npairs = nt * POW2_BITS;
  XYZZ acc = xyzz_inf();
#pragma unroll 1
  for (uint32_t j = threadIdx.x; j < npairs; j += blockDim.x) {
    const uint32_t term = j / POW2_BITS, bit = j - term * POW2_BITS;
    if ((d[16 + 8 * term + (bit >> 5)] >> (bit & 31)) & 1u)
      acc = xyzz_add_inl(acc, xyzz_load(table + 32 * ((size_t)d[1 + term] * POW2_BITS + bit)));
  }
  const XYZZ s = block_sum_quad(acc, sm);
  if (threadIdx.x == 0) {
    if (out) xyzz_store(out + 32 * (size_t)blockIdx.x, s);
    if (bits && xyzz_is_inf(s)) atomicOr(bits + (blockIdx.x >> 5), 1u << (blockIdx.x & 31));
    if (host_out) xyzz_store(host_out, s);
  }
  if (host_out) {
    for (uint32_t t = threadIdx.x; t < na + nb; t += blockDim.x) host_out[32 + t] = t < na ? ea[t] : eb[t - na];
    sc_drain_stores();
    __syncthreads();
    if (threadIdx.x == 0) sc_flag_store(flag, seq);
  }
}

}  // namespace sbn
