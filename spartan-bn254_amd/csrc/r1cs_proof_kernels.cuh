// r1cs_proof_kernels.cuh — the kernels sbn_r1cs_proof_prove (abi_r1cs_proof.inc) adds to the pieces it composes: R1CSProof::prove
// (r1csproof.rs:241-459).
//   k_r1cs_build_z        z = vars ‖ 1 ‖ input ‖ 0 ...  (r1csproof.rs:268-277) as a table of 2 num_vars entries
//   k_r1cs_sigma_rows     the n-row form of k_zk_host_rows: rows [0 ... 0 ‖ v ‖ b] over a derived set that ends in gens_1's two points — every
//                         group element of KnowledgeProof / ProductProof / EqualityProof::prove (nizk/mod.rs:34-59, :167-227, :96-124) is one
// The rows' XYZZ sums go to the host (k_points_to_host) in the four ZK mailbox slots, which are contiguous and idle between the two sumchecks.
#pragma once
#include "zk_sumcheck_kernels.cuh"

namespace sbn {

constexpr int R1CS_SIGMA_ROWS_MAX = 11;      // the Σ step behind phase 1: 2 (knowledge) + 6 (product) + 3 (equality) elements; the last step has 3
static_assert(R1CS_SIGMA_ROWS_MAX * 32 <= ZK_MBOX_SLOTS * ZK_MBOX_SLOT_WORDS, "mailbox: the XYZZ sums of the Σ step must fit the four ZK result slots together");

// z[i] = vars[i] for i < nv (copied as it is: a table entry), z[nv] = 1, z[nv + 1 + k] = input[k] (canonical words in, table representation
// out), zero behind them.  One entry per lane and step: two 16-byte loads and two 16-byte stores, consecutive lanes on consecutive entries.
// Reads 32 nv bytes, writes 64 nv: a streaming kernel — the grid is stream_grid's (about 8 blocks per CU), the loop strides over it.
__global__ void __launch_bounds__(256) k_r1cs_build_z(const uint32_t* __restrict__ vars, const uint32_t* __restrict__ input, size_t nv, size_t num_inputs,
                                                      uint32_t* __restrict__ z) {
  const size_t total = 2 * nv;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    sbn_g_u32x4* o = (sbn_g_u32x4*)(z + 8 * i);
    if (i < nv) {
      const sbn_g_u32x4* s = (const sbn_g_u32x4*)(vars + 8 * i);
      const sbn_u32x4 lo = s[0], hi = s[1];
      o[0] = lo; o[1] = hi;
    } else if (i == nv) {
      fe_gstore_tab<FrP>(z + 8 * i, fe_one<FrP>());
    } else if (i - nv - 1 < num_inputs) {
      fe_gstore_tab<FrP>(z + 8 * i, fe_to_mont(fe_gload<FrP>(input + 8 * (i - nv - 1))));
    } else {
      sbn_u32x4 zero; zero.x = zero.y = zero.z = zero.w = 0u;
      o[0] = zero; o[1] = zero;
    }
  }
}

// nrows rows of R columns: zero but for the last two, which take v[row], b[row] (canonical words, 16 words a row in `vb`)
struct R1csSigmaRows { uint32_t vb[R1CS_SIGMA_ROWS_MAX][16]; };
__global__ void __launch_bounds__(256) k_r1cs_sigma_rows(uint32_t* __restrict__ rows, uint32_t R, uint32_t nrows, R1csSigmaRows A) {
  for (uint32_t t = threadIdx.x; t < nrows * R; t += blockDim.x) {
    const uint32_t row = t / R, col = t - row * R;
    const uint32_t* src = col + 2 == R ? A.vb[row] : A.vb[row] + 8;      // (read straight from the kernel-argument segment: no copy, no scratch)
    const bool live = col + 2 >= R;
    sbn_u32x4 lo, hi;
    lo.x = live ? src[0] : 0u; lo.y = live ? src[1] : 0u; lo.z = live ? src[2] : 0u; lo.w = live ? src[3] : 0u;
    hi.x = live ? src[4] : 0u; hi.y = live ? src[5] : 0u; hi.z = live ? src[6] : 0u; hi.w = live ? src[7] : 0u;
    sbn_g_u32x4* o = (sbn_g_u32x4*)(rows + 8 * t);
    o[0] = lo; o[1] = hi;
  }
}

}  // namespace sbn
