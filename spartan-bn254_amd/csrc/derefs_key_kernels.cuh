// derefs_key_kernels.cuh — the kernels sbn_derefs_key (abi_sparse_eval_kzg.inc) adds to the bucket accumulate it reuses:
// the KZG build's derefs commitment (sparse_mlpoly_full.rs:307-312) as a sum over memory cells,
//   sum_i derefs[i] [tau^i]G = sum_a eq[a] S_a,   S_a = sum_{i : addr[i] = a} [tau^i]G.
//   k_dk_place     the sorted entry lists of the 2 x cells buckets from the counting sort sbn_dense already holds: audit_ts is the per-cell
//                  count, read_ts the rank within the cell, so entry e goes to offs[cell] + read_ts[e] with no atomics and no second sort
//   k_dk_gather    the buckets of the cells read at least once, compacted (XYZZ, 128 B each)
//   k_dk_scalars   eq(rx)[a] / eq(ry)[a] of the kept cells as canonical integers: the MSM's scalars (replaces k_scalars_from_internal over
//                  the gathered table)
#pragma once
#include "msm_kernels.cuh"

namespace sbn {

// u32s: row addr | row read_ts | col addr | col read_ts, bN entries each (sbn_dense).  Entry e = side * bN + j is coefficient
// (side * b + k) * N + i of the merged derefs polynomial (Derefs::new, :293-297), i.e. e itself; bit 31 stays clear: every point enters positive.
// An address or a rank outside the handle's shape writes nothing (sbn_dense_build cannot produce one).
__global__ void __launch_bounds__(256) k_dk_place(const uint32_t* __restrict__ u32s, size_t bN, uint32_t cells, const uint32_t* __restrict__ hist,
                                                  const uint32_t* __restrict__ offs, uint32_t* __restrict__ sorted) {
  for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < 2 * bN; e += (size_t)gridDim.x * blockDim.x) {
    const size_t side = e >= bN ? 1 : 0, j = e - side * bN;
    const uint32_t a = u32s[side * 2 * bN + j], rk = u32s[side * 2 * bN + bN + j];
    if (a >= cells) continue;
    const size_t t = side * (size_t)cells + a;
    if (rk >= hist[t]) continue;
    const size_t pos = (size_t)offs[t] + rk;
    if (pos < bN) sorted[side * bN + pos] = (uint32_t)e;
  }
}

__global__ void __launch_bounds__(256) k_dk_gather(const uint32_t* __restrict__ buckets, const uint32_t* __restrict__ ids, uint32_t cells, size_t len,
                                                   uint32_t* __restrict__ out) {
  for (size_t j = (size_t)blockIdx.x * blockDim.x + threadIdx.x; j < len; j += (size_t)gridDim.x * blockDim.x) {
    const uint32_t id = ids[j];
    const size_t t = (size_t)(id >> 31) * cells + (id & 0x7fffffffu);
    xyzz_store(out + 32 * j, xyzz_load(buckets + 32 * t));
  }
}

__global__ void __launch_bounds__(256) k_dk_scalars(const uint32_t* __restrict__ mem_rx, const uint32_t* __restrict__ mem_ry, const uint32_t* __restrict__ ids,
                                                    size_t len, uint32_t* __restrict__ out) {
  for (size_t j = (size_t)blockIdx.x * blockDim.x + threadIdx.x; j < len; j += (size_t)gridDim.x * blockDim.x) {
    const uint32_t id = ids[j];
    const uint32_t* m = (id >> 31) ? mem_ry : mem_rx;
    fe_store_packed<FrP>(out + 8 * j, fe_from_mont(fe_load<FrP>(m + 8 * (size_t)(id & 0x7fffffffu))));
  }
}

}  // namespace sbn
