// r1cs_kernels.cuh — the sparse R1CS matrices on the device: one segmented sum of val * x[idx] over a compressed matrix.
//
// Reference loops replaced (serial loops over the (row, col, val) triplets there):
//   R1CSShape::multiply_vec -> SparseMatPolynomial::multiply_vec   src/r1cs.rs:132-146, src/sparse_mlpoly.rs:77-87   -> k_r1cs_spmv<false>, row-major
//   compute_eval_table_sparse + the r_A/r_B/r_C combination         src/r1cs.rs:148-163, src/r1csproof.rs:376-387     -> k_r1cs_scale3 + k_r1cs_spmv<false>, column-major
//   R1CSShape::evaluate -> multi_evaluate                           src/r1cs.rs:126-129, src/sparse_mlpoly.rs:113-143 -> k_r1cs_spmv<true>, row-major
//
// Load balance (circom matrices are skewed: the constant column alone fills a large share of all rows, padded rows are empty):
// merge path over (row ends, non-zeros) (Merrill & Garland, SC'16).  The items of the merged list — every non-zero and every
// row end — are cut into chunks of R1CS_CHUNK; a lane walks one chunk, so every lane does the same work whatever the row lengths.
// A lane writes the rows it finishes; the row it is still in when its chunk ends leaves as a carry (row, partial sum).  Carries
// are sorted by row; k_r1cs_fix adds them into the rows in further passes of R1CS_FIX_FIRST, then R1CS_FIX_CHUNK carries per lane, each pass handing
// its own last run on, until one lane is left.  A row receives at most one write or add per pass, so no atomics are needed;
// field addition is exact, so every run gives the same canonical values.
// Arithmetic: products go into fp.cuh's 17 columns (cols_mac) with a carry pass every 6, and one reduction per row-in-chunk.
#pragma once
#include "sumcheck_kernels.cuh"

namespace sbn {

constexpr uint32_t R1CS_CHUNK = 16;          // merge-path items (row ends + non-zeros) per lane
constexpr uint32_t R1CS_FIX_FIRST = 4;       // carries per lane in the first fix-up pass (one carry per chunk: keep the lanes many)
constexpr uint32_t R1CS_FIX_CHUNK = 32;      // carries per lane in the later passes
constexpr unsigned R1CS_EVAL_BLOCKS = 1024;  // k_sc_finish folds up to 64 x 16 block partials

// where row k of the stacked matrix goes: table k >> shift, entry k & (2^shift - 1)
struct R1csOut { uint32_t* p[3]; uint32_t shift; };
__device__ __forceinline__ uint32_t* r1cs_out_ptr(const R1csOut& o, uint32_t k) {
  const uint32_t m = k >> o.shift;
  uint32_t* base = m == 0 ? o.p[0] : (m == 1 ? o.p[1] : o.p[2]);
  return base + 8 * (size_t)(k & ((1u << o.shift) - 1u));
}

// start_row[t] = the number of row ends among the first t * R1CS_CHUNK items of the merged list (t = 0 .. nchunks).
// Row end i is item row_end[i] + i: it comes after the non-zeros of rows 0..i and the row ends before it.
__global__ void __launch_bounds__(256) k_r1cs_partition(const uint32_t* __restrict__ row_end, uint32_t nrows, uint32_t nnz, uint32_t nchunks,
                                                        uint32_t* __restrict__ start_row) {
  const uint64_t total = (uint64_t)nrows + nnz;
  for (uint32_t t = blockIdx.x * blockDim.x + threadIdx.x; t <= nchunks; t += gridDim.x * blockDim.x) {
    const uint64_t d = min((uint64_t)t * R1CS_CHUNK, total);
    uint32_t lo = d > nnz ? (uint32_t)(d - nnz) : 0u, hi = (uint32_t)min(d, (uint64_t)nrows);
    while (lo < hi) {
      const uint32_t mid = lo + (hi - lo) / 2;
      if ((uint64_t)row_end[mid] + mid + 1 <= d) lo = mid + 1; else hi = mid;
    }
    start_row[t] = lo;
  }
}

// x[m * n + i] = r_m * eq[i], m < 3 (r_m in Montgomery form): the gathered vector of the phase-2 table
__global__ void __launch_bounds__(256) k_r1cs_scale3(const uint32_t* __restrict__ eq, uint32_t log_n, ScScalar rA, ScScalar rB, ScScalar rC,
                                                     uint32_t* __restrict__ x) {
  const size_t n = (size_t)1 << log_n;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < 3 * n; i += (size_t)gridDim.x * blockDim.x) {
    const size_t m = i >> log_n;
    const Fr r = fr_from_words(m == 0 ? rA : (m == 1 ? rB : rC));
    fe_gstore_tab<FrP>(x + 8 * i, fe_mul(fe_load<FrP>(eq + 8 * (i & (n - 1))), r));
  }
}

// y = M x over the merged list of one compressed matrix (nrows rows, nnz non-zeros; idx: the column of each non-zero, val: its value,
// x: the gathered vector; all values below 2^256, so every limb is below 2^29 and cols_mac's operand limits hold).
//   EVAL = false: rows a lane finishes go to `out` (canonical); carry_key / carry_val[t] <- the row chunk t ends in and its partial sum
//                 (row nrows when the chunk ends on the last row end).  One chunk per thread.
//   EVAL = true:  each finished row and each partial sum is multiplied by w[row & mask] and added to the sum of matrix row >> shift;
//                 partial[block][3] <- the block's three sums (grid-stride over the chunks, at most R1CS_EVAL_BLOCKS blocks).
template <bool EVAL>
__global__ void __launch_bounds__(256) k_r1cs_spmv(const uint32_t* __restrict__ row_end, const uint32_t* __restrict__ start_row, const uint32_t* __restrict__ idx,
                                                   const uint32_t* __restrict__ val, uint32_t nrows, uint32_t nnz, uint32_t nchunks, const uint32_t* __restrict__ x,
                                                   R1csOut out, uint32_t* __restrict__ carry_key, uint32_t* __restrict__ carry_val,
                                                   const uint32_t* __restrict__ w, uint32_t* __restrict__ partial) {
  const uint64_t total = (uint64_t)nrows + nnz;
  const uint32_t mask = (1u << out.shift) - 1u;
  Fr e0 = fe_zero<FrP>(), e1 = fe_zero<FrP>(), e2 = fe_zero<FrP>();
  uint32_t c0 = 0, c1 = 0, c2 = 0;
  auto eval_add = [&](uint32_t row, const Fr& s) {
    const Fr p = fe_mul(s, fe_load<FrP>(w + 8 * (size_t)(row & mask)));
    const uint32_t m = row >> out.shift;
    if (m == 0) fr_acc(e0, p, c0); else if (m == 1) fr_acc(e1, p, c1); else fr_acc(e2, p, c2);
  };
  for (uint32_t t = blockIdx.x * blockDim.x + threadIdx.x; t < nchunks; t += gridDim.x * blockDim.x) {
    const uint64_t d0 = (uint64_t)t * R1CS_CHUNK, d1 = min(d0 + R1CS_CHUNK, total);
    uint32_t i = start_row[t], j = (uint32_t)(d0 - i);
    uint32_t re = i < nrows ? row_end[i] : nnz;
    Cols acc; cols_zero(acc);
    uint32_t pend = 0; bool any = false;
    for (uint64_t k = d0; k < d1; k++) {
      if (j < re) {                                   // non-zero j of row i
        const uint32_t col = idx[j];
        cols_mac<FrP>(acc, fe_gload<FrP>(val + 8 * (size_t)j), fe_load<FrP>(x + 8 * (size_t)col));
        if (++pend == 6) { cols_carry(acc); pend = 0; }
        any = true; j++;
      } else {                                        // row i ends here (i < nrows: the merge path has no row end past the last row)
        if (EVAL) { if (any && i < nrows) eval_add(i, cols_reduce<FrP>(acc)); }
        else if (i < nrows) fe_gstore<FrP>(r1cs_out_ptr(out, i), any ? cols_reduce<FrP>(acc) : fe_zero<FrP>());
        cols_zero(acc); pend = 0; any = false;
        i++; re = i < nrows ? row_end[i] : nnz;
      }
    }
    if (EVAL) { if (any && i < nrows) eval_add(i, cols_reduce<FrP>(acc)); }
    else {
      carry_key[t] = i;
      fe_gstore<FrP>(carry_val + 8 * (size_t)t, any ? cols_reduce<FrP>(acc) : fe_zero<FrP>());
    }
  }
  if (EVAL) {
    __shared__ uint32_t sm[4][3][NL];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    Fr s[3] = {wave_sum_fr(fe_reduce(e0)), wave_sum_fr(fe_reduce(e1)), wave_sum_fr(fe_reduce(e2))};
    if (lane == 0) {
#pragma unroll
      for (int q = 0; q < 3; q++)
#pragma unroll
        for (int k = 0; k < NL; k++) sm[wv][q][k] = s[q].v[k];
    }
    __syncthreads();
    if (threadIdx.x < 3) {
      const int q = threadIdx.x;
      Fr a = fe_zero<FrP>();
      for (int v = 0; v < 4; v++) { Fr b; for (int k = 0; k < NL; k++) b.v[k] = sm[v][q][k]; a = fe_add(a, b); }
      fe_gstore_tab<FrP>(partial + 8 * ((size_t)blockIdx.x * 3 + q), fe_reduce(a));
    }
  }
}

// row k += s (k < nrows; the carry of a chunk that ended on the last row end has k = nrows and nothing to add)
__device__ __forceinline__ void r1cs_add_out(const R1csOut& out, uint32_t nrows, uint32_t k, const Fr& s) {
  if (k >= nrows) return;
  uint32_t* p = r1cs_out_ptr(out, k);
  fe_gstore<FrP>(p, fe_add(fe_gload<FrP>(p), s));
}
// one fix-up pass over n carries sorted by row: lane t sums runs of equal rows in carries [t F, (t + 1) F) and adds every run but its
// last into the output; the last run goes on as carry t of the next pass (nt = ceil(n / F) carries) — unless this pass has one lane,
// which adds it too.  A run that ends inside lane t's range is added by lane t alone, so no two lanes of a pass touch one row.
__global__ void __launch_bounds__(256) k_r1cs_fix(const uint32_t* __restrict__ key, const uint32_t* __restrict__ val, uint32_t n, uint32_t F, uint32_t nrows,
                                                  R1csOut out, uint32_t* __restrict__ next_key, uint32_t* __restrict__ next_val) {
  const uint32_t nt = (n + F - 1) / F;
  for (uint32_t t = blockIdx.x * blockDim.x + threadIdx.x; t < nt; t += gridDim.x * blockDim.x) {
    const uint32_t a = t * F, b = min(a + F, n);
    uint32_t k = key[a], cnt = 0;
    Fr s = fe_gload<FrP>(val + 8 * (size_t)a);
    for (uint32_t e = a + 1; e < b; e++) {
      const uint32_t ke = key[e];
      const Fr v = fe_gload<FrP>(val + 8 * (size_t)e);
      if (ke != k) { r1cs_add_out(out, nrows, k, s); k = ke; s = v; cnt = 0; }
      else fr_acc(s, v, cnt);
    }
    if (nt == 1) r1cs_add_out(out, nrows, k, s);
    else { next_key[t] = k; fe_gstore<FrP>(next_val + 8 * (size_t)t, s); }
  }
}

// R1CSShape::is_sat's last line (r1cs.rs:121-122) over the three product tables: row i is violated when Az[i] Bz[i] - Cz[i] != 0 (mod r).
// One streaming pass: a lane takes one row at a time (three 32-byte loads, one Montgomery product), the grid is stream_grid's and the loop strides
// over the rows.  The test is on the canonical value of the difference (fe_is_zero), never on the stored words: a table entry is whatever
// representative its producer left.  out[0] += the block's violated rows, out[1] = min(out[1], its lowest violated row): ONE atomicAdd and ONE
// atomicMin a block; the host sets out = {0, 0xffffffff} in front of the launch.  Row numbers are below 2^29 (sbn_r1cs_upload).
__global__ void __launch_bounds__(256) k_r1cs_sat_check(const uint32_t* __restrict__ Az, const uint32_t* __restrict__ Bz, const uint32_t* __restrict__ Cz, uint32_t nrows,
                                                        uint32_t* __restrict__ out) {
  uint32_t bad = 0, first = 0xffffffffu;
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < nrows; i += gridDim.x * blockDim.x) {
    const Fr a = fe_gload<FrP>(Az + 8 * (size_t)i), b = fe_gload<FrP>(Bz + 8 * (size_t)i), cc = fe_gload<FrP>(Cz + 8 * (size_t)i);
    if (!fe_is_zero<FrP>(fe_sub_lazy<FrP>(fe_mul(a, b), fe_norm(cc)))) { bad++; first = min(first, i); }
  }
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) { bad += __shfl_down(bad, d); first = min(first, (uint32_t)__shfl_down(first, d)); }
  __shared__ uint32_t sm[2][4];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  if (lane == 0) { sm[0][wv] = bad; sm[1][wv] = first; }
  __syncthreads();
  if (threadIdx.x == 0) {
    atomicAdd(out, sm[0][0] + sm[0][1] + sm[0][2] + sm[0][3]);
    atomicMin(out + 1, min(min(sm[1][0], sm[1][1]), min(sm[1][2], sm[1][3])));
  }
}

}  // namespace sbn
