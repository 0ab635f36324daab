// dense_kernels.cuh — MultiSparseMatPolynomialAsDense on the device: padded address arrays, memory-checking timestamps, comb_ops / comb_mem.
//
// Reference loops replaced (serial on the host there, run once per circuit by SNARK::encode -> R1CSShape::commit, src/r1cs.rs:375-400):
//   SparseMatPolynomial::sparse_to_dense_vecs        src/sparse_mlpoly_full.rs:89-101    -> k_dense_expand
//   AddrTimestamps::new (the read_ts / audit_ts loop) src/sparse_mlpoly_full.rs:211-243   -> k_dense_hist / _scan / _scan_top / _scatter (per radix pass),
//                                                                                            k_dense_bounds, k_dense_rank
//   multi_sparse_to_dense_rep (merge into comb_ops, comb_mem)  src/sparse_mlpoly_full.rs:120-174, src/hyrax.rs:237-251 -> k_dense_tables
//
// Timestamps.  The reference walks the batch * N ops of one side in (k, i) order with one audit_ts: read_ts of an op is the number of
// EARLIER ops on the same cell, audit_ts of a cell the number of all ops on it.  Here the ops are sorted stably by address (payload: the
// op's index k * N + i); an op's read_ts is then its sorted position minus the position its run of equal addresses starts at, and a
// cell's audit_ts the length of its run.
//
// The sort is a least-significant-digit radix sort over the bits an address can have (log2 of the cell count), in passes of at most
// DENSE_RADIX_BITS.  One pass: per-tile digit counts (LDS atomics only COUNT, their return values are not used) -> exclusive scan of the
// digit-major (digit, tile) counts in chunks, then of the chunk sums -> scatter.  The scatter ranks an element inside its tile without
// any atomic: the lanes of a wave that hold the same digit find each other with one ballot per digit bit (match-any), an element's rank
// in its wave round is the number of such lanes below it, and per-wave running counts in LDS carry the rank over the rounds; the waves'
// totals are then prefixed per digit.  Every step is a function of the input order alone, and its cost does not depend on how the keys
// are distributed: all ops on one cell take the same path as all ops on distinct cells.
#pragma once
#include "sumcheck_kernels.cuh"

namespace sbn {

constexpr uint32_t DENSE_RADIX_BITS = 8;
constexpr uint32_t DENSE_BINS = 1u << DENSE_RADIX_BITS;
constexpr uint32_t DENSE_BLOCK = 256;                              // 4 waves; one thread per digit in the per-digit steps
constexpr uint32_t DENSE_WAVES = DENSE_BLOCK / 64;
constexpr uint32_t DENSE_ITEMS = 8;                                // wave rounds per tile
constexpr uint32_t DENSE_TILE = DENSE_BLOCK * DENSE_ITEMS;         // elements per sort block
constexpr uint32_t DENSE_SCAN_ITEMS = 8;
constexpr uint32_t DENSE_SCAN_CHUNK = DENSE_BLOCK * DENSE_SCAN_ITEMS;   // counts per scan block
constexpr uint32_t DENSE_SCAN_SHIFT = 11;
static_assert(DENSE_SCAN_CHUNK == (1u << DENSE_SCAN_SHIFT), "chunk index = entry >> DENSE_SCAN_SHIFT");
static_assert(DENSE_BINS == DENSE_BLOCK, "one thread per digit");
constexpr int DENSE_MAX_BATCH = 8;

// where the triplets of matrix k start in the staged upload, and how many there are
struct DenseArgs { uint32_t off[DENSE_MAX_BATCH]; uint32_t nnz[DENSE_MAX_BATCH]; };
// (statically indexed selects: a dynamic index into a by-value argument would make the compiler copy it to scratch)
__device__ __forceinline__ void dense_pick(const DenseArgs& a, uint32_t k, uint32_t& off, uint32_t& nnz) {
  off = 0; nnz = 0;
#pragma unroll
  for (int j = 0; j < DENSE_MAX_BATCH; j++) if ((uint32_t)j == k) { off = a.off[j]; nnz = a.nnz[j]; }
}

// sparse_to_dense_vecs (sparse_mlpoly_full.rs:89-101) for both sides: entry k * N + i of row_addr / col_addr <- the i-th triplet of
// matrix k in the caller's order, 0 from nnz[k] on.  N = 2^log_n.
__global__ void __launch_bounds__(256) k_dense_expand(const uint32_t* __restrict__ rows, const uint32_t* __restrict__ cols, DenseArgs a, uint32_t log_n,
                                                      uint32_t total, uint32_t* __restrict__ row_addr, uint32_t* __restrict__ col_addr) {
  for (uint32_t e = blockIdx.x * blockDim.x + threadIdx.x; e < total; e += gridDim.x * blockDim.x) {
    const uint32_t k = e >> log_n, i = e & ((1u << log_n) - 1u);
    uint32_t off, nnz; dense_pick(a, k, off, nnz);
    const bool live = i < nnz;
    row_addr[e] = live ? rows[off + i] : 0u;
    col_addr[e] = live ? cols[off + i] : 0u;
  }
}

// exclusive scan of one value per thread over the block (256 threads); *total <- the block's sum.  sm: DENSE_WAVES words.
__device__ __forceinline__ uint32_t dense_block_scan(uint32_t v, uint32_t* sm, uint32_t* total) {
  const uint32_t lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  uint32_t inc = v;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) { const uint32_t o = __shfl_up(inc, d, 64); if (lane >= (uint32_t)d) inc += o; }
  __syncthreads();                                  // sm may still be read from an earlier call
  if (lane == 63) sm[wv] = inc;
  __syncthreads();
  uint32_t base = 0, sum = 0;
#pragma unroll
  for (uint32_t w = 0; w < DENSE_WAVES; w++) { const uint32_t t = sm[w]; if (w < wv) base += t; sum += t; }
  *total = sum;
  return base + inc - v;
}

// counts[d * ntiles + tile] <- the number of keys of tile `tile` whose digit (key >> shift) & mask is d
__global__ void __launch_bounds__(DENSE_BLOCK) k_dense_hist(const uint32_t* __restrict__ keys, uint32_t n, uint32_t shift, uint32_t mask, uint32_t ntiles,
                                                            uint32_t* __restrict__ counts) {
  __shared__ uint32_t h[DENSE_BINS];
  const uint32_t tile = blockIdx.x;
  h[threadIdx.x] = 0;
  __syncthreads();
  const uint32_t base = tile * DENSE_TILE;
#pragma unroll
  for (uint32_t r = 0; r < DENSE_ITEMS; r++) {
    const uint32_t p = base + r * DENSE_BLOCK + threadIdx.x;
    if (p < n) atomicAdd(&h[(keys[p] >> shift) & mask], 1u);          // counting only: the sum does not depend on the order
  }
  __syncthreads();
  counts[(size_t)threadIdx.x * ntiles + tile] = h[threadIdx.x];
}

// in-place exclusive scan of chunk blockIdx.x of `data` (DENSE_SCAN_CHUNK entries, the last one shorter); sums[blockIdx.x] <- its total
__global__ void __launch_bounds__(DENSE_BLOCK) k_dense_scan(uint32_t* __restrict__ data, uint32_t n, uint32_t* __restrict__ sums) {
  __shared__ uint32_t sm[DENSE_WAVES];
  const uint32_t first = blockIdx.x * DENSE_SCAN_CHUNK + threadIdx.x * DENSE_SCAN_ITEMS;
  uint32_t v[DENSE_SCAN_ITEMS], s = 0;
#pragma unroll
  for (uint32_t j = 0; j < DENSE_SCAN_ITEMS; j++) { v[j] = first + j < n ? data[first + j] : 0u; s += v[j]; }
  uint32_t total;
  uint32_t run = dense_block_scan(s, sm, &total);
#pragma unroll
  for (uint32_t j = 0; j < DENSE_SCAN_ITEMS; j++) { if (first + j < n) data[first + j] = run; run += v[j]; }
  if (threadIdx.x == 0) sums[blockIdx.x] = total;
}
// in-place exclusive scan of the chunk sums by one block
__global__ void __launch_bounds__(DENSE_BLOCK) k_dense_scan_top(uint32_t* __restrict__ sums, uint32_t n) {
  __shared__ uint32_t sm[DENSE_WAVES];
  uint32_t carry = 0;
  for (uint32_t base = 0; base < n; base += DENSE_BLOCK) {
    const uint32_t i = base + threadIdx.x;
    const uint32_t v = i < n ? sums[i] : 0u;
    uint32_t total;
    const uint32_t ex = dense_block_scan(v, sm, &total);
    if (i < n) sums[i] = carry + ex;
    carry += total;
  }
}

// One stable pass: element p of tile blockIdx.x goes to (scanned count of its (digit, tile)) + (its rank among the tile's elements with
// that digit, in input order).  Element order inside a tile: wave w holds [w * 64 * ITEMS, (w + 1) * 64 * ITEMS), round r of it the 64
// consecutive elements from r * 64.  idx_in == nullptr: the payload is the position itself (first pass).
__global__ void __launch_bounds__(DENSE_BLOCK) k_dense_scatter(const uint32_t* __restrict__ keys_in, const uint32_t* __restrict__ idx_in, uint32_t n, uint32_t shift,
                                                               uint32_t mask, uint32_t ntiles, const uint32_t* __restrict__ counts, const uint32_t* __restrict__ sums,
                                                               uint32_t* __restrict__ keys_out, uint32_t* __restrict__ idx_out) {
  __shared__ uint32_t cnt[DENSE_WAVES][DENSE_BINS];
  const uint32_t tile = blockIdx.x, lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const uint64_t below = ((uint64_t)1 << lane) - 1;
#pragma unroll
  for (uint32_t w = 0; w < DENSE_WAVES; w++) cnt[w][threadIdx.x] = 0;
  __syncthreads();
  const uint32_t base = tile * DENSE_TILE + wv * (64 * DENSE_ITEMS) + lane;
  uint32_t key[DENSE_ITEMS], pay[DENSE_ITEMS], rank[DENSE_ITEMS];
#pragma unroll
  for (uint32_t r = 0; r < DENSE_ITEMS; r++) {
    const uint32_t p = base + r * 64;
    const bool live = p < n;
    key[r] = live ? keys_in[p] : 0u;
    pay[r] = live ? (idx_in ? idx_in[p] : p) : 0u;
    const uint32_t d = (key[r] >> shift) & mask;
    uint64_t peers = __ballot(live);                 // lanes of this round with my digit
#pragma unroll
    for (uint32_t b = 0; b < DENSE_RADIX_BITS; b++) {
      const bool bit = (d >> b) & 1u;
      const uint64_t m = __ballot(bit);
      peers &= bit ? m : ~m;
    }
    const uint32_t before = (uint32_t)__popcll(peers & below);
    rank[r] = live ? cnt[wv][d] + before : 0u;       // elements of this wave with digit d in earlier rounds + earlier lanes of this one
    __syncthreads();                                 // every lane has read the running count before its digit's first lane moves it on
    if (live && before == 0) cnt[wv][d] += (uint32_t)__popcll(peers);
    __syncthreads();
  }
  // per digit (one thread each): the waves' totals -> where each wave's elements of this digit start in the output
  {
    const uint32_t d = threadIdx.x;
    const size_t e = (size_t)d * ntiles + tile;
    uint32_t run = counts[e] + sums[e >> DENSE_SCAN_SHIFT];
#pragma unroll
    for (uint32_t w = 0; w < DENSE_WAVES; w++) { const uint32_t t = cnt[w][d]; cnt[w][d] = run; run += t; }
  }
  __syncthreads();
#pragma unroll
  for (uint32_t r = 0; r < DENSE_ITEMS; r++) {
    const uint32_t p = base + r * 64;
    if (p < n) {
      const uint32_t dst = cnt[wv][(key[r] >> shift) & mask] + rank[r];
      if (dst < n) { keys_out[dst] = key[r]; idx_out[dst] = pay[r]; }
    }
  }
}

// start[a] <- the sorted position of the first op on cell a (cells without an op keep whatever they hold: they are never read)
__global__ void __launch_bounds__(256) k_dense_bounds(const uint32_t* __restrict__ keys, uint32_t n, uint32_t cells, uint32_t* __restrict__ start) {
  for (uint32_t p = blockIdx.x * blockDim.x + threadIdx.x; p < n; p += gridDim.x * blockDim.x) {
    const uint32_t k = keys[p];
    if ((p == 0 || keys[p - 1] != k) && k < cells) start[k] = p;
  }
}
// read_ts[op] <- position - start of its run; audit_ts[cell] <- length of its run, written by the run's last op (audit_ts is zeroed before)
__global__ void __launch_bounds__(256) k_dense_rank(const uint32_t* __restrict__ keys, const uint32_t* __restrict__ idx, uint32_t n, uint32_t cells,
                                                    const uint32_t* __restrict__ start, uint32_t* __restrict__ read_ts, uint32_t* __restrict__ audit_ts) {
  for (uint32_t p = blockIdx.x * blockDim.x + threadIdx.x; p < n; p += gridDim.x * blockDim.x) {
    const uint32_t k = keys[p], op = idx[p];
    if (k >= cells || op >= n) continue;
    const uint32_t s = start[k];
    read_ts[op] = p - s;
    if (p + 1 == n || keys[p + 1] != k) audit_ts[k] = p + 1 - s;
  }
}

// comb_ops and comb_mem in the table representation, zero tails included, in one pass (sparse_mlpoly_full.rs:154-164, hyrax.rs:237-251).
//   u32s: row addr | row read_ts | col addr | col read_ts, batch * N entries each = the first 4 * batch * N entries of comb_ops (Scalar::from_u64);
//   then batch * N values (the staged triplet values through the conversion of k_fr_to_mont / k_fr_from_ark, zero from nnz[k] on), then zeros up to ops_len;
//   audit: row audit_ts | col audit_ts = comb_mem (mem_len = 2 * cells entries).
__global__ void __launch_bounds__(256) k_dense_tables(const uint32_t* __restrict__ u32s, const uint32_t* __restrict__ vals, DenseArgs a, uint32_t log_n, uint32_t batch,
                                                      int ark, const uint32_t* __restrict__ audit, size_t ops_len, size_t mem_len,
                                                      uint32_t* __restrict__ comb_ops, uint32_t* __restrict__ comb_mem) {
  const size_t ints = (size_t)4 * batch << log_n, live = (size_t)5 * batch << log_n;
  for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < ops_len + mem_len; e += (size_t)gridDim.x * blockDim.x) {
    Fr x = fe_zero<FrP>();
    uint32_t* dst;
    if (e < ops_len) {
      dst = comb_ops + 8 * e;
      if (e < ints) {
        const uint32_t v = u32s[e];
        if (v) x = fe_to_mont(fe_from_u64<FrP>(v));
      } else if (e < live) {
        const size_t q = e - ints;
        const uint32_t k = (uint32_t)(q >> log_n), i = (uint32_t)q & ((1u << log_n) - 1u);
        uint32_t off, nnz; dense_pick(a, k, off, nnz);
        if (i < nnz) {
          const Fr v = fe_gload<FrP>(vals + 8 * ((size_t)off + i));
          x = ark ? fe_from_ark_mont(v) : fe_to_mont(v);
        }
      }
    } else {
      dst = comb_mem + 8 * (e - ops_len);
      const uint32_t v = audit[e - ops_len];
      if (v) x = fe_to_mont(fe_from_u64<FrP>(v));
    }
    fe_gstore_tab<FrP>(dst, x);
  }
}

}  // namespace sbn
