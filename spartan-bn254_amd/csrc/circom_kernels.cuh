// circom_kernels.cuh — a circom .r1cs constraints section and a .wtns value section on the device (reference src/r1cs_reader.rs:131-242,
// examples/keyless_benchmark.rs:38-72).  The host has walked the 3 * nConstraints entry counts (circom_host.hpp: run_first, mat_first); everything
// per entry happens here, one lane per entry, in streaming passes.
//
// Reference loops replaced (serial on the host there, once per circuit):
//   read_constraints_section's three inner loops, bytes_to_scalar (r1cs_reader.rs:149-182, :286-299)   -> k_circom_entries
//   to_sparse_matrices_padded's remap_col (:224-235)                                                      -> k_circom_entries
//   the `if let Some(scalar)` that skips a value >= r (:156-158)                                          -> the keep flag, k_dense_scan / _scan_top, k_circom_compact
//   the two compressed copies sbn_r1cs_upload builds with counting sorts on the host (abi_r1cs.inc)      -> k_circom_gkeys, k_circom_ends, the radix passes of
//                                                                                                           dense_kernels.cuh on (column, position), k_circom_gather
//   parse_wtns's value loop (keyless_benchmark.rs:59-67)                                                 -> k_circom_wtns
//
// The payload of section 2 lies in a 256-byte-aligned buffer from its own first byte: a record starts at byte 4 (k + 1) + 36 g (k: its run, g: its number
// in file order), a multiple of four whatever the section's offset in the file was, so a record is nine aligned dwords: the wire, then eight value words.
#pragma once
#include "dense_kernels.cuh"

namespace sbn {

struct CircomArgs {
  uint32_t n_pub, n_wires, nv_padded;        // nPubOut + nPubIn, nWires, num_vars_padded
  uint32_t mat_off[3];                       // where matrix m's entries start in the staged arrays
};

// the run of entry g: the last k with run_first[k] <= g (runs without entries share their start with the next run and are passed over).
// run_first has nruns + 1 values, the last one the entry count
__device__ __forceinline__ uint32_t circom_run_of(const uint32_t* __restrict__ run_first, uint32_t nruns, uint32_t g) {
  uint32_t lo = 0, hi = nruns;               // the answer is in [lo, hi): run_first[lo] <= g < run_first[hi]
  while (hi - lo > 1) {
    const uint32_t mid = lo + ((hi - lo) >> 1);
    if (run_first[mid] <= g) lo = mid; else hi = mid;
  }
  return lo;
}

// One lane per entry.  out: {values >= r in A, in B, in C, the lowest entry (file order) whose wire is >= nWires}; the host sets {0, 0, 0, 0xffffffff}.
// Three atomicAdd (where non-zero) and one atomicMin a block.  A dropped entry still gets its slot (keep = 0): the compaction closes the gaps.
__global__ void __launch_bounds__(256) k_circom_entries(const uint32_t* __restrict__ payload, size_t payload_words, const uint32_t* __restrict__ run_first,
                                                        const uint32_t* __restrict__ mat_first, uint32_t nruns, uint32_t total, CircomArgs a,
                                                        uint32_t* __restrict__ rows, uint32_t* __restrict__ cols, uint32_t* __restrict__ vals,
                                                        uint32_t* __restrict__ keep, uint32_t* __restrict__ out) {
  uint32_t drop0 = 0, drop1 = 0, drop2 = 0, bad = 0xffffffffu;
  for (uint32_t g = blockIdx.x * blockDim.x + threadIdx.x; g < total; g += gridDim.x * blockDim.x) {
    const uint32_t k = circom_run_of(run_first, nruns, g);
    const uint32_t m = k % 3u, i = k / 3u, e = g - run_first[k];
    const size_t w = (size_t)k + 1 + (size_t)9 * g;                 // dword index of the record: byte 4 (k + 1) + 36 g
    if (w + 9 > payload_words) continue;                            // (the host's walk has checked every record against the section's end)
    const uint32_t wire = payload[w];
    uint32_t v[8];
#pragma unroll
    for (int j = 0; j < 8; j++) v[j] = payload[w + 1 + j];
    const bool ok = fe_is_canonical<FrP>(v);                        // bytes_to_scalar -> None: the reader skips the entry (r1cs_reader.rs:156-158)
    if (!ok) { drop0 += m == 0; drop1 += m == 1; drop2 += m == 2; }
    if (ok && wire >= a.n_wires) bad = min(bad, g);                 // the reference aliases such a wire onto another column
    const uint32_t col = wire == 0 ? a.nv_padded : (wire <= a.n_pub ? a.nv_padded + wire : wire - a.n_pub - 1);      // remap_col, :224-235
    const uint32_t off = m == 0 ? a.mat_off[0] : (m == 1 ? a.mat_off[1] : a.mat_off[2]);
    const size_t dst = (size_t)off + mat_first[k] + e;
    if (dst >= total) continue;
    rows[dst] = i; cols[dst] = col; keep[dst] = ok ? 1u : 0u;
#pragma unroll
    for (int j = 0; j < 8; j++) vals[8 * dst + j] = v[j];
  }
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    drop0 += __shfl_down(drop0, d); drop1 += __shfl_down(drop1, d); drop2 += __shfl_down(drop2, d);
    bad = min(bad, (uint32_t)__shfl_down(bad, d));
  }
  __shared__ uint32_t sm[4][4];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  if (lane == 0) { sm[0][wv] = drop0; sm[1][wv] = drop1; sm[2][wv] = drop2; sm[3][wv] = bad; }
  __syncthreads();
  if (threadIdx.x < 3) {
    const uint32_t s = sm[threadIdx.x][0] + sm[threadIdx.x][1] + sm[threadIdx.x][2] + sm[threadIdx.x][3];
    if (s) atomicAdd(out + threadIdx.x, s);
  } else if (threadIdx.x == 3) {
    const uint32_t b = min(min(sm[3][0], sm[3][1]), min(sm[3][2], sm[3][3]));
    if (b != 0xffffffffu) atomicMin(out + 3, b);
  }
}

// stable compaction: entry e with keep[e] goes to scan[e] + sums[e >> DENSE_SCAN_SHIFT] (k_dense_scan over a copy of keep, k_dense_scan_top over its sums)
__global__ void __launch_bounds__(256) k_circom_compact(const uint32_t* __restrict__ keep, const uint32_t* __restrict__ scan, const uint32_t* __restrict__ sums, uint32_t n,
                                                        uint32_t n_out, const uint32_t* __restrict__ rows, const uint32_t* __restrict__ cols, const uint32_t* __restrict__ vals,
                                                        uint32_t* __restrict__ rows_out, uint32_t* __restrict__ cols_out, uint32_t* __restrict__ vals_out) {
  for (uint32_t e = blockIdx.x * blockDim.x + threadIdx.x; e < n; e += gridDim.x * blockDim.x) {
    if (!keep[e]) continue;
    const uint32_t dst = scan[e] + sums[e >> DENSE_SCAN_SHIFT];
    if (dst >= n_out) continue;
    rows_out[dst] = rows[e]; cols_out[dst] = cols[e];
#pragma unroll
    for (int j = 0; j < 8; j++) vals_out[8 * (size_t)dst + j] = vals[8 * (size_t)e + j];
  }
}

// gkey[p] <- m * num_cons + row of staged entry p: its row in [A; B; C], and the index the column-major copy gathers with
__global__ void __launch_bounds__(256) k_circom_gkeys(const uint32_t* __restrict__ rows, uint32_t n, uint32_t off1, uint32_t off2, uint32_t num_cons, uint32_t* __restrict__ gkey) {
  for (uint32_t p = blockIdx.x * blockDim.x + threadIdx.x; p < n; p += gridDim.x * blockDim.x)
    gkey[p] = ((p >= off1 ? 1u : 0u) + (p >= off2 ? 1u : 0u)) * num_cons + rows[p];
}

// ends[j] <- the number of keys <= j, for j < nrows, over n ascending keys: row_end of a compressed copy.  One lane per row, a binary search each
__global__ void __launch_bounds__(256) k_circom_ends(const uint32_t* __restrict__ keys, uint32_t n, uint32_t nrows, uint32_t* __restrict__ ends) {
  for (uint32_t j = blockIdx.x * blockDim.x + threadIdx.x; j < nrows; j += gridDim.x * blockDim.x) {
    uint32_t lo = 0, hi = n;                   // keys[< lo] <= j < keys[>= hi]
    while (lo < hi) {
      const uint32_t mid = lo + ((hi - lo) >> 1);
      if (keys[mid] <= j) lo = mid + 1; else hi = mid;
    }
    ends[j] = lo;
  }
}

// the column-major copy behind the sort: idx[q] <- gkey[pos[q]], val[q] <- the canonical value of staged entry pos[q] (k_fr_to_mont follows in place)
__global__ void __launch_bounds__(256) k_circom_gather(const uint32_t* __restrict__ pos, const uint32_t* __restrict__ gkey, const uint32_t* __restrict__ vals, uint32_t n,
                                                       uint32_t* __restrict__ idx, uint32_t* __restrict__ val) {
  for (uint32_t q = blockIdx.x * blockDim.x + threadIdx.x; q < n; q += gridDim.x * blockDim.x) {
    const uint32_t p = pos[q];
    if (p >= n) continue;
    idx[q] = gkey[p];
#pragma unroll
    for (int j = 0; j < 8; j++) val[8 * (size_t)q + j] = vals[8 * (size_t)p + j];
  }
}

// witness values [0, first + len): each one there is (j < count) is tested against r — *bad <- the lowest index of a value >= r (the host sets
// 0xffffffff) — and table[j - first] <- the value in the table representation for j >= first, zero behind the file's last value
__global__ void __launch_bounds__(256) k_circom_wtns(const uint32_t* __restrict__ src, uint32_t count, uint32_t first, uint32_t len, uint32_t* __restrict__ table,
                                                     uint32_t* __restrict__ bad) {
  for (uint32_t j = blockIdx.x * blockDim.x + threadIdx.x; j < first + len; j += gridDim.x * blockDim.x) {
    Fr x = fe_zero<FrP>();
    if (j < count) {
      uint32_t v[8];
#pragma unroll
      for (int t = 0; t < 8; t++) v[t] = src[8 * (size_t)j + t];
      if (!fe_is_canonical<FrP>(v)) { atomicMin(bad, j); continue; }      // (rare: a witness circom wrote has none)
      if (j >= first) x = fe_to_mont(fe_load<FrP>(src + 8 * (size_t)j));
    }
    if (j >= first) fe_store_tab<FrP>(table + 8 * (size_t)(j - first), x);
  }
}

// ---- the circuit digest's leaves (circom_host.hpp: the definition): leaf(m, j) = SHAKE256(header | k x (u32le row | u32le col | val[32]))[0..32] over
// entries 128 j .. 128 j + k - 1 of matrix m.  One lane a leaf, one wave a block: a leaf is 38 dependent permutations and nothing of it is shared, so
// the lanes of a wave walk their leaves block by block in step.
// The message is read as dwords.  The header has 39 bytes, so one zero byte is put in front of it: in the stream V = 0 | header | entries the header
// fills words 0 .. 9 and entry e words 10 + 10 e .. (row, col, eight value words: exactly what rows / cols / vals hold), and message word n is
// (V[n] >> 8) | (V[n + 1] << 24).  A block of the rate (136 B = 34 words) is therefore 35 loads whose REGISTER index is fixed and whose ADDRESS moves:
// the state and the block stay in registers under static indices (no scratch), and the position inside the entry is address arithmetic.  A lane's
// loads walk its own 5 KiB, 4 B a time: each line is fetched once and re-read from L1 / L2 (64 lanes x 128 B live a wave); against the ~8 k ALU
// instructions of one permutation the 35 loads a block are a few per cent of the time (DESIGN 4.25 has the measured figure).
struct CircomDigestArgs {
  uint32_t head[7];                          // V[0 .. 6] of a leaf: the zero byte, the 26 bytes of the domain string, a zero byte where m goes
  uint32_t off[3], nnz[3];                   // where matrix m's entries start in rows / cols / vals, and how many there are
  uint32_t leaf_first[3], leaves;            // the leaves of matrix m are leaf_first[m] .. ; leaves: all of them
};
static const int DIGEST_LEAF = 128;          // entries a leaf
static const int DIGEST_RATE_WORDS = 34;     // SHAKE256: 136 bytes

// Keccak-f[1600] (FIPS 202 3.2-3.4) on 25 lanes in registers; rho and pi folded into one table of fixed rotations, chi row by row
__device__ __forceinline__ uint64_t keccak_rol(uint64_t x, int n) { return n ? (x << n) | (x >> (64 - n)) : x; }
__device__ __forceinline__ void keccak_f1600(uint64_t (&a)[25]) {
  static constexpr uint64_t RC[24] = {
    0x0000000000000001ull, 0x0000000000008082ull, 0x800000000000808aull, 0x8000000080008000ull, 0x000000000000808bull, 0x0000000080000001ull,
    0x8000000080008081ull, 0x8000000000008009ull, 0x000000000000008aull, 0x0000000000000088ull, 0x0000000080008009ull, 0x000000008000000aull,
    0x000000008000808bull, 0x800000000000008bull, 0x8000000000008089ull, 0x8000000000008003ull, 0x8000000000008002ull, 0x8000000000000080ull,
    0x000000000000800aull, 0x800000008000000aull, 0x8000000080008081ull, 0x8000000000008080ull, 0x0000000080000001ull, 0x8000000080008008ull};
  // rho offset of lane x + 5 y
  constexpr int RHO[25] = {0, 1, 62, 28, 27, 36, 44, 6, 55, 20, 3, 10, 43, 25, 39, 41, 45, 15, 21, 8, 18, 2, 61, 56, 14};
#pragma unroll 1
  for (int r = 0; r < 24; r++) {
    uint64_t C[5], B[25];
#pragma unroll
    for (int x = 0; x < 5; x++) C[x] = a[x] ^ a[x + 5] ^ a[x + 10] ^ a[x + 15] ^ a[x + 20];
#pragma unroll
    for (int x = 0; x < 5; x++) {
      const uint64_t D = C[(x + 4) % 5] ^ keccak_rol(C[(x + 1) % 5], 1);
#pragma unroll
      for (int y = 0; y < 5; y++) a[x + 5 * y] ^= D;
    }
#pragma unroll
    for (int x = 0; x < 5; x++)
#pragma unroll
      for (int y = 0; y < 5; y++) B[y + 5 * ((2 * x + 3 * y) % 5)] = keccak_rol(a[x + 5 * y], RHO[x + 5 * y]);      // pi after rho
#pragma unroll
    for (int y = 0; y < 5; y++)
#pragma unroll
      for (int x = 0; x < 5; x++) a[x + 5 * y] = B[x + 5 * y] ^ (~B[(x + 1) % 5 + 5 * y] & B[(x + 2) % 5 + 5 * y]);
    a[0] ^= RC[r];
  }
}

__global__ void __launch_bounds__(64) k_circom_digest_leaves(const uint32_t* __restrict__ rows, const uint32_t* __restrict__ cols, const uint32_t* __restrict__ vals,
                                                             size_t total, CircomDigestArgs A, uint64_t* __restrict__ out) {
  const uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= A.leaves) return;
  const uint32_t m = (g >= A.leaf_first[1] ? 1u : 0u) + (g >= A.leaf_first[2] ? 1u : 0u);
  const uint32_t first = m == 0 ? A.leaf_first[0] : (m == 1 ? A.leaf_first[1] : A.leaf_first[2]);
  const uint32_t nnz = m == 0 ? A.nnz[0] : (m == 1 ? A.nnz[1] : A.nnz[2]);
  const uint32_t off = m == 0 ? A.off[0] : (m == 1 ? A.off[1] : A.off[2]);
  const uint32_t j = g - first;
  // this guard and the one on e0 + k keep every read inside the arrays; sbn_circom_r1cs_digest checks off[m] + nnz[m] <= total before the launch and
  // derives the leaf counts from the same nnz, so neither fires and every lane below `leaves` writes its 32 bytes
  if ((uint64_t)j * DIGEST_LEAF >= nnz) return;
  const uint32_t k = min((uint32_t)DIGEST_LEAF, nnz - j * DIGEST_LEAF);
  const size_t e0 = (size_t)off + (size_t)j * DIGEST_LEAF;           // the leaf's first entry; e0 + k <= off + nnz <= total
  if (e0 + k > total) return;
  const uint32_t vwords = 10u + 10u * k;                             // the words of V that exist; behind them the stream is zero
  const uint32_t len = 39u + 40u * k;                                // the message's bytes
  const uint32_t nblocks = len / 136u + 1u;                          // pad10*1 always adds at least one byte
  const uint32_t pad_word = len >> 2, pad_val = 0x1fu << (8u * (len & 3u));
  uint32_t head[10];
#pragma unroll
  for (int i = 0; i < 7; i++) head[i] = A.head[i];
  head[6] |= m << 24; head[7] = j; head[8] = 0u; head[9] = k;        // u8 m | u64le j | u32le k
  uint64_t a[25];
#pragma unroll
  for (int i = 0; i < 25; i++) a[i] = 0;
  for (uint32_t b = 0; b < nblocks; b++) {
    const uint32_t w0 = b * DIGEST_RATE_WORDS;                       // the block's first message word
    uint32_t v[DIGEST_RATE_WORDS + 1];
#pragma unroll
    for (int i = 0; i <= DIGEST_RATE_WORDS; i++) {
      const uint32_t n = w0 + i;
      uint32_t x = 0;
      if (i < 10 && b == 0) x = head[i];
      else if (n < vwords) {
        const uint32_t t = n - 10u, e = t / 10u, f = t - 10u * e;
        x = f == 0 ? rows[e0 + e] : (f == 1 ? cols[e0 + e] : vals[8 * (e0 + e) + (f - 2u)]);
      }
      v[i] = x;
    }
#pragma unroll
    for (int i = 0; i < DIGEST_RATE_WORDS; i += 2) {
      uint32_t lo = (v[i] >> 8) | (v[i + 1] << 24), hi = (v[i + 1] >> 8) | (v[i + 2] << 24);
      if (w0 + i == pad_word) lo ^= pad_val;
      if (w0 + i + 1 == pad_word) hi ^= pad_val;
      if (i == DIGEST_RATE_WORDS - 2 && b == nblocks - 1) hi ^= 0x80000000u;      // the last bit of pad10*1, in the last byte of the rate
      a[i >> 1] ^= (uint64_t)lo | ((uint64_t)hi << 32);
    }
    keccak_f1600(a);
  }
#pragma unroll
  for (int i = 0; i < 4; i++) out[4 * (size_t)g + i] = a[i];
}

}  // namespace sbn
