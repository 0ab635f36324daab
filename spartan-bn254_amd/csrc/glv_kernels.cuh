// glv_kernels.cuh — the GLV endomorphism of BN254 G1 for single MSMs.
//
// phi(x, y) = (beta * x, y) = lambda * P for every P in G1 (beta^3 = 1 mod p, lambda^3 = 1 mod r).  A scalar k < r is split as
// k = k1 + lambda * k2 (mod r) with 0 <= k1, k2 < 2^127, so that sum k_i P_i = sum k1_i P_i + k2_i phi(P_i): an MSM of 2n points whose
// scalars are 127 bits wide (8 windows of 16 bits instead of 17 of 15 at 2^20).
//
// The split is Babai's with FLOOR instead of rounding (the "shifted" decomposition).  The short lattice basis of
// {(a, b) : a + lambda b = 0 mod r} from extended Euclid on (r, lambda) is v1 = (A, -B), v2 = (B, C) (A, C: 127 bits, B: 64 bits,
// A C + B^2 = r).  With c1 = floor(k C / r), c2 = floor(k B / r):
//   k1 = k - c1 A - c2 B,   k2 = c1 B - c2 C          (k1, k2) = f1 v1 + f2 v2 with f1, f2 in [0, 1)
// so k1 in [0, A + B) and k2 in (-B, C); a negative k2 takes the lattice vector v2 once more: (k1 + B, k2 + C), in [0, A + 2B) x [0, C).
// Both bounds are below 0x6f4e * 2^112: the top 16-bit window of either half never reaches 2^15 and the signed recoding never carries
// out of it (tests/test_glv_cpu.py re-derives the basis and the bounds with exact integers).
// c1, c2 come from the precomputed g = floor(2^256 C / r), floor(2^256 B / r): (k g) >> 256 is the exact floor or one less, and the
// remainder k C - c r (exact modulo 2^256, it lies in [0, 2r)) decides the correction.
#pragma once
#include "msm_kernels.cuh"

namespace sbn {

namespace glv {
constexpr uint64_t A[2] = {0x8211bbeb7d4f1128ull, 0x6f4d8248eeb859fcull};
constexpr uint64_t B = 0x89d3256894d213e3ull;
constexpr uint64_t C[2] = {0x0be4e1541221250bull, 0x6f4d8248eeb859fdull};
constexpr uint64_t G1[3] = {0x5398fd0300ff6565ull, 0x4ccef014a773d2d2ull, 0x2ull};      // floor(2^256 C / r)
constexpr uint64_t G2[2] = {0xd91d232ec7e0b3d7ull, 0x2ull};                             // floor(2^256 B / r)
constexpr uint64_t R[4] = {0x43e1f593f0000001ull, 0x2833e84879b97091ull, 0xb85045b68181585dull, 0x30644e72e131a029ull};
// beta (canonical, little-endian 32-bit words): the cube root of unity in Fq with phi(P) = lambda P for
// lambda = 0x30644e72e131a029048b6e193fd84104cc37a73fec2bc5e9b8ca0b2d36636f23
constexpr uint32_t BETA[8] = {0x607cfd48u, 0xe4bd44e5u, 0xbb966e3du, 0xc28f069fu, 0xe0acccb0u, 0x5e6dd9e7u, 0xe131a029u, 0x30644e72u};
}  // namespace glv

// out[0 .. NA+NB) = a * b (schoolbook on 64-bit limbs)
template <int NA, int NB>
__device__ __forceinline__ void glv_mul(const uint64_t (&a)[NA], const uint64_t (&b)[NB], uint64_t (&out)[NA + NB]) {
#pragma unroll
  for (int i = 0; i < NA + NB; i++) out[i] = 0;
#pragma unroll
  for (int i = 0; i < NA; i++) {
    uint64_t carry = 0;
#pragma unroll
    for (int j = 0; j < NB; j++) {
      const uint64_t lo = a[i] * b[j], hi = __umul64hi(a[i], b[j]);
      uint64_t s = out[i + j] + lo; uint64_t cy = s < lo ? 1 : 0;
      s += carry; cy += s < carry ? 1 : 0;
      out[i + j] = s; carry = hi + cy;
    }
    out[i + NB] = carry;
  }
}
// the low 4 limbs of a * b (a: 4 limbs, b: NB <= 4 limbs)
template <int NB>
__device__ __forceinline__ void glv_mul_lo256(const uint64_t (&a)[4], const uint64_t (&b)[NB], uint64_t (&out)[4]) {
#pragma unroll
  for (int i = 0; i < 4; i++) out[i] = 0;
#pragma unroll
  for (int i = 0; i < 4; i++) {
    uint64_t carry = 0;
#pragma unroll
    for (int j = 0; j < NB && i + j < 4; j++) {
      const uint64_t lo = a[i] * b[j], hi = __umul64hi(a[i], b[j]);
      uint64_t s = out[i + j] + lo; uint64_t cy = s < lo ? 1 : 0;
      s += carry; cy += s < carry ? 1 : 0;
      out[i + j] = s; carry = hi + cy;
    }
    if (i + NB < 4) out[i + NB] = carry;
  }
}
// (x - y) mod 2^256 >= r ?
__device__ __forceinline__ bool glv_diff_ge_r(const uint64_t (&x)[4], const uint64_t (&y)[4]) {
  uint64_t d[4], borrow = 0;
#pragma unroll
  for (int i = 0; i < 4; i++) { const uint64_t t = x[i] - y[i]; const uint64_t b1 = x[i] < y[i]; d[i] = t - borrow; borrow = b1 | (t < borrow); }
#pragma unroll
  for (int i = 3; i >= 0; i--) { if (d[i] != glv::R[i]) return d[i] > glv::R[i]; }
  return true;
}
// 128-bit helpers (lo, hi)
__device__ __forceinline__ void u128_mul_lo(uint64_t a0, uint64_t a1, uint64_t b0, uint64_t b1, uint64_t& o0, uint64_t& o1) {
  o0 = a0 * b0; o1 = __umul64hi(a0, b0) + a0 * b1 + a1 * b0;
}
__device__ __forceinline__ void u128_add(uint64_t& x0, uint64_t& x1, uint64_t y0, uint64_t y1) { const uint64_t s = x0 + y0; x1 += y1 + (s < x0 ? 1 : 0); x0 = s; }
__device__ __forceinline__ void u128_sub(uint64_t& x0, uint64_t& x1, uint64_t y0, uint64_t y1) { const uint64_t b = x0 < y0 ? 1 : 0; x0 -= y0; x1 -= y1 + b; }

// k (canonical, 4 limbs) -> (k1, k2), both in [0, 2^127)
__device__ __forceinline__ void glv_split(const uint64_t (&k)[4], uint64_t (&k1)[2], uint64_t (&k2)[2]) {
  uint64_t p1[7], p2[6];
  glv_mul<4, 3>(k, glv::G1, p1);
  glv_mul<4, 2>(k, glv::G2, p2);
  uint64_t c1[2] = {p1[4], p1[5]}, c2[1] = {p2[4]};                   // c1 < C < 2^127, c2 < B < 2^64
  {
    uint64_t kc[4], cr[4];
    glv_mul_lo256<2>(k, glv::C, kc);
    const uint64_t c1v[4] = {c1[0], c1[1], 0, 0};
    glv_mul_lo256<4>(c1v, glv::R, cr);
    if (glv_diff_ge_r(kc, cr)) { if (++c1[0] == 0) ++c1[1]; }
  }
  {
    uint64_t kb[4], cr[4];
    const uint64_t bb[1] = {glv::B};
    glv_mul_lo256<1>(k, bb, kb);
    const uint64_t c2v[4] = {c2[0], 0, 0, 0};
    glv_mul_lo256<4>(c2v, glv::R, cr);
    if (glv_diff_ge_r(kb, cr)) ++c2[0];
  }
  // modulo 2^128: the exact values are in [0, A + B) and (-B, C)
  uint64_t x0 = k[0], x1 = k[1], t0, t1;
  u128_mul_lo(c1[0], c1[1], glv::A[0], glv::A[1], t0, t1); u128_sub(x0, x1, t0, t1);
  u128_mul_lo(c2[0], 0, glv::B, 0, t0, t1); u128_sub(x0, x1, t0, t1);
  uint64_t y0, y1;
  u128_mul_lo(c1[0], c1[1], glv::B, 0, y0, y1);
  u128_mul_lo(c2[0], 0, glv::C[0], glv::C[1], t0, t1); u128_sub(y0, y1, t0, t1);
  if (y1 >> 63) { u128_add(x0, x1, glv::B, 0); u128_add(y0, y1, glv::C[0], glv::C[1]); }
  k1[0] = x0; k1[1] = x1; k2[0] = y0; k2[1] = y1;
}

// n canonical 32-byte scalars -> 2n 16-byte sub-scalars: record i = k1_i, record n + i = k2_i (the digit kernels of the two-level
// sort read 16-byte records: k_s2_count / k_s2_scatter<C, SPT, 4>).  Scalars >= r are counted in *bad (SBN_EINVAL, as on the plain
// path) and split as zero.
__global__ void __launch_bounds__(256) k_glv_split(const uint32_t* __restrict__ scalars, size_t n, uint32_t* __restrict__ out, uint32_t* __restrict__ bad) {
  wave_prio_helper();
  const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n) return;
  const uint4 a = reinterpret_cast<const uint4*>(scalars + 8 * t)[0], b = reinterpret_cast<const uint4*>(scalars + 8 * t)[1];
  const uint32_t kk[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
  uint64_t k1[2] = {0, 0}, k2[2] = {0, 0};
  if (!fe_is_canonical<FrP>(kk)) atomicAdd(bad, 1u);
  else {
    const uint64_t k[4] = {(uint64_t)a.x | ((uint64_t)a.y << 32), (uint64_t)a.z | ((uint64_t)a.w << 32), (uint64_t)b.x | ((uint64_t)b.y << 32), (uint64_t)b.z | ((uint64_t)b.w << 32)};
    glv_split(k, k1, k2);
  }
  uint4* o = reinterpret_cast<uint4*>(out);
  o[t] = make_uint4((uint32_t)k1[0], (uint32_t)(k1[0] >> 32), (uint32_t)k1[1], (uint32_t)(k1[1] >> 32));
  o[n + t] = make_uint4((uint32_t)k2[0], (uint32_t)(k2[0] >> 32), (uint32_t)k2[1], (uint32_t)(k2[1] >> 32));
}

// the GLV base table of a generator set: npts points as they are, then their images phi(P_j) = (beta x_j, y_j); infinity stays (0, 0)
__global__ void __launch_bounds__(256) k_glv_table(const uint32_t* __restrict__ pts, size_t npts, uint32_t* __restrict__ out) {
  const size_t j = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= npts) return;
  const uint4* s = reinterpret_cast<const uint4*>(pts + 16 * j);
  uint4* d0 = reinterpret_cast<uint4*>(out + 16 * j);
  uint4* d1 = reinterpret_cast<uint4*>(out + 16 * (npts + j));
  const uint4 w0 = s[0], w1 = s[1], w2 = s[2], w3 = s[3];
  d0[0] = w0; d0[1] = w1; d0[2] = w2; d0[3] = w3;
  const Fq beta = fe_to_mont(fe_unpack<FqP>(glv::BETA));
  const Fq x = fe_load<FqP>(pts + 16 * j);
  fe_store<FqP>(out + 16 * (npts + j), fe_mul(x, beta));
  d1[2] = w2; d1[3] = w3;
}

}  // namespace sbn
