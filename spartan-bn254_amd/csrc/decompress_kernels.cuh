// decompress_kernels.cuh — the kernels of the opening check (abi_polyeval_verify.inc):
//   k_g1_decompress         arkworks deserialize_compressed of a batch of G1 points (group.rs:323-329), one point per lane: the inverse of
//                           sbn_g1_compress.  32 bytes = x little-endian, bit 7 of byte 31 = "y is the larger root", bit 6 = identity.
//   k_polyeval_verify_row   the row -z1 * s of the verifier's folded equation, written straight from the lg n challenges
//                           (compute_s, bullet.rs:183-200), in the commit's input layout.
#pragma once
#include "polyeval_kernels.cuh"

namespace sbn {

// a^((p + 1) / 4): the square root of a residue for p = 3 mod 4 (both roots are +- this).  A fixed-exponent square-and-multiply, as fe_inv.
template <class M> __device__ __noinline__ Fe<M> fe_sqrt_3mod4(const Fe<M>& a) {
  uint32_t e[8];
  for (int i = 0; i < 8; i++) e[i] = modlimb<M>(i);
  e[0] += 1;                    // p0 = ...47 for Fq: no carry
  for (int i = 0; i < 8; i++) e[i] = (e[i] >> 2) | (i < 7 ? e[i + 1] << 30 : 0u);
  Fe<M> acc = fe_one<M>();
  for (int i = 253; i >= 0; i--) {
    acc = fe_sqr<M>(acc);
    if ((e[i >> 5] >> (i & 31)) & 1) acc = fe_mul<M>(acc, a);
  }
  return acc;
}

// in: n x 32 bytes.  ok[i] = 0: x >= p, or x^3 + 3 is not a square; the point is then written as all-zero.  The identity (bit 6) is the all-zero
// affine point with ok = 1, whatever the other bits hold.  out_canon: n x 64 canonical x || y, or null; out_mont: the same as Montgomery
// affine points (a generator table's layout, k_points_to_mont), or null.
__global__ void __launch_bounds__(64) k_g1_decompress(const uint32_t* __restrict__ in, size_t n, uint32_t* __restrict__ out_canon, uint32_t* __restrict__ out_mont,
                                                      uint8_t* __restrict__ ok) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint4 lo = reinterpret_cast<const uint4*>(in + 8 * i)[0], hi = reinterpret_cast<const uint4*>(in + 8 * i)[1];
  uint32_t w[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
  const uint32_t flags = w[7] >> 30;          // bit 0: identity, bit 1: the larger root
  w[7] &= 0x3fffffffu;
  const Fq zero = fe_zero<FqP>();
  Fq xc = zero, yc = zero;                    // canonical plain integers
  bool good = true, finite = false;
  if (!(flags & 1u)) {
    good = fe_is_canonical<FqP>(w);
    if (good) {
      xc = fe_unpack<FqP>(w);
      const Fq x = fe_to_mont(xc);
      const Fq rhs = fe_add(fe_mul(fe_sqr(x), x), fe_to_mont(fe_small<FqP>(3u)));
      const Fq y = fe_sqrt_3mod4(rhs);
      good = fe_eq(fe_sqr(y), rhs);
      if (good) {
        finite = true;
        yc = fe_from_mont(y);                 // in [0, p)
        Fq ny;                                // p - y
#pragma unroll
        for (int k = 0; k < NL; k++) ny.v[k] = p29<FqP>(k) - yc.v[k];
        ny = fe_norm(ny);
        const Fq d = fe_norm(fe_sub_lazy(ny, yc));
        const bool is_larger = (int32_t)d.v[NL - 1] < 0;         // y > p - y
        if (is_larger != ((flags & 2u) != 0)) yc = ny;
      } else xc = zero;
    }
  }
  ok[i] = good ? 1 : 0;
  if (out_canon) { fe_store_packed<FqP>(out_canon + 16 * i, xc); fe_store_packed<FqP>(out_canon + 16 * i + 8, yc); }
  if (out_mont) {
    fe_store_packed<FqP>(out_mont + 16 * i, finite ? fe_canon_small(fe_to_mont(xc)) : zero);
    fe_store_packed<FqP>(out_mont + 16 * i + 8, finite ? fe_canon_small(fe_to_mont(yc)) : zero);
  }
}

// row[j] = -z1 * s_j for j < n = 2^lg, s_j = prod_k (bit_{lg-1-k}(j) ? u_k : u_k^-1)  (bullet.rs:183-200: bit j of the index takes u[lg - 1 - j]);
// row[n] = tail (the scalar on gens_1.G[0]) and the blind behind the row — canonical words, as the commit cuts digits from them.
// U.l: the challenges, U.r: their inverses, nz1 = -z1: Montgomery form.
__global__ void __launch_bounds__(256) k_polyeval_verify_row(PolyEvalPoint U, int lg, ScScalar nz1, ScScalar tail, ScScalar blind, uint32_t* __restrict__ row, uint32_t* __restrict__ bl) {
  const size_t j = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const size_t n = (size_t)1 << lg;
  if (j < n) {
    Fr acc = fr_from_words(nz1);
#pragma unroll
    for (int k = 0; k < PE_SIDE_MAX; k++)
      if (k < lg) acc = fe_mul(acc, fe_unpack<FrP>(((j >> (lg - 1 - k)) & 1) ? U.l[k] : U.r[k]));
    fe_store_packed<FrP>(row + 8 * j, fe_from_mont(acc));
  }
  if (blockIdx.x == 0 && threadIdx.x >= 64 && threadIdx.x < 72) { const int k = threadIdx.x - 64; row[8 * n + k] = tail.v[k]; bl[k] = blind.v[k]; }
}

}  // namespace sbn
