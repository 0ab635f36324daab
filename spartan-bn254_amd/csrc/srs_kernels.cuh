// srs_kernels.cuh — the kernels of the KZG SRS file (abi_kzg_srs.inc), one point per lane in both directions:
//   k_srs_decompress    a chunk of the file's compressed powers -> Montgomery affine points, written straight into the handle's d_pts.  Nothing else is
//                       written per point: no canonical copy, no flag byte (k_g1_decompress keeps both for its callers, which read them on the host).
//                       A refused point lowers ONE 64-bit word to its index with atomicMin; the host reads that word once per chunk.
//   k_srs_compress      the handle's Montgomery affine points -> the file's 32 bytes a point, flag bits included (sbn_g1_compress on the device).
// The square root is decompress_kernels.cuh's fe_sqrt_3mod4 (a plain square-and-multiply over (q + 1)/4; no fixed-window form was built or measured).
#pragma once
#include "decompress_kernels.cuh"

namespace sbn {

// y > q - y for a canonical y (normalised limbs of a value in [0, q))
__device__ __forceinline__ bool srs_is_larger(const Fq& yc) {
  Fq ny;
#pragma unroll
  for (int k = 0; k < NL; k++) ny.v[k] = p29<FqP>(k) - yc.v[k];
  ny = fe_norm(ny);
  const Fq d = fe_norm(fe_sub_lazy(ny, yc));
  return (int32_t)d.v[NL - 1] < 0;
}

// in: n x 32 bytes (16-byte aligned), the points first .. first + n of the file; out: the handle's points from `first` on (16 words a point).
// Refused: x >= q, x^3 + 3 not a square, both flag bits, the identity (no SRS holds one, and every consumer divides by it in effect).  A refused point
// is written as all-zero and *bad = min(*bad, first + i).
__global__ void __launch_bounds__(64) k_srs_decompress(const uint32_t* __restrict__ in, size_t n, size_t first, uint32_t* __restrict__ out, unsigned long long* __restrict__ bad) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint4 lo = reinterpret_cast<const uint4*>(in + 8 * i)[0], hi = reinterpret_cast<const uint4*>(in + 8 * i)[1];
  uint32_t w[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
  const uint32_t flags = w[7] >> 30;          // bit 0: identity, bit 1: the larger root
  w[7] &= 0x3fffffffu;
  Fq xm = fe_zero<FqP>(), ym = xm;
  bool good = !(flags & 1u) && fe_is_canonical<FqP>(w);
  if (good) {
    const Fq x = fe_to_mont(fe_unpack<FqP>(w));
    const Fq rhs = fe_add(fe_mul(fe_sqr(x), x), fe_to_mont(fe_small<FqP>(3u)));
    const Fq y = fe_sqrt_3mod4(rhs);
    good = fe_eq(fe_sqr(y), rhs);
    if (good) {
      Fq yc = fe_from_mont(y);                  // in [0, q)
      if (srs_is_larger(yc) != ((flags & 2u) != 0)) {
#pragma unroll
        for (int k = 0; k < NL; k++) yc.v[k] = p29<FqP>(k) - yc.v[k];
        yc = fe_norm(yc);
      }
      xm = fe_canon_small(x);
      ym = fe_canon_small(fe_to_mont(yc));
    }
  }
  fe_store_packed<FqP>(out + 16 * (first + i), xm);
  fe_store_packed<FqP>(out + 16 * (first + i) + 8, ym);
  if (!good) atomicMin(bad, (unsigned long long)(first + i));
}

// in: the handle's points from `first` on; out: n x 32 bytes.  The all-zero point is the identity: 31 zero bytes and 0x40, as sbn_g1_compress writes it.
__global__ void __launch_bounds__(64) k_srs_compress(const uint32_t* __restrict__ in, size_t n, size_t first, uint32_t* __restrict__ out) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const Fq xc = fe_from_mont(fe_load<FqP>(in + 16 * (first + i))), yc = fe_from_mont(fe_load<FqP>(in + 16 * (first + i) + 8));
  uint32_t w[8];
  fe_pack<FqP>(xc, w);
  if (fe_is_zero_limbs(xc) && fe_is_zero_limbs(yc)) w[7] = 0x40000000u;
  else if (srs_is_larger(yc)) w[7] |= 0x80000000u;
  uint4* q = reinterpret_cast<uint4*>(out + 8 * i);
  q[0] = make_uint4(w[0], w[1], w[2], w[3]);
  q[1] = make_uint4(w[4], w[5], w[6], w[7]);
}

}  // namespace sbn
