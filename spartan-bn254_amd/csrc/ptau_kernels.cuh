// ptau_kernels.cuh — the kernel of a powers-of-tau file as the KZG SRS (abi_kzg_srs.inc: sbn_kzg_srs_load_ptau), one point per lane:
//   k_ptau_points    a chunk of the file's uncompressed G1 points (x | y, 32 B each, ark-ff's Montgomery limbs: v 2^256 mod q) -> the library's Montgomery
//                    affine points (v 2^261 mod q), written straight into the handle's d_pts exactly as k_srs_decompress writes them.
// A coordinate changes form with ONE field product by the constant 2^266 mod q (fe_from_ark_mont): no trip through canonical form.  The curve equation
// is tested in the library's form.  No square root, no inversion: a handful of products per point where k_srs_decompress spends about 380.
#pragma once
#include "fp.cuh"

namespace sbn {

// in: n x 64 bytes (16-byte aligned), the points first .. first + n of section 2; out: the handle's points from `first` on (16 words a point).
// Refused: a residue >= q, the all-zero point (the identity: no SRS holds one), y^2 != x^3 + 3.  A refused point is written as all-zero and
// *bad = min(*bad, first + i).
__global__ void __launch_bounds__(64) k_ptau_points(const uint32_t* __restrict__ in, size_t n, size_t first, uint32_t* __restrict__ out, unsigned long long* __restrict__ bad) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint4* p = reinterpret_cast<const uint4*>(in + 16 * i);
  const uint4 a = p[0], b = p[1], c = p[2], d = p[3];
  const uint32_t wx[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w}, wy[8] = {c.x, c.y, c.z, c.w, d.x, d.y, d.z, d.w};
  uint32_t any = 0;
#pragma unroll
  for (int k = 0; k < 8; k++) any |= wx[k] | wy[k];
  Fq xm = fe_zero<FqP>(), ym = xm;
  bool good = any != 0 && fe_is_canonical<FqP>(wx) && fe_is_canonical<FqP>(wy);
  if (good) {
    const Fq x = fe_from_ark_mont(fe_unpack<FqP>(wx)), y = fe_from_ark_mont(fe_unpack<FqP>(wy));      // in (-0.1 q, 1.1 q), normalised
    const Fq rhs = fe_add(fe_mul(fe_sqr(x), x), fe_to_mont(fe_small<FqP>(3u)));
    good = fe_eq(fe_sqr(y), rhs);
    if (good) { xm = fe_canon_small(x); ym = fe_canon_small(y); }
  }
  fe_store_packed<FqP>(out + 16 * (first + i), xm);
  fe_store_packed<FqP>(out + 16 * (first + i) + 8, ym);
  if (!good) atomicMin(bad, (unsigned long long)(first + i));
}

}  // namespace sbn
