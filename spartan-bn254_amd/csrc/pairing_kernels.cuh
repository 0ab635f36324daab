// pairing_kernels.cuh — products of BN254 optimal-ate pairings, one WAVE per product (abi_pairing.inc: sbn_pairing_products, sbn_kzg_verify*).
// Stands in for Bn254::pairing / multi_pairing of ark-bn254 at the reference's two verifier call sites (kzg.rs:212-216, sparse_mlpoly_full.rs:552-595).
//   k_pairing_products   block c (64 lanes) computes  prod_t e(P_t, Q_t)  over at most four terms: the Miller loops share one accumulator f (one
//                        Fq12 squaring per doubling step, one line product per term and line), the lines come from the tables pairing_host.hpp
//                        built once per G2 point, and the EXACT final exponentiation (q^12 - 1)/r follows; out: f == 1, and the 384 GT bytes.
// Fq12 = Fq2[w]/(w^6 - xi), six Fq2 coefficients, held in LDS as 12 canonical Fq values (fp.cuh limbs, Montgomery R = 2^261).  The arithmetic is
// one dependent chain of ~600 Fq12 products, so the PRODUCT is what the wave's lanes share (f12_mul):
//   c_k = sum_{i <= k} a_i b_(k-i) + sum_{i > k} a_i (xi b)_(k+6-i):   12 output Fq coefficients, 12 Fq products each.
//   lanes 0..5 write b_j, -b_j.c1, xi b_j, -(xi b_j).c1 to LDS (additions only: xi = 9 + u);
//   quad q = 2k + part owns output coefficient (k, part); each of its 4 lanes accumulates 3 of the 12 products unreduced (cols_mac), carries its
//   columns, the quad adds its four column sets, and lane 0 of the quad runs the ONE Montgomery reduction (cols_reduce) and canonicalises.
// 3 x 81 + 90 multiplier instructions a lane and product.  A squaring and a product by a (sparse) line are the same routine: with the products
// dealt out over the lanes a sparse operand would shorten the longest lane's work from three products to two, and the code stays one routine.
// Value ranges: a canonical (< p); b_j < p, -b_j.c1 = 2p - b < 2p + 1, (xi b).c0 = 9x - y + 2p < 11p, (xi b).c1 = x + 9y < 10p, its negation
// 11p - . <= 11p: a sum of 12 products is below 132 p^2, the reduction returns below 132 p / 169 + p < 2p (R / p = 169), fe_canon_small's range.
// The final exponentiation is a PROGRAM of register-free steps over LDS slots (mul, Frobenius, conjugate, the one Fq inversion), generated with
// the constants by tools/gen_pairing_consts.py, which also states it in Python for the model to check (tests/test_pairing_model_cpu.py):
//   easy part  f^((q^6 - 1)(q^2 + 1)) with 1/f = f^(q + ... + q^11) / N(f), N(f) in Fq;
//   hard part  (q^4 - q^2 + 1)/r = l0 + l1 q + l2 q^2 + q^3 exactly (l_i polynomials in u: three powers by u and the chain of Scott et al.).
// Lanes exchange data through LDS only, ordered by __syncthreads(): one wave, so a barrier is cheap, and nothing relies on lock-step.
#pragma once
#include "fp.cuh"

namespace sbn {

#include "pairing_consts.inc"

constexpr int PAIR_TERMS_MAX = 4;
constexpr int F12_WORDS = 12 * NL;                       // 108
constexpr int PAIR_SLOTS = 10;                           // slots of the final exponentiation's program; slot 0 is the accumulator
constexpr int PAIR_LINE_OFF = PAIR_SLOTS * F12_WORDS;    // the current line as a full Fq12 value: only coefficients 0, 2, 3, 6, 7 are ever non-zero
constexpr int PAIR_T_OFF = PAIR_LINE_OFF + F12_WORDS;    // f12_mul's operand table: 12 x 3 values
constexpr int PAIR_P_OFF = PAIR_T_OFF + 36 * NL;         // the terms' points: 4 x (x, y)
constexpr int PAIR_LDS_WORDS = PAIR_P_OFF + 2 * PAIR_TERMS_MAX * NL;
constexpr int PAIR_LINE_BYTES = 128;
enum { PAIR_OP_MUL = 0, PAIR_OP_FROB = 1, PAIR_OP_CONJ = 2, PAIR_OP_INV = 3 };

// one check: its terms' points (device Montgomery form, 8 words a coordinate) and line tables
struct alignas(16) PairCheck {
  uint32_t count, pad[3];
  const uint8_t* lines[PAIR_TERMS_MAX];
  uint32_t p[PAIR_TERMS_MAX][16];
};

__device__ const uint32_t PAIR_FROB[12][2][NL] = SBN_PAIRING_FROB_ROWS;
__device__ const uint32_t PAIR_QM2[8] = {FqP::P0 - 2, FqP::P1, FqP::P2, FqP::P3, FqP::P4, FqP::P5, FqP::P6, FqP::P7};      // q - 2: Fermat's exponent
__device__ const uint16_t PAIR_FINAL_EXP[SBN_PAIRING_FINAL_EXP_LEN] = SBN_PAIRING_FINAL_EXP;

__device__ __forceinline__ Fq lds_fe(const uint32_t* p) { Fq r;
#pragma unroll
  for (int i = 0; i < NL; i++) r.v[i] = p[i];
  return r; }
__device__ __forceinline__ void lds_fe_store(uint32_t* p, const Fq& a) {
#pragma unroll
  for (int i = 0; i < NL; i++) p[i] = a.v[i];
}
// 9 a of a normalised non-negative a, normalised
__device__ __forceinline__ Fq fe_nine(const Fq& a) {
  Fq t;
#pragma unroll
  for (int i = 0; i < NL; i++) t.v[i] = a.v[i] << 2;
  t = fe_normu<FqP>(t);
  return fe_normu<FqP>(fe_add_lazy<FqP>(fe_dbl_lazy<FqP>(t), a));
}

// S[dst] = S[a] * S[b] in Fq12; dst, a, b: word offsets of slots, any of them equal.  All 64 lanes call it; the operands are complete (a barrier
// lies behind whatever wrote them) and the result is complete on return.
__device__ __forceinline__ void f12_mul(uint32_t* S, int dst, int a, int b, int lane) {
  uint32_t* T = S + PAIR_T_OFF;
  if (lane < 6) {
    const Fq x = lds_fe(S + b + (2 * lane) * NL), y = lds_fe(S + b + (2 * lane + 1) * NL);
    const Fq wx = fe_normu<FqP>(fe_subb<FqP, 2, 1>(fe_nine(x), y));                  // 9x - y + 2p
    const Fq wy = fe_normu<FqP>(fe_add_lazy<FqP>(x, fe_nine(y)));                    // x + 9y
    lds_fe_store(T + (3 * lane + 0) * NL, x);
    lds_fe_store(T + (3 * lane + 1) * NL, y);
    lds_fe_store(T + (3 * lane + 2) * NL, fe_normu<FqP>(fe_negb<FqP, 2>(y)));
    lds_fe_store(T + (3 * (6 + lane) + 0) * NL, wx);
    lds_fe_store(T + (3 * (6 + lane) + 1) * NL, wy);
    lds_fe_store(T + (3 * (6 + lane) + 2) * NL, fe_normu<FqP>(fe_negb<FqP, 11>(wy)));
  }
  __syncthreads();
  const int q = min(lane >> 2, 11), r = lane & 3, k = q >> 1, part = q & 1;          // lanes 48..63 repeat quad 11 and store nothing
  Cols s; cols_zero(s);
#pragma unroll 1
  for (int u = 0; u < 3; u++) {
    const int t = 3 * r + u, i = t >> 1, h = t & 1;
    const int j = i <= k ? k - i : 12 + k - i;                                         // b_(k-i), or (xi b)_(k+6-i) at table row 6 + (k+6-i)
    const int sel = part ? (h ? 0 : 1) : (h ? 2 : 0);                                  // re: a0 B0 + a1 (-B1);  im: a0 B1 + a1 B0
    const Fq A = lds_fe(S + a + (2 * i + h) * NL), B = lds_fe(T + (3 * j + sel) * NL);
    cols_mac<FqP>(s, A, B);
  }
  cols_carry(s);                                                                        // columns 0..15 below 2^29: four of them fit 32 bits
#pragma unroll
  for (int c = 0; c < NC - 1; c++) {
    uint32_t lo = (uint32_t)s.c[c];
    lo += (uint32_t)__shfl_xor((int)lo, 1, 64);
    lo += (uint32_t)__shfl_xor((int)lo, 2, 64);
    s.c[c] = lo;
  }
  {
    uint64_t top = s.c[NC - 1];
#pragma unroll
    for (int m = 1; m <= 2; m <<= 1) {
      const uint32_t ol = (uint32_t)__shfl_xor((int)(uint32_t)top, m, 64), oh = (uint32_t)__shfl_xor((int)(uint32_t)(top >> 32), m, 64);
      top += ((uint64_t)oh << 32) | ol;
    }
    s.c[NC - 1] = top;
  }
  __syncthreads();                                                                      // every read of a, b and T lies behind: dst may be one of them
  if (r == 0 && lane < 48) lds_fe_store(S + dst + q * NL, fe_canon_small<FqP>(cols_reduce<FqP>(s)));
  __syncthreads();
}
// S[dst] = S[a]^q: conj(a_i) g_i, the constants dealt out per output coefficient (pairing_consts.inc)
__device__ __forceinline__ void f12_frob(uint32_t* S, int dst, int a, int lane) {
  Fq res = fe_zero<FqP>();
  if (lane < 12) {
    const int i = lane >> 1;
    const Fq x = lds_fe(S + a + (2 * i) * NL), y = lds_fe(S + a + (2 * i + 1) * NL);
    Fq k0, k1;
#pragma unroll
    for (int l = 0; l < NL; l++) { k0.v[l] = PAIR_FROB[lane][0][l]; k1.v[l] = PAIR_FROB[lane][1][l]; }
    Cols s; cols_zero(s);
    cols_mac<FqP>(s, x, k0); cols_mac<FqP>(s, y, k1);
    res = fe_canon_small<FqP>(cols_reduce<FqP>(s));
  }
  __syncthreads();
  if (lane < 12) lds_fe_store(S + dst + lane * NL, res);
  __syncthreads();
}
// S[dst] = S[a]^(q^6): w -> -w
__device__ __forceinline__ void f12_conj(uint32_t* S, int dst, int a, int lane) {
  Fq res = fe_zero<FqP>();
  if (lane < 12) {
    res = lds_fe(S + a + lane * NL);
    if ((lane >> 1) & 1) res = fe_canon_small<FqP>(fe_norm<FqP>(fe_neg_lazy<FqP>(res)));
  }
  __syncthreads();
  if (lane < 12) lds_fe_store(S + dst + lane * NL, res);
  __syncthreads();
}
// S[dst] = 1 / (coefficient 0 of S[a]) as an Fq12 value (the norm of the easy part lies in Fq): one lane, ~380 serial products.  fe_inv's loop
// with the exponent's words read from memory: fe_inv keeps them in a local array it indexes by the bit counter, which costs a scratch segment
__device__ __forceinline__ void f12_inv_fq(uint32_t* S, int dst, int a, int lane) {
  Fq res = fe_zero<FqP>();
  if (lane == 0) {
    const Fq x = lds_fe(S + a);
    res = fe_one<FqP>();
#pragma unroll 1
    for (int i = 255; i >= 0; i--) {
      res = fe_sqr<FqP>(res);
      if ((PAIR_QM2[i >> 5] >> (i & 31)) & 1) res = fe_mul<FqP>(res, x);
    }
    res = fe_canon<FqP>(res);
  }
  __syncthreads();
  if (lane < 12) lds_fe_store(S + dst + lane * NL, res);
  __syncthreads();
}
// S[0] = S[0]^((q^12 - 1)/r) for a non-zero S[0]: the program PAIR_FINAL_EXP over the slots 0 .. PAIR_SLOTS - 1 (every slot is written before it is read)
__device__ __forceinline__ void f12_final_exp(uint32_t* S, int lane) {
#pragma unroll 1
  for (int pc = 0; pc < SBN_PAIRING_FINAL_EXP_LEN; pc++) {
    const uint32_t w = PAIR_FINAL_EXP[pc];
    const int op = w & 3, dst = ((w >> 2) & 15) * F12_WORDS, a = ((w >> 6) & 15) * F12_WORDS, b = ((w >> 10) & 15) * F12_WORDS;
    if (op == PAIR_OP_MUL) f12_mul(S, dst, a, b, lane);
    else if (op == PAIR_OP_FROB) f12_frob(S, dst, a, lane);
    else if (op == PAIR_OP_CONJ) f12_conj(S, dst, a, lane);
    else f12_inv_fq(S, dst, a, lane);
  }
}

// checks: gridDim.x descriptors; square_first[nlines]: the schedule every table was built over; out_is_one: a byte a check; out_gt: 384 bytes a
// check (arkworks' coefficient order, canonical little-endian) or null
__global__ void __launch_bounds__(64) k_pairing_products(const PairCheck* __restrict__ checks, const uint32_t* __restrict__ square_first, uint32_t nlines,
                                                         uint8_t* __restrict__ out_is_one, uint8_t* __restrict__ out_gt) {
  __shared__ uint32_t S[PAIR_LDS_WORDS];
  const int lane = threadIdx.x;
  const PairCheck* ck = checks + blockIdx.x;
  const uint32_t count = min(ck->count, (uint32_t)PAIR_TERMS_MAX);
  for (int i = lane; i < PAIR_T_OFF; i += 64) S[i] = 0;
  __syncthreads();
  if (lane == 0) lds_fe_store(S, fe_one<FqP>());
  if (lane < 2 * PAIR_TERMS_MAX) lds_fe_store(S + PAIR_P_OFF + lane * NL, fe_gload<FqP>(&ck->p[lane >> 1][8 * (lane & 1)]));
  __syncthreads();
  if (count) {
#pragma unroll 1
    for (uint32_t l = 0; l < nlines; l++) {
      if (square_first[l]) f12_mul(S, 0, 0, 0, lane);
#pragma unroll 1
      for (uint32_t t = 0; t < count; t++) {
        // the line at P_t:  yP  -  lam xP w  +  (lam xT - yT) w^3 ; lanes 1..4 take the record's four values, the first two times xP
        if (lane == 0) lds_fe_store(S + PAIR_LINE_OFF, lds_fe(S + PAIR_P_OFF + (2 * t + 1) * NL));
        if (lane >= 1 && lane <= 4) {
          const Fq v = fe_gload<FqP>(ck->lines[t] + (size_t)PAIR_LINE_BYTES * l + 32 * (lane - 1));
          const Fq m = lane <= 2 ? lds_fe(S + PAIR_P_OFF + (2 * t) * NL) : fe_one<FqP>();
          lds_fe_store(S + PAIR_LINE_OFF + (lane <= 2 ? 1 + lane : 3 + lane) * NL, fe_canon_small<FqP>(fe_mulu<FqP>(v, m)));
        }
        __syncthreads();
        f12_mul(S, 0, 0, PAIR_LINE_OFF, lane);
      }
    }
    f12_final_exp(S, lane);
  }
  bool ok = true;
  if (lane < 12) {
    const Fq x = lds_fe(S + lane * NL);
#pragma unroll
    for (int i = 0; i < NL; i++) ok = ok && x.v[i] == (lane == 0 ? SBN_C9(FqP::ONE29, i) : 0u);
    if (out_gt) {
      const int i = lane >> 1, part = lane & 1, pos = (i & 1) * 6 + (i >> 1) * 2 + part;      // w^(2m + h) is arkworks' c_h.c_m
      fe_gstore_packed<FqP>(out_gt + 384 * (size_t)blockIdx.x + 32 * pos, fe_from_mont<FqP>(x));
    }
  }
  const bool all_ok = __syncthreads_and(ok);
  if (lane == 0) out_is_one[blockIdx.x] = all_ok ? 1 : 0;
}

}  // namespace sbn
