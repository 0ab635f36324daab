// polyeval_kernels.cuh — the kernels around the bullet rounds of sbn_polyeval_prove (abi_polyeval.inc): PolyEvalProof::prove
// (hyrax.rs:65-116) with DotProductProofLog::prove (nizk/mod.rs:439-522).  Every group element of the opening is a row commitment over
// the ONE derived set G ‖ Q_base with h (abi_bullet.inc), so these kernels only write rows in the commit's input layout — two rows of
// n + 1 canonical scalars, then the two blinds — straight into the bullet state's buffers:
//   front:  Cx row [L*Z ‖ 0] with blind <blinds, L>,  Cy row [0 ... 0 ‖ Zr] with blind blind_Zr;  a = L*Z, b = R, s = 1 for the rounds
//   close:  delta row [d * s_t ‖ 0] with blind r_delta,  beta row [0 ... 0 ‖ d * r] with blind r_beta;  a_hat, b_hat for the host
// No block of these kernels reads what another block of the same launch wrote: everything is handed over in stream order.
#pragma once
#include "sumcheck_kernels.cuh"

namespace sbn {

// the two halves of the opening point (compute_factored_lens, hyrax.rs:371-373), Montgomery form, by value: ell <= 40, so <= 20 per side
constexpr int PE_SIDE_MAX = 20;
struct PolyEvalPoint { uint32_t l[PE_SIDE_MAX][8]; uint32_t r[PE_SIDE_MAX][8]; };

// EqPolynomial::compute_factored_evals (hyrax.rs:375-383): L[i] = prod_j (bit_{ml-1-j}(i) ? l_j : 1 - l_j), R likewise — the field
// elements the recurrence of hyrax.rs:360-366 produces (k_eq_direct's form; statically indexed selects keep the point in registers).
// Lv: 2^ml entries, Rv: 2^mr entries, s: 2^mr ones (the generator coefficients of the bullet state before the first fold).
__global__ void __launch_bounds__(256) k_polyeval_eq(PolyEvalPoint p, int ml, int mr, uint32_t* __restrict__ Lv, uint32_t* __restrict__ Rv, uint32_t* __restrict__ s) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const Fr one = fe_one<FrP>();
  if (i < ((size_t)1 << ml)) {
    Fr acc = one;
#pragma unroll
    for (int j = 0; j < PE_SIDE_MAX; j++)
      if (j < ml) { const Fr r = fe_unpack<FrP>(p.l[j]); acc = fe_mul(acc, ((i >> (ml - 1 - j)) & 1) ? r : fe_sub(one, r)); }
    fe_store_tab<FrP>(Lv + 8 * i, acc);
  }
  if (i < ((size_t)1 << mr)) {
    Fr acc = one;
#pragma unroll
    for (int j = 0; j < PE_SIDE_MAX; j++)
      if (j < mr) { const Fr r = fe_unpack<FrP>(p.r[j]); acc = fe_mul(acc, ((i >> (mr - 1 - j)) & 1) ? r : fe_sub(one, r)); }
    fe_store_tab<FrP>(Rv + 8 * i, acc);
    fe_store_packed<FrP>(s + 8 * i, one);
  }
}

struct PolyEvalFront {
  const uint32_t* partial;      // k_bound_partial's slices: nslices x n, Montgomery
  const uint32_t* Lv;           // L, Montgomery (L_size entries)
  const uint32_t* blinds;       // L_size canonical scalars, or null = zeros (hyrax.rs:83-86)
  uint32_t* a;                  // L*Z, Montgomery: the bullet state's a
  uint32_t* w0; uint32_t* w1;   // the two commit rows, n + 1 canonical scalars each
  uint32_t* bl;                 // the two blinds, canonical
  uint32_t* dots;               // 2 x 8 words for the host: <blinds, L>, 0
};
// blocks [0, gridDim.x - 1): the fold of the bound slices (k_bound_fold) with the Cx / Cy rows written beside the table;
// the last block: LZ_blind = <blinds, L> (hyrax.rs:101), the rows' last column (0 for Cx, Zr for Cy) and the two blinds.
__global__ void __launch_bounds__(256) k_polyeval_front(PolyEvalFront A, size_t nslices, size_t n, size_t L_size, ScScalar Zr, ScScalar blind_Zr) {
  if (blockIdx.x + 1 < gridDim.x) {
    const size_t col = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (col >= n) return;
    Fr s = fe_zero<FrP>();
    uint32_t cnt = 0;
    for (size_t k = 0; k < nslices; k++) fr_acc(s, fe_load<FrP>(A.partial + 8 * (k * n + col)), cnt);
    s = fe_reduce(s);
    fe_store_tab<FrP>(A.a + 8 * col, s);
    fe_store_packed<FrP>(A.w0 + 8 * col, fe_from_mont(s));        // canonical plain integer: the commit cuts digits from it
    fe_store_packed<FrP>(A.w1 + 8 * col, fe_zero<FrP>());
    return;
  }
  Fr acc = fe_zero<FrP>();
  uint32_t cnt = 0;
  if (A.blinds)
    for (size_t i = threadIdx.x; i < L_size; i += blockDim.x)
      fr_acc(acc, fe_mul(fe_to_mont(fe_load<FrP>(A.blinds + 8 * i)), fe_load<FrP>(A.Lv + 8 * i)), cnt);
  __shared__ uint32_t sm[4][NL];
  acc = wave_sum_fr(fe_reduce(acc));
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  if (lane == 0) for (int k = 0; k < NL; k++) sm[wv][k] = acc.v[k];
  __syncthreads();
  if (threadIdx.x == 0) {
    Fr s = fe_zero<FrP>();
    for (int w = 0; w < 4; w++) { Fr x; for (int k = 0; k < NL; k++) x.v[k] = sm[w][k]; s = fe_add(s, x); }
    const Fr bx = fe_from_mont(fe_reduce(s));
    fe_store_packed<FrP>(A.bl, bx);
    fe_store_packed<FrP>(A.dots, bx);
    fe_store_packed<FrP>(A.dots + 8, fe_zero<FrP>());
    fe_store_packed<FrP>(A.w0 + 8 * n, fe_zero<FrP>());
  }
  if (threadIdx.x >= 64 && threadIdx.x < 72) { const int k = threadIdx.x - 64; A.w1[8 * n + k] = Zr.v[k]; A.bl[8 + k] = blind_Zr.v[k]; }
}

// After the last round the vectors have two entries.  The fold with the last challenge (bullet.rs:86-106) and, from its results, the rows of
//   delta = d * g_hat + r_delta * h  with g_hat = MSM(s, G) (nizk/mod.rs:497-500):  [d * s_t ‖ 0],  blind r_delta
//   beta  = d * (r * Q_base) + r_beta * h (nizk/mod.rs:503):                         [0 ... 0 ‖ d * r],  blind r_beta
// canonical, as k_bullet_prep writes its rows; a_hat, b_hat (bullet.rs:114-115) go to dots for the host.  g_hat itself is never formed.
// d: Montgomery form; dr = d * r and the blinds: canonical words.  s is only read (the state is dropped behind this launch).
__global__ void __launch_bounds__(256) k_polyeval_close(const uint32_t* __restrict__ a, const uint32_t* __restrict__ b, const uint32_t* __restrict__ s,
                                                        uint32_t* __restrict__ w0, uint32_t* __restrict__ w1, uint32_t* __restrict__ bl, uint32_t* __restrict__ dots,
                                                        size_t n, ScScalar su, ScScalar si, ScScalar d, ScScalar dr, ScScalar r_delta, ScScalar r_beta) {
  const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const Fr u = fr_from_words(su), ui = fr_from_words(si);
  if (t < n) {
    const Fr st = fe_mul(fe_load<FrP>(s + 8 * t), (t & 1) ? u : ui);                 // the last fold of the coefficients: m = 2
    fe_store_packed<FrP>(w0 + 8 * t, fe_from_mont(fe_mul(st, fr_from_words(d))));
    fe_store_packed<FrP>(w1 + 8 * t, fe_zero<FrP>());
  }
  if (blockIdx.x != 0) return;
  if (threadIdx.x == 0) {
    const Fr ah = fe_add(fe_mul(u, fe_load<FrP>(a)), fe_mul(ui, fe_load<FrP>(a + 8)));
    const Fr bh = fe_add(fe_mul(ui, fe_load<FrP>(b)), fe_mul(u, fe_load<FrP>(b + 8)));
    fe_store_packed<FrP>(dots, fe_from_mont(fe_reduce(ah)));
    fe_store_packed<FrP>(dots + 8, fe_from_mont(fe_reduce(bh)));
    fe_store_packed<FrP>(w0 + 8 * n, fe_zero<FrP>());
  }
  if (threadIdx.x >= 64 && threadIdx.x < 72) { const int k = threadIdx.x - 64; w1[8 * n + k] = dr.v[k]; bl[k] = r_delta.v[k]; bl[8 + k] = r_beta.v[k]; }
}

}  // namespace sbn
