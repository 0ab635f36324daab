// sparse_eval_kernels.cuh — the one kernel sbn_sparse_eval_prove (abi_sparse_eval.inc) adds to the pieces it composes:
// SparseMatPolyEvalProof::prove (sparse_mlpoly_full.rs:1700-1755).
//   k_se_claims   every claim ProductLayerProof::prove appends before its two product proofs (sparse_mlpoly_full.rs:1316-1369) to ONE host slot:
//                 ProductCircuit::evaluate of the 4 batch + 4 circuits (entry 0 of each circuit's one-entry top layer) and
//                 DotProductCircuit::evaluate of the 2 batch split dot-product circuits (the fold of k_pp_dotp's per-block partial sums)
// and the fused kernel of the construction path (sbn_hash_layer_pair_product, abi_tables.inc):
//   k_hash_pair_prod   k_hash_layer_pair and the first k_product_layer of both sets in one pass: the hashed sets are not read back
#pragma once
#include "zk_sumcheck_kernels.cuh"

namespace sbn {

constexpr int SE_BATCH_MAX = 4;                          // 6 batch instances in proof_ops <= SC_PACK_MAX, 4 batch circuits <= PC_MANY_MAX
constexpr int SE_TOPS_MAX = 4 * SE_BATCH_MAX + 4;
constexpr int SE_DOTP_MAX = 2 * SE_BATCH_MAX;
static_assert(6 * SE_BATCH_MAX <= SC_PACK_MAX && 4 * SE_BATCH_MAX <= PC_MANY_MAX, "batch limit against the instance and circuit packs");
static_assert((SE_TOPS_MAX + SE_DOTP_MAX) * 8 <= ZK_MBOX_SLOTS * ZK_MBOX_SLOT_WORDS, "mailbox: the claims must fit the four ZK result slots together");

struct SeTops { const uint32_t* p[SE_TOPS_MAX]; };
// One block of four waves.  Lane t < n_tops: the top of circuit t (a per-lane select over the kernel-argument block, as k_pp_read0: a dynamic
// index would move the block to scratch).  Wave w: the dot-product sums w, w + 4: partial[k * nblk + b] as k_pp_dotp left them (table format,
// at most 16 terms per lane as in k_pp_claims0).  Canonical integers out: tops first, the sums behind them; the flag follows the results.
__global__ void __launch_bounds__(256) k_se_claims(SeTops tops, uint32_t n_tops, const uint32_t* __restrict__ partial, uint32_t nblk, uint32_t n_dotp,
                                                   uint32_t* __restrict__ host_out, uint32_t* __restrict__ flag, uint32_t seq) {
  const uint32_t t = threadIdx.x, lane = t & 63, wv = t >> 6;
  const uint32_t* z = nullptr;
#pragma unroll
  for (int i = 0; i < SE_TOPS_MAX; i++) if (i == (int)t) z = tops.p[i];
  if (t < n_tops) fe_store_packed<FrP>(host_out + 8 * t, fe_from_mont(fe_load<FrP>(z)));
  for (uint32_t k = wv; k < n_dotp; k += 4) {
    Fr s = fe_zero<FrP>();
    for (uint32_t b = lane; b < nblk; b += 64) s = fe_add(s, fe_load<FrP>(partial + 8 * ((size_t)k * nblk + b)));
    s = wave_sum_fr(fe_reduce(s));
    if (lane == 0) fe_store_packed<FrP>(host_out + 8 * (n_tops + k), fe_from_mont(fe_reduce(s)));
  }
  sc_drain_stores();
  __syncthreads();
  if (t == 0) sc_flag_store(flag, seq);
}

// Two hashed sets over the same (addr, val) — k_hash_layer_pair — and the first layer of both product circuits (ProductCircuit::compute_layer,
// product_tree.rs:21-37) in one pass: index i < half forms the pair's four hashes at i and i + half, stores them to out_a / out_b (the sumcheck
// reads layer 0) and stores prod_a[i] = a[i] * a[i + half], prod_b[i] likewise.  The products are formed from the values AS STORED: fe_store_tab
// stores fe_fix_tab(fe_norm(x)), so that representative is made once, stored packed and multiplied — what k_product_layer multiplies after its
// fe_load of the same words (a normalised value in [0, 2.5 r) packs and unpacks to the same limbs).  16-byte loads and stores, consecutive lanes on consecutive entries, grid-stride.  Timestamps enter the field as
// 64-bit sums, so 2^32 - 1 with add 1 does not wrap.
__global__ void __launch_bounds__(256) k_hash_pair_prod(const uint32_t* __restrict__ addr, const uint32_t* __restrict__ val, const uint32_t* __restrict__ ts_a, uint32_t add_a,
                                                        const uint32_t* __restrict__ ts_b, uint32_t add_b, ScScalar g_m, ScScalar g2rr_m, ScScalar ntau_m, size_t half,
                                                        uint32_t* __restrict__ out_a, uint32_t* __restrict__ out_b, uint32_t* __restrict__ prod_a, uint32_t* __restrict__ prod_b) {
  const Fr g = fr_from_words(g_m), g2rr = fr_from_words(g2rr_m), ntau = fr_from_words(ntau_m);
  const Fr rr = fe_const_r2<FrP>();
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < half; i += (size_t)gridDim.x * blockDim.x) {
    Fr ha[2], hb[2];
#pragma unroll
    for (int s = 0; s < 2; s++) {
      const size_t j = i + (size_t)s * half;
      const unsigned long long av = addr ? addr[j] : (unsigned long long)j;
      const unsigned long long ta = (unsigned long long)(ts_a ? ts_a[j] : 0u) + add_a, tb = (unsigned long long)(ts_b ? ts_b[j] : 0u) + add_b;
      const Fr base = fe_add(fe_add(fe_mul(fe_gload<FrP>(val + 8 * j), g), fe_mul(rr, fe_from_u64<FrP>(av))), ntau);      // as k_hash_layer_pair
      ha[s] = fe_fix_tab<FrP>(fe_norm(fe_add(base, fe_mul(g2rr, fe_from_u64<FrP>(ta)))));
      hb[s] = fe_fix_tab<FrP>(fe_norm(fe_add(base, fe_mul(g2rr, fe_from_u64<FrP>(tb)))));
      fe_gstore_packed<FrP>(out_a + 8 * j, ha[s]);
      fe_gstore_packed<FrP>(out_b + 8 * j, hb[s]);
    }
    fe_gstore_tab<FrP>(prod_a + 8 * i, fe_mul(ha[0], ha[1]));
    fe_gstore_tab<FrP>(prod_b + 8 * i, fe_mul(hb[0], hb[1]));
  }
}

}  // namespace sbn
