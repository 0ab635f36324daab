// zk_sumcheck_kernels.cuh — the small kernels between the round launches of sbn_zk_sumcheck_prove_r1cs / _quad (abi_zk_sumcheck.inc):
// ZKSumcheckInstanceProof::prove_cubic_with_additive_term (sumcheck.rs:465-649) and ::prove_quad (sumcheck.rs:657-811).
// Every group element of a round is a row commitment over the ONE derived set  gens_n.G ‖ gens_n.h ‖ gens_1.G[0] ‖ gens_1.h  (n + 3 points,
// no blind column: the two h are ordinary columns), so these kernels only write rows of n + 3 canonical scalars:
//   tail:       behind the round kernel, [coeffs ‖ blinds_poly[j] ‖ 0 ‖ 0] (comm_poly_j) and [d_vec_j ‖ r_delta_j ‖ 0 ‖ 0] (delta_j)
//   host rows:  [0 ... 0 ‖ 0 ‖ v ‖ b] twice, from scalars the host already holds (comm_eval / comm_claim, Cy / beta)
// All of them are one block; what they read was written by earlier launches of the stream.
#pragma once
#include "transcript_kernels.cuh"

namespace sbn {

constexpr int ZK_MBOX_SLOT_WORDS = 128;      // one result slot of the host mailbox: two XYZZ sums (64 words), up to 4 scalars behind them, spare
constexpr int ZK_MBOX_SLOTS = 4;             // A = {comm_poly, delta}, B = {comm_eval, comm_claim}, C = {Cy, beta}, the final claims
static_assert(ZK_MBOX_SLOTS * ZK_MBOX_SLOT_WORDS <= SC_MBOX_WORDS - SC_MBOX_FINALS, "mailbox: the four result slots must fit the final-claims area");
static_assert(ZK_MBOX_SLOTS + 1 <= 8, "mailbox: one flag word per slot behind the final-claims flag");

struct ZkTailArgs {
  const uint32_t* sums;       // the round kernel's results: e0, e2 (, e3) as canonical integers (slot 0 of the mailbox's device twin)
  const uint32_t* rnd;        // the call's rnd, canonical, as the caller ordered it
  uint32_t* rows;             // out: two rows of n + 3 canonical scalars
  uint32_t* coeffs;           // out: the n coefficients, canonical (they travel to the host with the commit's sums)
  uint32_t blind_idx;         // index in rnd of blinds_poly[j]
  uint32_t d_idx;             // index in rnd of d_vec_j[0]; r_delta_j follows the n entries
};
// e1 = claim - e0 (sumcheck.rs:534, :701), UniPoly::from_evals (unipoly.rs:28-59) with k_tr_sumcheck_step's formulas and constants, the
// two commit rows.  claim: Montgomery form, canonical words.  Every lane runs the field work; lane k stores column k.
template <int KIND>
__global__ void __launch_bounds__(64) k_zk_round_tail(ZkTailArgs A, ScScalar claim) {
  constexpr int N = KIND == KIND_QUAD ? 3 : 4;
  const int lane = threadIdx.x;
  const Fr e0 = fe_to_mont(fe_load<FrP>(A.sums)), e2 = fe_to_mont(fe_load<FrP>(A.sums + 8));     // (-0.1 r, 1.1 r)
  const Fr e1 = fe_sub(fr_from_words(claim), e0);
  Fr mine;
  if (KIND == KIND_QUAD) {
    const Fr ca = fe_mul(fe_add(fe_sub(e2, fe_dbl(e1)), e0), tr_fr_inv2());             // a = (e2 - 2 e1 + e0) / 2;  |.| < 5 r
    const Fr cb = fe_sub(fe_sub(e1, e0), ca);                                           // b = e1 - c - a
    mine = fe_sel4(lane & 3, e0, cb, ca, ca);                                           // [c, b, a]
  } else {
    const Fr e3 = fe_to_mont(fe_load<FrP>(A.sums + 16));
    Fr xa = fe_sub(e3, e0), d21 = fe_sub(e1, e2);
    xa = fe_add(xa, fe_add(fe_dbl(d21), d21));                                          // e3 - 3 e2 + 3 e1 - e0;  |.| < 9 r
    Fr xb = fe_sub(fe_dbl(fe_sub(e0, e1)), e3);
    xb = fe_add(xb, fe_add(fe_dbl(fe_dbl(fe_sub(e2, e1))), e1));                        // 2 e0 - 5 e1 + 4 e2 - e3;  |.| < 16 r
    const Fr ca = fe_mul(xa, tr_fr_inv6()), cb = fe_mul(xb, tr_fr_inv2());
    const Fr cc = fe_sub(fe_sub(e1, e0), fe_add(ca, cb));                               // c = e1 - d - a - b
    mine = fe_sel4(lane & 3, e0, cc, cb, ca);                                           // [d, c, b, a]
  }
  const Fr plain = fe_from_mont(mine);
  uint32_t* row0 = A.rows; uint32_t* row1 = A.rows + 8 * (N + 3);
  if (lane < N) {
    fe_store_packed<FrP>(row0 + 8 * lane, plain);
    fe_store_packed<FrP>(A.coeffs + 8 * lane, plain);
    fe_store_packed<FrP>(row1 + 8 * lane, fe_load<FrP>(A.rnd + 8 * (A.d_idx + lane)));
  } else if (lane == N) {
    fe_store_packed<FrP>(row0 + 8 * N, fe_load<FrP>(A.rnd + 8 * A.blind_idx));
    fe_store_packed<FrP>(row1 + 8 * N, fe_load<FrP>(A.rnd + 8 * (A.d_idx + N)));
  } else if (lane < N + 3) {
    fe_store_packed<FrP>(row0 + 8 * lane, fe_zero<FrP>());
    fe_store_packed<FrP>(row1 + 8 * lane, fe_zero<FrP>());
  }
}

// two rows [0 ... 0 ‖ 0 ‖ v ‖ b] over the derived set: v * gens_1.G[0] + b * gens_1.h.  v0, b0, v1, b1: canonical words
__global__ void __launch_bounds__(64) k_zk_host_rows(uint32_t* __restrict__ rows, uint32_t n, ScScalar v0, ScScalar b0, ScScalar v1, ScScalar b1) {
  const uint32_t t = threadIdx.x, R = n + 3;
  if (t >= 2 * R) return;
  const uint32_t row = t / R, col = t - row * R;
  uint32_t* o = rows + 8 * t;
#pragma unroll
  for (int k = 0; k < 8; k++) {
    uint32_t x = 0;
    if (col == n + 1) x = row ? v1.v[k] : v0.v[k];
    if (col == n + 2) x = row ? b1.v[k] : b0.v[k];
    o[k] = x;
  }
}

// The hand-over of a row commit (abi_proof_common.inc: rows_to_host_launch): the npoints XYZZ sums (32 words each) and the `nextra` words that
// travel with them, to the host mailbox from `host_out` on, the flag behind them.  One block; a caller with at most 128 words launches 128 threads.
__global__ void __launch_bounds__(256) k_points_to_host(const uint32_t* __restrict__ sums, uint32_t npoints, const uint32_t* __restrict__ extra, uint32_t nextra,
                                                        uint32_t* __restrict__ host_out, uint32_t* __restrict__ flag, uint32_t seq) {
  const uint32_t ns = 32 * npoints;
  for (uint32_t t = threadIdx.x; t < ns + nextra; t += blockDim.x) host_out[t] = t < ns ? sums[t] : extra[t - ns];
  sc_drain_stores();
  __syncthreads();
  if (threadIdx.x == 0) sc_flag_store(flag, seq);
}

// the last bind (two entries per table left), in place as k_bind_top leaves it, and the final claims to the host: one lane per table
struct ZkTabs { uint32_t* p[4]; };
__global__ void __launch_bounds__(64) k_zk_bind_last(ZkTabs T, uint32_t count, ScScalar rmont, uint32_t* __restrict__ host_out, uint32_t* __restrict__ flag, uint32_t seq) {
  const uint32_t t = threadIdx.x;
  uint32_t* z = nullptr;
#pragma unroll
  for (int i = 0; i < 4; i++) if (i == (int)t) z = T.p[i];
  if (t < count) {
    const Fr v = sc_bind1(fe_load<FrP>(z), fe_load<FrP>(z + 8), fr_from_words(rmont));
    fe_store_packed<FrP>(z, v);
    fe_store_packed<FrP>(host_out + 8 * t, fe_from_mont(v));
  }
  sc_drain_stores();
  __syncthreads();
  if (t == 0) sc_flag_store(flag, seq);
}

}  // namespace sbn
