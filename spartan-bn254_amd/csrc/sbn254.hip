// sbn254.hip — context, launch code and the C ABI (include/sbn254.h) of libsbn254_hip.so.
//
// Host-side mirror of the reference's operator boundary for the hot path:
//   GroupElement::msm_affine            src/group.rs:171-175        -> sbn_msm / sbn_msm_bases*
//   MultiCommitGens                     src/commitments.rs:17-114   -> sbn_bases_upload / sbn_gens_new
//   Commitments::commit, commit_inner   src/commitments.rs:144-154, src/hyrax.rs:253-308 -> sbn_commit_rows*
//   sumcheck prover loops / bind        src/sumcheck.rs, src/hyrax.rs:195-203            -> sbn_sc_* / sbn_bind_top
//   KZG commit / open (--features kzg)  src/kzg.rs                                       -> sbn_kzg_* / sbn_poly_div_linear
//   R1CSShape multiply_vec / evaluate, compute_eval_table_sparse  src/r1cs.rs:126-163  -> sbn_r1cs_*
//   multi_sparse_to_dense_rep, AddrTimestamps::new      src/sparse_mlpoly_full.rs:120-174, 211-243  -> sbn_dense_*
//   PolyEvalProof::prove, DotProductProofLog::prove     src/hyrax.rs:65-116, src/nizk/mod.rs:439-522 -> sbn_polyeval_prove / sbn_joint_opening_prove
//   PolyEvalProof::verify / verify_plain, DotProductProofLog::verify  src/hyrax.rs:118-151, src/nizk/mod.rs:525-567 -> sbn_polyeval_verify / sbn_joint_opening_verify
//   SparseMatPolyEvalProof::prove                        src/sparse_mlpoly_full.rs:1700-1755 -> sbn_sparse_eval_prove
//   SparseMatPolyEvalProof::prove (--features kzg), Derefs::commit_kzg  src/sparse_mlpoly_full.rs:1757-1813, 307-312 -> sbn_sparse_eval_prove_kzg / sbn_derefs_key_*
//   ZKSumcheckInstanceProof::prove_cubic_with_additive_term, ::prove_quad, DotProductProof::prove  src/sumcheck.rs:465-811, src/nizk/mod.rs:306-366 -> sbn_zk_sumcheck_prove_r1cs / _quad
//   R1CSProof::verify, ZKSumcheckInstanceProof::verify, DotProductProof::verify  src/r1csproof.rs:463-619, src/sumcheck.rs:366-457, src/nizk/mod.rs:368-400 -> sbn_r1cs_proof_verify / sbn_zk_sumcheck_verify
//   SparseMatPolyEvalProof::verify, PolyEvalNetworkProof::verify, ProductLayerProof / HashLayerProof::verify  src/sparse_mlpoly_full.rs:1815-1845, :1581-1650, :1436-1520, :1048-1265 -> sbn_sparse_eval_verify
//   KZGProof::verify, KZGBatchProof::batch_verify, Bn254::pairing  src/kzg.rs:196-217, :315-352 -> sbn_kzg_verify / _batched / sbn_pairing_products / sbn_g2_prepare
//   NIZKGens::new, NIZK::prove, NIZK::verify            src/snark.rs:162-287 -> sbn_nizk_*
//   R1CS::from_reader, to_sparse_matrices_padded, parse_wtns   src/r1cs_reader.rs:55-242, examples/keyless_benchmark.rs:38-72 -> sbn_circom_*
//   KZGSrs::load_from_file, save_to_file, load_or_generate  src/kzg.rs:66-115 -> sbn_kzg_srs_load / _save / _check / _g2_from_tau
//   (no twin in the reference) a powers-of-tau ceremony file as that SRS                   -> sbn_ptau_scan / sbn_kzg_srs_load_ptau
//   the verifier's short sums of proof points (nizk/mod.rs:560-565, :389-394 as GroupElement::vartime_multiscalar_mul)          -> sbn_g1_small_sums
// There is no CPU fallback in this file: every entry point needs the gfx950 device.
#include "../../include/sbn254.h"
#include "host_field.hpp"
#include "msm_kernels.cuh"
#include "sort2_kernels.cuh"
#include "glv_kernels.cuh"
#include "comb_kernels.cuh"
#include "sumcheck_kernels.cuh"
#include "sumcheck_comb_kernels.cuh"
#include "kzg_kernels.cuh"
#include "r1cs_kernels.cuh"
#include "dense_kernels.cuh"
#include "circom_kernels.cuh"
#include "transcript_kernels.cuh"
#include "polyeval_kernels.cuh"
#include "decompress_kernels.cuh"
#include "zk_sumcheck_kernels.cuh"
#include "r1cs_proof_kernels.cuh"
#include "r1cs_verify_kernels.cuh"
#include "small_sum_kernels.cuh"
#include "sparse_eval_kernels.cuh"
#include "derefs_key_kernels.cuh"
#include "pairing_kernels.cuh"
#include "srs_kernels.cuh"
#include "ptau_kernels.cuh"
#include "host_keccak.hpp"
#include "host_strobe.hpp"
#include "proof_host.hpp"
#include "verify_host.hpp"
#include "sparse_verify_host.hpp"
#include "snark_host.hpp"
#include "circom_host.hpp"
#include "pairing_host.hpp"
#include "srs_host.hpp"
#include "ptau_host.hpp"
#include "random_tape_host.hpp"

#include <hip/hip_runtime.h>
#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <condition_variable>
#include <cstring>
#include <functional>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <unordered_map>
#include <vector>

using namespace sbn;
// the host vocabulary of host_field.hpp and verify_host.hpp that the abi_*.inc files call by its short names
using sbn_host::fr::el_from; using sbn_host::fr::fr_canonical;
using sbn_host::g1_xy_valid; using sbn_host::g1_compressed_normalise; using sbn_host::g1_is_identity; using sbn_host::g1_neg_bytes; using sbn_host::fr_neg_bytes;
using sbn_host::fq_to_dev_mont; using sbn_host::OpeningShape; using sbn_host::opening_shape; using sbn_host::polyeval_host_eq; using sbn_host::joint_reduce;
using sbn_host::polyeval_verify_script; using sbn_host::polyeval_verify_scalars; using sbn_host::PolyevalFinal;

#include "ctx.hpp"
#include "msm_host.hpp"

#include "abi_msm.inc"
#include "abi_tables.inc"
#include "abi_transcript.inc"
#include "abi_sumcheck.inc"
#include "abi_product_proof.inc"
#include "abi_proof_common.inc"
#include "abi_verify_common.inc"
#include "abi_bullet.inc"
#include "abi_polyeval.inc"
#include "abi_polyeval_verify.inc"
#include "abi_zk_sumcheck.inc"
#include "abi_group.inc"
#include "abi_kzg.inc"
#include "abi_r1cs.inc"
#include "abi_r1cs_proof.inc"
#include "abi_r1cs_verify.inc"
#include "abi_small_sums.inc"
#include "abi_pairing.inc"
#include "abi_dense.inc"
#include "abi_derefs_key.inc"
#include "abi_sparse_eval.inc"
#include "abi_sparse_verify.inc"
#include "abi_snark.inc"
#include "abi_nizk.inc"
#include "abi_circom.inc"
#include "abi_kzg_srs.inc"
#include "abi_random_tape.inc"

extern "C" {

int sbn_prof_enable(sbn_ctx* c, int on) { if (!c) return SBN_EINVAL; std::lock_guard<std::mutex> g(c->mu); c->prof = on != 0; return SBN_OK; }
int sbn_prof_reset(sbn_ctx* c) { if (!c) return SBN_EINVAL; std::lock_guard<std::mutex> g(c->mu); hipStreamSynchronize(c->stream); prof_drain(c); c->prof_entries.clear(); return SBN_OK; }
int sbn_prof_count(sbn_ctx* c) { if (!c) return 0; std::lock_guard<std::mutex> g(c->mu); hipStreamSynchronize(c->stream); prof_drain(c); return (int)c->prof_entries.size(); }
int sbn_prof_get(sbn_ctx* c, int i, const char** name, double* total_ms, uint64_t* launches) {
  if (!c || i < 0 || (size_t)i >= c->prof_entries.size()) return SBN_EINVAL;
  if (name) *name = c->prof_entries[i].name.c_str();
  if (total_ms) *total_ms = c->prof_entries[i].ms;
  if (launches) *launches = c->prof_entries[i].launches;
  return SBN_OK;
}
int sbn_prof_last_job(sbn_ctx* c, uint64_t out[4]) {
  if (!c || !out) return SBN_EINVAL;
  std::lock_guard<std::mutex> g(c->mu);
  for (int i = 0; i < 4; i++) out[i] = c->last_job[i];
  return SBN_OK;
}
int sbn_prof_last_acc(sbn_ctx* c, uint64_t out[8]) {
  if (!c || !out) return SBN_EINVAL;
  std::lock_guard<std::mutex> g(c->mu);
  for (int i = 0; i < 6; i++) out[i] = c->last_acc[i];
  out[6] = out[7] = 0;
  if (!c->acc_ctr.p) return SBN_OK;          // no bucket job yet
  AccCounters h;
  HIPCHK(c, hipStreamSynchronize(c->stream));
  HIPCHK(c, hipMemcpy(&h, c->acc_ctr.p, sizeof h, hipMemcpyDeviceToHost));
  out[6] = h.extra_count; out[7] = h.big_count;
  return SBN_OK;
}

}  // extern "C"
