//! `src/hip.rs` of the reference crate (feature `hip`): the Rust side of libsbn254_hip.so.
//!
//! Everything the reference's prover hot path needs from the MI355X library, behind the reference's own function
//! signatures: `shim/patches/*.diff` replace the bodies of
//!   GroupElement::msm_affine / vartime_multiscalar_mul      group.rs:143-158, 171-175
//!   <[Scalar] as Commitments>::commit                        commitments.rs:131-154
//!   DensePolynomial::commit_inner                            hyrax.rs:253-281
//!   SumcheckInstanceProof::{prove_cubic, prove_cubic_batched}          sumcheck.rs:89-161, 165-330
//!   ZKSumcheckInstanceProof::{prove_cubic_with_additive_term, prove_quad}   sumcheck.rs:465-649, 657-811
//!   BulletReductionProof::prove (through DotProductProofLog::prove)    nizk/bullet.rs:41-126, nizk/mod.rs:478-494
//! by calls into this module; nothing else in the crate changes.  The `extern "C"` block is generated from
//! include/sbn254.h (`tools/gen_rust_ffi.py`); `tests/test_shim_consistency.py` checks name, arity, argument order and
//! pointer-ness of every declaration against the header, so the two cannot drift.
//!
//! Not compiled in the build image (no Rust toolchain there): complete on paper, checked mechanically as far as that goes.
#![allow(non_camel_case_types, non_snake_case, clippy::too_many_arguments, clippy::missing_safety_doc)]

use std::borrow::Cow;
use std::collections::HashMap;
use std::os::raw::{c_char, c_int, c_void};
use std::ptr::{null, null_mut};
use std::sync::{Arc, Mutex, OnceLock};

use ark_bn254::{Fq, G1Affine, G1Projective};
use ark_ec::{AffineRepr, CurveGroup};
use ark_ff::PrimeField;
use merlin::Transcript;

use crate::commitments::MultiCommitGens;
use crate::group::GroupElement;
use crate::hyrax::DensePolynomial;
use crate::scalar::Scalar;
use crate::sparse_mlpoly::SparseMatPolynomial;
use crate::group::CompressedGroup;
use crate::nizk::DotProductProof;
use crate::random::RandomTape;
use crate::r1cs::R1CSShape;
use crate::r1csproof::{R1CSGens, R1CSProof};
use crate::sparse_mlpoly_full::{SparseMatPolyCommitmentGens, SparseMatPolyEvalProof};
use crate::sumcheck::{SumcheckInstanceProof, ZKSumcheckInstanceProof};
use ark_serialize::{CanonicalDeserialize, CanonicalSerialize};
use crate::errors::ProofVerifyError;
use crate::hyrax::{PolyCommitment, PolyCommitmentGens, PolyEvalProof};
use crate::transcript::{AppendToTranscript, ProofTranscript};
use crate::unipoly::{CompressedUniPoly, UniPoly};

// ---- opaque handles of the C ABI ------------------------------------------------------------------------------------
#[repr(C)] pub struct sbn_ctx { _p: [u8; 0] }
#[repr(C)] pub struct sbn_bases { _p: [u8; 0] }
#[repr(C)] pub struct sbn_table { _p: [u8; 0] }
#[repr(C)] pub struct sbn_sumcheck { _p: [u8; 0] }
#[repr(C)] pub struct sbn_bullet { _p: [u8; 0] }
#[repr(C)] pub struct sbn_group { _p: [u8; 0] }
#[repr(C)] pub struct sbn_group_bases { _p: [u8; 0] }
#[repr(C)] pub struct sbn_r1cs { _p: [u8; 0] }
#[repr(C)] pub struct sbn_dense { _p: [u8; 0] }
#[repr(C)] pub struct sbn_derefs_key { _p: [u8; 0] }
#[repr(C)] pub struct sbn_g2_lines { _p: [u8; 0] }
#[repr(C)] pub struct sbn_transcript { _p: [u8; 0] }
#[repr(C)] pub struct sbn_snark_gens { _p: [u8; 0] }
#[repr(C)] pub struct sbn_snark_key { _p: [u8; 0] }
#[repr(C)] pub struct sbn_nizk_inst { _p: [u8; 0] }
#[repr(C)] pub struct sbn_circom_r1cs { _p: [u8; 0] }
#[repr(C)] pub struct sbn_random_tape { _p: [u8; 0] }
/// what `sbn_circom_r1cs_info` fills: the file's header fields, the kept and dropped entries per matrix, the shape `Instance::new` gives
#[repr(C)] #[derive(Clone, Copy, Debug, Default)]
pub struct sbn_circom_info {
    pub num_constraints: u64, pub num_variables: u64, pub num_pub_inputs: u64, pub num_prv_inputs: u64, pub num_labels: u64,
    pub nnz: [u64; 3], pub dropped: [u64; 3],
    pub num_vars: u64, pub num_cons_padded: u64, pub num_vars_padded: u64,
}
/// what `sbn_ptau_scan` fills: the header section of a powers-of-tau file, the point counts and the byte offsets of sections 2 and 3
#[repr(C)] #[derive(Clone, Copy, Debug, Default)]
pub struct sbn_ptau_info {
    pub power: u32, pub ceremony_power: u32,
    pub n_g1: u64, pub n_g2: u64, pub off_g1: u64, pub off_g2: u64,
}

pub const SBN_OK: c_int = 0;
pub const SBN_SCALARS_MONT: u32 = 1;
pub const SBN_POINTS_MONT: u32 = 2;
pub const SBN_SRS_CHECK: u32 = 1;

/// MSMs below this many terms stay on arkworks: the Σ-protocol steps commit 1–5 scalars at a time (`nizk/mod.rs`,
/// `sumcheck.rs:539-634`) and a device call is a ~20 µs round trip + a ~0.3 ms latency-bound bucket pass.
pub const MIN_GPU_MSM: usize = 256;

#[link(name = "sbn254_hip")]
extern "C" {
    // GENERATED-BEGIN (tools/gen_rust_ffi.py from include/sbn254.h — do not edit by hand)
    pub fn sbn_ctx_create(device: c_int, out: *mut *mut sbn_ctx) -> c_int;
    pub fn sbn_ctx_destroy(ctx: *mut sbn_ctx);
    pub fn sbn_last_error(ctx: *const sbn_ctx) -> *const c_char;
    pub fn sbn_ctx_set_stream(ctx: *mut sbn_ctx, hip_stream: *mut c_void) -> c_int;
    pub fn sbn_ctx_sync(ctx: *mut sbn_ctx) -> c_int;
    pub fn sbn_version() -> *const c_char;
    pub fn sbn_dev_alloc(ctx: *mut sbn_ctx, bytes: usize, out_dev: *mut *mut c_void) -> c_int;
    pub fn sbn_dev_free(ctx: *mut sbn_ctx, dev: *mut c_void) -> c_int;
    pub fn sbn_dev_upload(ctx: *mut sbn_ctx, dst_dev: *mut c_void, src_host: *const c_void, bytes: usize) -> c_int;
    pub fn sbn_dev_download(ctx: *mut sbn_ctx, dst_host: *mut c_void, src_dev: *const c_void, bytes: usize) -> c_int;
    pub fn sbn_msm(ctx: *mut sbn_ctx, scalars: *const u8, points: *const u8, n: usize, flags: u32, out_xy: *mut u8, out_is_inf: *mut c_int) -> c_int;
    pub fn sbn_msm_jacobian(ctx: *mut sbn_ctx, scalars: *const u8, points_xyz: *const u8, n: usize, flags: u32, out_xy: *mut u8, out_is_inf: *mut c_int) -> c_int;
    pub fn sbn_bases_upload(ctx: *mut sbn_ctx, g_xy: *const u8, n: usize, h_xy: *const u8, flags: u32, out: *mut *mut sbn_bases) -> c_int;
    pub fn sbn_bases_free(ctx: *mut sbn_ctx, b: *mut sbn_bases);
    pub fn sbn_bases_len(b: *const sbn_bases) -> usize;
    pub fn sbn_bases_precompute(ctx: *mut sbn_ctx, b: *mut sbn_bases, max_bytes: usize, window_bits: *mut c_int) -> c_int;
    pub fn sbn_gens_new(ctx: *mut sbn_ctx, n: usize, label: *const u8, label_len: usize, out_xy: *mut u8, out: *mut *mut sbn_bases) -> c_int;
    pub fn sbn_bases_synthetic(ctx: *mut sbn_ctx, n: usize, first: u64, s0: *const u8, d: *const u8, out: *mut *mut sbn_bases) -> c_int;
    pub fn sbn_scalars_synthetic(ctx: *mut sbn_ctx, seed: u64, first: u64, n: usize, out_dev: *mut c_void) -> c_int;
    pub fn sbn_bases_download(ctx: *mut sbn_ctx, b: *const sbn_bases, first: usize, count: usize, out_xy: *mut u8) -> c_int;
    pub fn sbn_bases_split_at(ctx: *mut sbn_ctx, b: *const sbn_bases, mid: usize, left: *mut *mut sbn_bases, right: *mut *mut sbn_bases) -> c_int;
    pub fn sbn_bases_scale(ctx: *mut sbn_ctx, b: *const sbn_bases, s: *const u8, out: *mut *mut sbn_bases) -> c_int;
    pub fn sbn_msm_bases(ctx: *mut sbn_ctx, b: *const sbn_bases, scalars: *const u8, n: usize, flags: u32, out_xy: *mut u8, out_is_inf: *mut c_int) -> c_int;
    pub fn sbn_msm_bases_dev(ctx: *mut sbn_ctx, b: *const sbn_bases, scalars_dev: *const c_void, n: usize, flags: u32, out_xy: *mut u8, out_is_inf: *mut c_int) -> c_int;
    pub fn sbn_commit_rows(ctx: *mut sbn_ctx, b: *const sbn_bases, z: *const u8, blinds: *const u8, l: usize, r: usize, flags: u32, out_xy: *mut u8, out_inf: *mut u8) -> c_int;
    pub fn sbn_commit_rows_dev(ctx: *mut sbn_ctx, b: *const sbn_bases, z_dev: *const c_void, blinds_dev: *const c_void, l: usize, r: usize, flags: u32, out_xy: *mut u8, out_inf: *mut u8) -> c_int;
    pub fn sbn_g1_compress(xy: *const u8, n: usize, out32: *mut u8) -> c_int;
    pub fn sbn_g1_sum(xy: *const u8, n: usize, out_xy: *mut u8, out_is_inf: *mut c_int) -> c_int;
    pub fn sbn_unipoly_from_evals(evals: *const u8, n: usize, coeffs: *mut u8) -> c_int;
    pub fn sbn_unipoly_eval(coeffs: *const u8, n: usize, r: *const u8, out: *mut u8) -> c_int;
    pub fn sbn_factored_lens(ell: usize, left: *mut usize, right: *mut usize);
    pub fn sbn_table_upload(ctx: *mut sbn_ctx, z: *const u8, len: usize, flags: u32, out: *mut *mut sbn_table) -> c_int;
    pub fn sbn_table_from_dev(ctx: *mut sbn_ctx, z_dev: *const c_void, len: usize, flags: u32, out: *mut *mut sbn_table) -> c_int;
    pub fn sbn_table_free(ctx: *mut sbn_ctx, t: *mut sbn_table);
    pub fn sbn_table_len(t: *const sbn_table) -> usize;
    pub fn sbn_table_download(ctx: *mut sbn_ctx, t: *const sbn_table, out: *mut u8) -> c_int;
    pub fn sbn_table_read0(ctx: *mut sbn_ctx, t: *const sbn_table, out: *mut u8) -> c_int;
    pub fn sbn_table_read0_many(ctx: *mut sbn_ctx, ts: *const *const sbn_table, count: usize, out: *mut u8) -> c_int;
    pub fn sbn_bind_top(ctx: *mut sbn_ctx, t: *mut sbn_table, r: *const u8) -> c_int;
    pub fn sbn_bind_top_many(ctx: *mut sbn_ctx, ts: *const *mut sbn_table, count: usize, r: *const u8) -> c_int;
    pub fn sbn_sc_eval_cubic(ctx: *mut sbn_ctx, a: *const sbn_table, b: *const sbn_table, c: *const sbn_table, out: *mut u8) -> c_int;
    pub fn sbn_sc_eval_cubic_batched(ctx: *mut sbn_ctx, a: *const *const sbn_table, b: *const *const sbn_table, c: *const *const sbn_table, count: usize, out: *mut u8) -> c_int;
    pub fn sbn_sc_eval_r1cs(ctx: *mut sbn_ctx, tau: *const sbn_table, az: *const sbn_table, bz: *const sbn_table, cz: *const sbn_table, out: *mut u8) -> c_int;
    pub fn sbn_sc_eval_quad(ctx: *mut sbn_ctx, z: *const sbn_table, abc: *const sbn_table, out: *mut u8) -> c_int;
    pub fn sbn_sc_bind_eval_cubic_batched(ctx: *mut sbn_ctx, a: *const *mut sbn_table, b: *const *mut sbn_table, c: *const *mut sbn_table, count: usize, r: *const u8, out: *mut u8) -> c_int;
    pub fn sbn_sc_bind_eval_r1cs(ctx: *mut sbn_ctx, tau: *mut sbn_table, az: *mut sbn_table, bz: *mut sbn_table, cz: *mut sbn_table, r: *const u8, out: *mut u8) -> c_int;
    pub fn sbn_sc_bind_eval_quad(ctx: *mut sbn_ctx, z: *mut sbn_table, abc: *mut sbn_table, r: *const u8, out: *mut u8) -> c_int;
    pub fn sbn_sumcheck_begin(ctx: *mut sbn_ctx, a_par: *const *const sbn_table, b_par: *const *const sbn_table, c_par: *const sbn_table, n_par: usize, a_seq: *const *const sbn_table, b_seq: *const *const sbn_table, c_seq: *const *const sbn_table, n_seq: usize, coeffs: *const u8, out_evals: *mut u8, out: *mut *mut sbn_sumcheck) -> c_int;
    pub fn sbn_sumcheck_begin_eq(ctx: *mut sbn_ctx, a_par: *const *const sbn_table, b_par: *const *const sbn_table, n_par: usize, rand: *const u8, ell: usize, a_seq: *const *const sbn_table, b_seq: *const *const sbn_table, c_seq: *const *const sbn_table, n_seq: usize, coeffs: *const u8, out_evals: *mut u8, out: *mut *mut sbn_sumcheck) -> c_int;
    pub fn sbn_sumcheck_round(ctx: *mut sbn_ctx, st: *mut sbn_sumcheck, r: *const u8, out_evals: *mut u8) -> c_int;
    pub fn sbn_sumcheck_len(st: *const sbn_sumcheck) -> usize;
    pub fn sbn_sumcheck_finish(ctx: *mut sbn_ctx, st: *mut sbn_sumcheck, finals: *mut u8) -> c_int;
    pub fn sbn_sumcheck_free(ctx: *mut sbn_ctx, st: *mut sbn_sumcheck);
    pub fn sbn_transcript_new(label: *const u8, label_len: usize, out: *mut *mut sbn_transcript) -> c_int;
    pub fn sbn_transcript_clone(t: *const sbn_transcript, out: *mut *mut sbn_transcript) -> c_int;
    pub fn sbn_transcript_free(t: *mut sbn_transcript);
    pub fn sbn_transcript_append_message(t: *mut sbn_transcript, label: *const u8, label_len: usize, msg: *const u8, msg_len: usize) -> c_int;
    pub fn sbn_transcript_challenge_bytes(t: *mut sbn_transcript, label: *const u8, label_len: usize, out: *mut u8, out_len: usize) -> c_int;
    pub fn sbn_transcript_challenge_scalar(t: *mut sbn_transcript, label: *const u8, label_len: usize, out: *mut u8) -> c_int;
    pub fn sbn_transcript_state(t: *const sbn_transcript, out: *mut u8) -> c_int;
    pub fn sbn_transcript_from_state(input: *const u8, out: *mut *mut sbn_transcript) -> c_int;
    pub fn sbn_fr_from_wide(input: *const u8, out: *mut u8) -> c_int;
    pub fn sbn_sumcheck_prove(ctx: *mut sbn_ctx, st: *mut sbn_sumcheck, tr: *mut sbn_transcript, claim: *const u8, out_polys: *mut u8, out_r: *mut u8, finals: *mut u8) -> c_int;
    pub fn sbn_product_proof_prove(ctx: *mut sbn_ctx, layers: *const *const sbn_table, n_circ: usize, n_layers: usize, dotp_left: *const *const sbn_table, dotp_right: *const *const sbn_table, dotp_weight: *const *const sbn_table, n_dotp: usize, tr: *mut sbn_transcript, out_polys: *mut u8, out_claims: *mut u8, out_rand: *mut u8, out_claims_final: *mut u8) -> c_int;
    pub fn sbn_eq_evals(ctx: *mut sbn_ctx, r: *const u8, ell: usize, out: *mut *mut sbn_table) -> c_int;
    pub fn sbn_table_dot(ctx: *mut sbn_ctx, a: *const sbn_table, b: *const sbn_table, out: *mut u8) -> c_int;
    pub fn sbn_table_evaluate(ctx: *mut sbn_ctx, z: *const sbn_table, r: *const u8, ell: usize, out: *mut u8) -> c_int;
    pub fn sbn_table_evaluate_many(ctx: *mut sbn_ctx, z: *const *const sbn_table, count: usize, r: *const u8, ell: usize, out: *mut u8) -> c_int;
    pub fn sbn_table_bound(ctx: *mut sbn_ctx, z: *const sbn_table, lvec: *const sbn_table, out: *mut *mut sbn_table) -> c_int;
    pub fn sbn_bullet_begin(ctx: *mut sbn_ctx, g: *const sbn_bases, q_xy: *const u8, a: *const sbn_table, b: *const sbn_table, blind: *const u8, gamma_xy: *mut u8, gamma_is_inf: *mut c_int, out: *mut *mut sbn_bullet) -> c_int;
    pub fn sbn_bullet_begin_scaled(ctx: *mut sbn_ctx, g: *const sbn_bases, q_base_xy: *const u8, q_scale: *const u8, a: *const sbn_table, b: *const sbn_table, blind: *const u8, gamma_xy: *mut u8, gamma_is_inf: *mut c_int, out: *mut *mut sbn_bullet) -> c_int;
    pub fn sbn_bullet_free(ctx: *mut sbn_ctx, st: *mut sbn_bullet);
    pub fn sbn_bullet_len(st: *const sbn_bullet) -> usize;
    pub fn sbn_bullet_cross(ctx: *mut sbn_ctx, st: *mut sbn_bullet, blind_l: *const u8, blind_r: *const u8, l_xy: *mut u8, l_is_inf: *mut c_int, r_xy: *mut u8, r_is_inf: *mut c_int, c_l: *mut u8, c_r: *mut u8) -> c_int;
    pub fn sbn_bullet_fold(ctx: *mut sbn_ctx, st: *mut sbn_bullet, u: *const u8, u_inv: *const u8) -> c_int;
    pub fn sbn_bullet_fold_cross(ctx: *mut sbn_ctx, st: *mut sbn_bullet, u: *const u8, u_inv: *const u8, blind_l: *const u8, blind_r: *const u8, l_xy: *mut u8, l_is_inf: *mut c_int, r_xy: *mut u8, r_is_inf: *mut c_int, c_l: *mut u8, c_r: *mut u8) -> c_int;
    pub fn sbn_bullet_finish(ctx: *mut sbn_ctx, st: *mut sbn_bullet, a_hat: *mut u8, b_hat: *mut u8, g_hat_xy: *mut u8, g_hat_is_inf: *mut c_int) -> c_int;
    pub fn sbn_polyeval_prove(ctx: *mut sbn_ctx, gens: *const sbn_bases, z: *const sbn_table, blinds: *const u8, r: *const u8, ell: usize, zr: *const u8, blind_zr: *const u8, rnd: *const u8, tr: *mut sbn_transcript, out_proof: *mut u8, out_cx_xy: *mut u8, cx_is_inf: *mut c_int, out_cy_xy: *mut u8, cy_is_inf: *mut c_int) -> c_int;
    pub fn sbn_joint_opening_prove(ctx: *mut sbn_ctx, gens: *const sbn_bases, z: *const sbn_table, evals: *const u8, count: usize, label_evals: *const u8, label_evals_len: usize, label_chal: *const u8, label_chal_len: usize, label_claim: *const u8, label_claim_len: usize, r: *const u8, ell_r: usize, rnd: *const u8, tr: *mut sbn_transcript, out_challenges: *mut u8, out_joint_claim: *mut u8, out_proof: *mut u8, out_cx_xy: *mut u8, cx_is_inf: *mut c_int, out_cy_xy: *mut u8, cy_is_inf: *mut c_int) -> c_int;
    pub fn sbn_g1_decompress(ctx: *mut sbn_ctx, in32: *const u8, n: usize, out_xy: *mut u8, out_ok: *mut u8) -> c_int;
    pub fn sbn_bases_from_compressed(ctx: *mut sbn_ctx, in32: *const u8, n: usize, out: *mut *mut sbn_bases, bad_index: *mut usize) -> c_int;
    pub fn sbn_polyeval_verify(ctx: *mut sbn_ctx, gens: *const sbn_bases, comm: *const sbn_bases, r: *const u8, ell: usize, c_zr_xy: *const u8, zr: *const u8, proof: *const u8, tr: *mut sbn_transcript, accepted: *mut c_int) -> c_int;
    pub fn sbn_joint_opening_verify(ctx: *mut sbn_ctx, gens: *const sbn_bases, comm: *const sbn_bases, evals: *const u8, count: usize, label_evals: *const u8, label_evals_len: usize, label_chal: *const u8, label_chal_len: usize, label_claim: *const u8, label_claim_len: usize, r: *const u8, ell_r: usize, proof: *const u8, tr: *mut sbn_transcript, out_challenges: *mut u8, accepted: *mut c_int) -> c_int;
    pub fn sbn_zk_sumcheck_prove_r1cs(ctx: *mut sbn_ctx, tau: *mut sbn_table, az: *mut sbn_table, bz: *mut sbn_table, cz: *mut sbn_table, gens_1: *const sbn_bases, gens_4: *const sbn_bases, claim: *const u8, blind_claim: *const u8, rnd: *const u8, tr: *mut sbn_transcript, out_proof: *mut u8, out_r: *mut u8, out_finals: *mut u8, out_blind: *mut u8) -> c_int;
    pub fn sbn_zk_sumcheck_prove_quad(ctx: *mut sbn_ctx, z: *mut sbn_table, abc: *mut sbn_table, gens_1: *const sbn_bases, gens_3: *const sbn_bases, claim: *const u8, blind_claim: *const u8, rnd: *const u8, tr: *mut sbn_transcript, out_proof: *mut u8, out_r: *mut u8, out_finals: *mut u8, out_blind: *mut u8) -> c_int;
    pub fn sbn_hash_layer(ctx: *mut sbn_ctx, addr_dev: *const c_void, val: *const sbn_table, ts_dev: *const c_void, ts_add: u32, r_hash: *const u8, r_multiset: *const u8, out: *mut *mut sbn_table) -> c_int;
    pub fn sbn_hash_layer_pair(ctx: *mut sbn_ctx, addr_dev: *const c_void, val: *const sbn_table, ts_a_dev: *const c_void, ts_a_add: u32, ts_b_dev: *const c_void, ts_b_add: u32, r_hash: *const u8, r_multiset: *const u8, out_a: *mut *mut sbn_table, out_b: *mut *mut sbn_table) -> c_int;
    pub fn sbn_hash_layer_pair_product(ctx: *mut sbn_ctx, addr_dev: *const c_void, val: *const sbn_table, ts_a_dev: *const c_void, ts_a_add: u32, ts_b_dev: *const c_void, ts_b_add: u32, r_hash: *const u8, r_multiset: *const u8, out_a: *mut *mut sbn_table, out_b: *mut *mut sbn_table, prod_a: *mut *mut sbn_table, prod_b: *mut *mut sbn_table) -> c_int;
    pub fn sbn_product_layer(ctx: *mut sbn_ctx, input: *const sbn_table, out: *mut *mut sbn_table) -> c_int;
    pub fn sbn_product_circuit(ctx: *mut sbn_ctx, input: *const sbn_table, layers: *mut *mut sbn_table, cap: usize, count: *mut usize) -> c_int;
    pub fn sbn_product_circuit_many(ctx: *mut sbn_ctx, ins: *const *const sbn_table, n: usize, layers: *mut *mut sbn_table, cap: usize, count: *mut usize) -> c_int;
    pub fn sbn_table_halves(ctx: *mut sbn_ctx, t: *const sbn_table, left: *mut *mut sbn_table, right: *mut *mut sbn_table) -> c_int;
    pub fn sbn_table_slice(ctx: *mut sbn_ctx, t: *const sbn_table, first: usize, len: usize, out: *mut *mut sbn_table) -> c_int;
    pub fn sbn_gather_merge(ctx: *mut sbn_ctx, mem: *const *const sbn_table, addr_dev: *const *const c_void, count: usize, n: usize, out: *mut *mut sbn_table) -> c_int;
    pub fn sbn_gather_merge_rows(ctx: *mut sbn_ctx, mem: *const *const sbn_table, addr_dev: *const *const c_void, count: usize, n: usize, r: usize, row0: usize, rstep: usize, nrows: usize, out: *mut *mut sbn_table) -> c_int;
    pub fn sbn_commit_table(ctx: *mut sbn_ctx, b: *const sbn_bases, t: *const sbn_table, blinds: *const u8, l: usize, r: usize, out_xy: *mut u8, out_inf: *mut u8) -> c_int;
    pub fn sbn_group_create(devices: *const c_int, n: usize, out: *mut *mut sbn_group) -> c_int;
    pub fn sbn_group_destroy(g: *mut sbn_group);
    pub fn sbn_group_size(g: *const sbn_group) -> usize;
    pub fn sbn_group_ctx(g: *mut sbn_group, i: usize) -> *mut sbn_ctx;
    pub fn sbn_group_last_error(g: *const sbn_group) -> *const c_char;
    pub fn sbn_group_bases_upload(g: *mut sbn_group, g_xy: *const u8, n: usize, h_xy: *const u8, flags: u32, out: *mut *mut sbn_group_bases) -> c_int;
    pub fn sbn_group_gens_new(g: *mut sbn_group, n: usize, label: *const u8, label_len: usize, out_xy: *mut u8, out: *mut *mut sbn_group_bases) -> c_int;
    pub fn sbn_group_bases_precompute(g: *mut sbn_group, gb: *mut sbn_group_bases, max_bytes_per_device: usize, window_bits: *mut c_int) -> c_int;
    pub fn sbn_group_bases_free(g: *mut sbn_group, gb: *mut sbn_group_bases);
    pub fn sbn_group_commit_rows(g: *mut sbn_group, gb: *const sbn_group_bases, z: *const u8, blinds: *const u8, l: usize, r: usize, flags: u32, out_xy: *mut u8, out_inf: *mut u8) -> c_int;
    pub fn sbn_group_commit_rows_dev(g: *mut sbn_group, gb: *const sbn_group_bases, z_dev: *const *const c_void, blinds_dev: *const *const c_void, l: usize, r: usize, flags: u32, out_xy: *mut u8, out_inf: *mut u8) -> c_int;
    pub fn sbn_group_gather_commit(g: *mut sbn_group, gb: *const sbn_group_bases, mem: *const *const sbn_table, addr_dev: *const *const c_void, count: usize, n: usize, l: usize, r: usize, out_xy: *mut u8, out_inf: *mut u8) -> c_int;
    pub fn sbn_group_msm(g: *mut sbn_group, scalars: *const u8, points: *const u8, n: usize, flags: u32, out_xy: *mut u8, out_is_inf: *mut c_int) -> c_int;
    pub fn sbn_group_bases_upload_ranges(g: *mut sbn_group, g_xy: *const u8, n: usize, flags: u32, out: *mut *mut sbn_group_bases) -> c_int;
    pub fn sbn_group_bases_synthetic_ranges(g: *mut sbn_group, n: usize, s0: *const u8, d: *const u8, out: *mut *mut sbn_group_bases) -> c_int;
    pub fn sbn_group_range(gb: *const sbn_group_bases, device: usize, lo: *mut usize, hi: *mut usize);
    pub fn sbn_group_msm_bases(g: *mut sbn_group, gb: *const sbn_group_bases, scalars: *const u8, n: usize, flags: u32, out_xy: *mut u8, out_is_inf: *mut c_int) -> c_int;
    pub fn sbn_group_msm_bases_dev(g: *mut sbn_group, gb: *const sbn_group_bases, scalars_dev: *const *const c_void, flags: u32, out_xy: *mut u8, out_is_inf: *mut c_int) -> c_int;
    pub fn sbn_kzg_srs_upload(ctx: *mut sbn_ctx, powers_xy: *const u8, n: usize, flags: u32, out: *mut *mut sbn_bases) -> c_int;
    pub fn sbn_kzg_srs_from_tau(ctx: *mut sbn_ctx, tau: *const u8, n: usize, out: *mut *mut sbn_bases) -> c_int;
    pub fn sbn_kzg_commit(ctx: *mut sbn_ctx, srs: *const sbn_bases, t: *const sbn_table, n: usize, out_xy: *mut u8, out_is_inf: *mut c_int) -> c_int;
    pub fn sbn_poly_div_linear(ctx: *mut sbn_ctx, t: *const sbn_table, n: usize, z: *const u8, eval: *mut u8, q: *mut *mut sbn_table) -> c_int;
    pub fn sbn_kzg_open(ctx: *mut sbn_ctx, srs: *const sbn_bases, t: *const sbn_table, n: usize, z: *const u8, eval: *mut u8, proof_xy: *mut u8, proof_is_inf: *mut c_int) -> c_int;
    pub fn sbn_kzg_open_batched(ctx: *mut sbn_ctx, srs: *const sbn_bases, ts: *const *const sbn_table, ns: *const usize, count: usize, z: *const u8, gamma: *const u8, evals: *mut u8, proof_xy: *mut u8, proof_is_inf: *mut c_int) -> c_int;
    pub fn sbn_r1cs_upload(ctx: *mut sbn_ctx, num_cons: usize, num_vars: usize, rows: *const *const u32, cols: *const *const u32, vals: *const *const u8, nnz: *const usize, flags: u32, out: *mut *mut sbn_r1cs) -> c_int;
    pub fn sbn_r1cs_free(ctx: *mut sbn_ctx, m: *mut sbn_r1cs);
    pub fn sbn_r1cs_multiply(ctx: *mut sbn_ctx, m: *const sbn_r1cs, z: *const sbn_table, az: *mut *mut sbn_table, bz: *mut *mut sbn_table, cz: *mut *mut sbn_table) -> c_int;
    pub fn sbn_r1cs_eval_table(ctx: *mut sbn_ctx, m: *const sbn_r1cs, rx: *const u8, ell_x: usize, ra: *const u8, rb: *const u8, rc: *const u8, out: *mut *mut sbn_table) -> c_int;
    pub fn sbn_r1cs_evaluate(ctx: *mut sbn_ctx, m: *const sbn_r1cs, rx: *const u8, ell_x: usize, ry: *const u8, ell_y: usize, out: *mut u8) -> c_int;
    pub fn sbn_r1cs_proof_sizes(num_cons: usize, num_vars: usize, rnd_scalars: *mut usize, proof_bytes: *mut usize) -> c_int;
    pub fn sbn_r1cs_proof_prove(ctx: *mut sbn_ctx, inst: *const sbn_r1cs, vars: *const sbn_table, input: *const u8, num_inputs: usize, gens_pc: *const sbn_bases, gens_3: *const sbn_bases, gens_4: *const sbn_bases, rnd: *const u8, tr: *mut sbn_transcript, out_proof: *mut u8, out_rx: *mut u8, out_ry: *mut u8) -> c_int;
    pub fn sbn_zk_sumcheck_verify(ctx: *mut sbn_ctx, gens_1: *const sbn_bases, gens_n: *const sbn_bases, comm_claim_xy: *const u8, num_rounds: usize, degree_bound: usize, proof: *const u8, tr: *mut sbn_transcript, out_r: *mut u8, out_comm_eval_xy: *mut u8, accepted: *mut c_int) -> c_int;
    pub fn sbn_r1cs_proof_verify(ctx: *mut sbn_ctx, num_cons: usize, num_vars: usize, input: *const u8, num_inputs: usize, evals: *const u8, gens_pc: *const sbn_bases, gens_3: *const sbn_bases, gens_4: *const sbn_bases, proof: *const u8, tr: *mut sbn_transcript, out_rx: *mut u8, out_ry: *mut u8, accepted: *mut c_int) -> c_int;
    pub fn sbn_g1_small_sums(ctx: *mut sbn_ctx, points_xy: *const u8, scalars: *const u8, counts: *const u32, nsums: usize, out_xy: *mut u8, out_is_inf: *mut u8) -> c_int;
    pub fn sbn_sparse_eval_verify(ctx: *mut sbn_ctx, num_vars_x: usize, num_vars_y: usize, num_ops: usize, num_cells: usize, batch: usize, comm_ops: *const sbn_bases, comm_mem: *const sbn_bases, rx: *const u8, ry: *const u8, evals: *const u8, gens_ops: *const sbn_bases, gens_mem: *const sbn_bases, gens_derefs: *const sbn_bases, proof: *const u8, tr: *mut sbn_transcript, accepted: *mut c_int) -> c_int;
    pub fn sbn_dense_build(ctx: *mut sbn_ctx, num_vars_x: usize, num_vars_y: usize, rows: *const *const u32, cols: *const *const u32, vals: *const *const u8, nnz: *const usize, batch: usize, flags: u32, out: *mut *mut sbn_dense) -> c_int;
    pub fn sbn_dense_free(ctx: *mut sbn_ctx, d: *mut sbn_dense);
    pub fn sbn_dense_num_ops(d: *const sbn_dense) -> usize;
    pub fn sbn_dense_num_cells(d: *const sbn_dense) -> usize;
    pub fn sbn_dense_batch(d: *const sbn_dense) -> usize;
    pub fn sbn_dense_addr_dev(d: *const sbn_dense, side: c_int, k: usize) -> *const c_void;
    pub fn sbn_dense_read_ts_dev(d: *const sbn_dense, side: c_int, k: usize) -> *const c_void;
    pub fn sbn_dense_audit_ts_dev(d: *const sbn_dense, side: c_int) -> *const c_void;
    pub fn sbn_dense_comb_ops(d: *const sbn_dense) -> *const sbn_table;
    pub fn sbn_dense_comb_mem(d: *const sbn_dense) -> *const sbn_table;
    pub fn sbn_sparse_eval_sizes(num_vars_x: usize, num_vars_y: usize, num_ops: usize, batch: usize, rnd_scalars: *mut usize, proof_bytes: *mut usize) -> c_int;
    pub fn sbn_sparse_eval_prove(ctx: *mut sbn_ctx, dense: *const sbn_dense, rx: *const u8, nx: usize, ry: *const u8, ny: usize, evals: *const u8, gens_ops: *const sbn_bases, gens_mem: *const sbn_bases, gens_derefs: *const sbn_bases, rnd: *const u8, tr: *mut sbn_transcript, out_proof: *mut u8) -> c_int;
    pub fn sbn_derefs_key_build(ctx: *mut sbn_ctx, dense: *const sbn_dense, srs: *const sbn_bases, out: *mut *mut sbn_derefs_key) -> c_int;
    pub fn sbn_derefs_key_free(ctx: *mut sbn_ctx, key: *mut sbn_derefs_key);
    pub fn sbn_derefs_key_len(key: *const sbn_derefs_key) -> usize;
    pub fn sbn_derefs_key_download(ctx: *mut sbn_ctx, key: *const sbn_derefs_key, first: usize, count: usize, out_cell: *mut u32, out_xy: *mut u8) -> c_int;
    pub fn sbn_derefs_key_commit(ctx: *mut sbn_ctx, key: *const sbn_derefs_key, mem_rx: *const sbn_table, mem_ry: *const sbn_table, out_xy: *mut u8, out_is_inf: *mut c_int) -> c_int;
    pub fn sbn_sparse_eval_kzg_sizes(num_vars_x: usize, num_vars_y: usize, num_ops: usize, batch: usize, rnd_scalars: *mut usize, proof_bytes: *mut usize) -> c_int;
    pub fn sbn_sparse_eval_prove_kzg(ctx: *mut sbn_ctx, dense: *const sbn_dense, rx: *const u8, nx: usize, ry: *const u8, ny: usize, evals: *const u8, gens_ops: *const sbn_bases, gens_mem: *const sbn_bases, srs: *const sbn_bases, key: *const sbn_derefs_key, rnd: *const u8, tr: *mut sbn_transcript, out_proof: *mut u8) -> c_int;
    pub fn sbn_g2_prepare(ctx: *mut sbn_ctx, q_xy: *const u8, flags: u32, out: *mut *mut sbn_g2_lines) -> c_int;
    pub fn sbn_g2_lines_free(ctx: *mut sbn_ctx, l: *mut sbn_g2_lines);
    pub fn sbn_pairing_products(ctx: *mut sbn_ctx, p_xy: *const u8, q: *const *const sbn_g2_lines, counts: *const u32, nchecks: usize, out_is_one: *mut u8, out_gt: *mut u8) -> c_int;
    pub fn sbn_kzg_verify(ctx: *mut sbn_ctx, g2: *const sbn_g2_lines, tau_g2: *const sbn_g2_lines, comm_xy: *const u8, z: *const u8, eval: *const u8, proof_xy: *const u8, accepted: *mut c_int) -> c_int;
    pub fn sbn_kzg_verify_batched(ctx: *mut sbn_ctx, g2: *const sbn_g2_lines, tau_g2: *const sbn_g2_lines, comms_xy: *const u8, count: usize, z: *const u8, gamma: *const u8, evals: *const u8, proof_xy: *const u8, accepted: *mut c_int) -> c_int;
    pub fn sbn_sparse_eval_verify_kzg(ctx: *mut sbn_ctx, num_vars_x: usize, num_vars_y: usize, num_ops: usize, num_cells: usize, batch: usize, comm_ops: *const sbn_bases, comm_mem: *const sbn_bases, rx: *const u8, ry: *const u8, evals: *const u8, gens_ops: *const sbn_bases, gens_mem: *const sbn_bases, g2: *const sbn_g2_lines, tau_g2: *const sbn_g2_lines, proof: *const u8, tr: *mut sbn_transcript, accepted: *mut c_int) -> c_int;
    pub fn sbn_r1cs_is_sat(ctx: *mut sbn_ctx, inst: *const sbn_r1cs, vars: *const sbn_table, input: *const u8, num_inputs: usize, sat: *mut c_int, num_bad: *mut u64, first_bad: *mut u64) -> c_int;
    pub fn sbn_snark_gens_new(ctx: *mut sbn_ctx, num_cons: usize, num_vars: usize, num_inputs: usize, num_nz_entries: usize, out: *mut *mut sbn_snark_gens) -> c_int;
    pub fn sbn_snark_gens_get(gens: *const sbn_snark_gens, which: c_int) -> *const sbn_bases;
    pub fn sbn_snark_gens_free(ctx: *mut sbn_ctx, gens: *mut sbn_snark_gens);
    pub fn sbn_snark_encode(ctx: *mut sbn_ctx, num_cons: usize, num_vars: usize, num_inputs: usize, rows: *const *const u32, cols: *const *const u32, vals: *const *const u8, nnz: *const usize, flags: u32, gens: *const sbn_snark_gens, out: *mut *mut sbn_snark_key) -> c_int;
    pub fn sbn_snark_key_from_comm(ctx: *mut sbn_ctx, comm: *const u8, len: usize, out: *mut *mut sbn_snark_key) -> c_int;
    pub fn sbn_snark_key_comm(key: *const sbn_snark_key, out: *mut u8, cap: usize, len: *mut usize) -> c_int;
    pub fn sbn_snark_key_dense(key: *const sbn_snark_key) -> *const sbn_dense;
    pub fn sbn_snark_key_free(ctx: *mut sbn_ctx, key: *mut sbn_snark_key);
    pub fn sbn_snark_sizes(key: *const sbn_snark_key, kzg: c_int, rnd_scalars: *mut usize, proof_bytes: *mut usize) -> c_int;
    pub fn sbn_snark_is_sat(ctx: *mut sbn_ctx, key: *const sbn_snark_key, vars: *const sbn_table, input: *const u8, num_inputs: usize, sat: *mut c_int, num_bad: *mut u64, first_bad: *mut u64) -> c_int;
    pub fn sbn_snark_prove(ctx: *mut sbn_ctx, key: *const sbn_snark_key, vars: *const sbn_table, input: *const u8, num_inputs: usize, gens: *const sbn_snark_gens, flags: u32, rnd: *const u8, tr: *mut sbn_transcript, out_proof: *mut u8) -> c_int;
    pub fn sbn_snark_verify(ctx: *mut sbn_ctx, key: *const sbn_snark_key, input: *const u8, num_inputs: usize, gens: *const sbn_snark_gens, proof: *const u8, proof_len: usize, tr: *mut sbn_transcript, accepted: *mut c_int) -> c_int;
    pub fn sbn_snark_prove_kzg(ctx: *mut sbn_ctx, key: *const sbn_snark_key, vars: *const sbn_table, input: *const u8, num_inputs: usize, gens: *const sbn_snark_gens, srs: *const sbn_bases, derefs_key: *const sbn_derefs_key, flags: u32, rnd: *const u8, tr: *mut sbn_transcript, out_proof: *mut u8) -> c_int;
    pub fn sbn_snark_verify_kzg(ctx: *mut sbn_ctx, key: *const sbn_snark_key, input: *const u8, num_inputs: usize, gens: *const sbn_snark_gens, g2: *const sbn_g2_lines, tau_g2: *const sbn_g2_lines, proof: *const u8, proof_len: usize, tr: *mut sbn_transcript, accepted: *mut c_int) -> c_int;
    pub fn sbn_nizk_gens_new(ctx: *mut sbn_ctx, num_cons: usize, num_vars: usize, num_inputs: usize, out: *mut *mut sbn_snark_gens) -> c_int;
    pub fn sbn_nizk_instance_new(ctx: *mut sbn_ctx, num_cons: usize, num_vars: usize, num_inputs: usize, rows: *const *const u32, cols: *const *const u32, vals: *const *const u8, nnz: *const usize, flags: u32, digest: *const u8, digest_len: usize, out: *mut *mut sbn_nizk_inst) -> c_int;
    pub fn sbn_nizk_instance_free(ctx: *mut sbn_ctx, inst: *mut sbn_nizk_inst);
    pub fn sbn_nizk_instance_r1cs(inst: *const sbn_nizk_inst) -> *const sbn_r1cs;
    pub fn sbn_nizk_sizes(inst: *const sbn_nizk_inst, rnd_scalars: *mut usize, proof_bytes: *mut usize) -> c_int;
    pub fn sbn_nizk_is_sat(ctx: *mut sbn_ctx, inst: *const sbn_nizk_inst, vars: *const sbn_table, input: *const u8, num_inputs: usize, sat: *mut c_int, num_bad: *mut u64, first_bad: *mut u64) -> c_int;
    pub fn sbn_nizk_prove(ctx: *mut sbn_ctx, inst: *const sbn_nizk_inst, vars: *const sbn_table, input: *const u8, num_inputs: usize, gens: *const sbn_snark_gens, flags: u32, rnd: *const u8, tr: *mut sbn_transcript, out_proof: *mut u8) -> c_int;
    pub fn sbn_nizk_verify(ctx: *mut sbn_ctx, inst: *const sbn_nizk_inst, input: *const u8, num_inputs: usize, gens: *const sbn_snark_gens, proof: *const u8, proof_len: usize, tr: *mut sbn_transcript, accepted: *mut c_int) -> c_int;
    pub fn sbn_circom_r1cs_load(ctx: *mut sbn_ctx, file: *const u8, len: usize, out: *mut *mut sbn_circom_r1cs) -> c_int;
    pub fn sbn_circom_r1cs_info(f: *const sbn_circom_r1cs, out: *mut sbn_circom_info) -> c_int;
    pub fn sbn_circom_r1cs_download(ctx: *mut sbn_ctx, f: *const sbn_circom_r1cs, m: c_int, rows: *mut u32, cols: *mut u32, vals: *mut u8) -> c_int;
    pub fn sbn_circom_r1cs_free(ctx: *mut sbn_ctx, f: *mut sbn_circom_r1cs);
    pub fn sbn_r1cs_from_circom(ctx: *mut sbn_ctx, f: *const sbn_circom_r1cs, out: *mut *mut sbn_r1cs) -> c_int;
    pub fn sbn_nizk_instance_from_circom(ctx: *mut sbn_ctx, f: *const sbn_circom_r1cs, digest: *const u8, digest_len: usize, out: *mut *mut sbn_nizk_inst) -> c_int;
    pub fn sbn_snark_encode_circom(ctx: *mut sbn_ctx, f: *const sbn_circom_r1cs, gens: *const sbn_snark_gens, out: *mut *mut sbn_snark_key) -> c_int;
    pub fn sbn_circom_wtns_load(ctx: *mut sbn_ctx, file: *const u8, len: usize, num_inputs: usize, vars: *mut *mut sbn_table, input: *mut u8, num_witness: *mut usize) -> c_int;
    pub fn sbn_circom_r1cs_digest(ctx: *mut sbn_ctx, f: *const sbn_circom_r1cs, out: *mut u8) -> c_int;
    pub fn sbn_random_tape_new(name: *const u8, name_len: usize, init: *const u8, out: *mut *mut sbn_random_tape) -> c_int;
    pub fn sbn_random_tape_scalars(tape: *mut sbn_random_tape, label: *const u8, label_len: usize, n: usize, out: *mut u8) -> c_int;
    pub fn sbn_random_tape_free(tape: *mut sbn_random_tape);
    pub fn sbn_random_tape_last_error(tape: *const sbn_random_tape) -> *const c_char;
    pub fn sbn_zk_sumcheck_draw_rnd(num_rounds: usize, n: usize, tape: *mut sbn_random_tape, out: *mut u8, out_scalars: usize) -> c_int;
    pub fn sbn_polyeval_draw_rnd(ell: usize, tape: *mut sbn_random_tape, out: *mut u8, out_scalars: usize) -> c_int;
    pub fn sbn_r1cs_proof_draw_rnd(num_cons: usize, num_vars: usize, tape: *mut sbn_random_tape, out: *mut u8, out_scalars: usize) -> c_int;
    pub fn sbn_sparse_eval_draw_rnd(num_vars_x: usize, num_vars_y: usize, num_ops: usize, batch: usize, kzg: c_int, tape: *mut sbn_random_tape, out: *mut u8, out_scalars: usize) -> c_int;
    pub fn sbn_snark_draw_rnd(key: *const sbn_snark_key, kzg: c_int, tape: *mut sbn_random_tape, out: *mut u8, out_scalars: usize) -> c_int;
    pub fn sbn_nizk_draw_rnd(inst: *const sbn_nizk_inst, tape: *mut sbn_random_tape, out: *mut u8, out_scalars: usize) -> c_int;
    pub fn sbn_kzg_srs_load(ctx: *mut sbn_ctx, bytes: *const u8, len: usize, flags: u32, out_srs: *mut *mut sbn_bases, out_g2: *mut *mut sbn_g2_lines, out_tau_g2: *mut *mut sbn_g2_lines, out_g2_xy: *mut u8, bad_index: *mut usize) -> c_int;
    pub fn sbn_kzg_srs_check(ctx: *mut sbn_ctx, srs: *const sbn_bases, g2: *const sbn_g2_lines, tau_g2: *const sbn_g2_lines, rho: *const u8, consistent: *mut c_int) -> c_int;
    pub fn sbn_kzg_srs_save(ctx: *mut sbn_ctx, srs: *const sbn_bases, g2_xy: *const u8, tau_g2_xy: *const u8, flags: u32, out: *mut u8, cap: usize, out_len: *mut usize) -> c_int;
    pub fn sbn_kzg_srs_g2_from_tau(tau: *const u8, out_g2_xy: *mut u8, out_tau_g2_xy: *mut u8) -> c_int;
    pub fn sbn_ptau_scan(bytes: *const u8, len: usize, out: *mut sbn_ptau_info) -> c_int;
    pub fn sbn_kzg_srs_load_ptau(ctx: *mut sbn_ctx, bytes: *const u8, len: usize, n: usize, flags: u32, out_srs: *mut *mut sbn_bases, out_g2: *mut *mut sbn_g2_lines, out_tau_g2: *mut *mut sbn_g2_lines, out_g2_xy: *mut u8, bad_index: *mut usize) -> c_int;
    pub fn sbn_prof_enable(ctx: *mut sbn_ctx, on: c_int) -> c_int;
    pub fn sbn_prof_reset(ctx: *mut sbn_ctx) -> c_int;
    pub fn sbn_prof_count(ctx: *mut sbn_ctx) -> c_int;
    pub fn sbn_prof_get(ctx: *mut sbn_ctx, i: c_int, name: *mut *const c_char, total_ms: *mut f64, launches: *mut u64) -> c_int;
    pub fn sbn_prof_last_job(ctx: *mut sbn_ctx, out: *mut u64) -> c_int;
    pub fn sbn_prof_last_acc(ctx: *mut sbn_ctx, out: *mut u64) -> c_int;
    pub fn sbn_prof_last_polyeval(ctx: *mut sbn_ctx, out_us: *mut f64) -> c_int;
    // GENERATED-END
}

// ---- errors: the reference's prover functions are infallible (assert! / panic on misuse, errors.rs:19-31 is verifier-only) ----
pub fn check(rc: c_int) {
    if rc != SBN_OK {
        let msg = unsafe { std::ffi::CStr::from_ptr(sbn_last_error(ctx())) }.to_string_lossy().into_owned();
        panic!("sbn254 (rc = {}): {}", rc, msg);
    }
}
pub fn check_group(rc: c_int) {
    if rc != SBN_OK {
        let msg = unsafe { std::ffi::CStr::from_ptr(sbn_group_last_error(group())) }.to_string_lossy().into_owned();
        panic!("sbn254 group (rc = {}): {}", rc, msg);
    }
}

// ---- one context per process; the library serialises calls on a context with a mutex (hyrax.rs:259-261 may enter from rayon workers) ----
struct CtxPtr(*mut sbn_ctx);
unsafe impl Send for CtxPtr {}
unsafe impl Sync for CtxPtr {}
pub fn ctx() -> *mut sbn_ctx {
    static CTX: OnceLock<CtxPtr> = OnceLock::new();
    CTX.get_or_init(|| {
        let dev: c_int = std::env::var("SBN_DEVICE").ok().and_then(|s| s.parse().ok()).unwrap_or(0);
        let mut c = null_mut();
        let rc = unsafe { sbn_ctx_create(dev, &mut c) };
        assert_eq!(rc, SBN_OK, "sbn254: no usable gfx950 device (there is no CPU fallback in the library; build without --features hip)");
        CtxPtr(c)
    })
    .0
}
/// all devices listed in SBN_DEVICES (e.g. "0,1,2,3,4,5,6,7"); a single-device list when the variable is absent
struct GroupPtr(*mut sbn_group);
unsafe impl Send for GroupPtr {}
unsafe impl Sync for GroupPtr {}
pub fn group() -> *mut sbn_group {
    static G: OnceLock<GroupPtr> = OnceLock::new();
    G.get_or_init(|| {
        let devs: Vec<c_int> = std::env::var("SBN_DEVICES").ok().map(|s| s.split(',').filter_map(|x| x.trim().parse().ok()).collect()).unwrap_or_else(|| vec![0]);
        let mut g = null_mut();
        let rc = unsafe { sbn_group_create(devs.as_ptr(), devs.len(), &mut g) };
        assert_eq!(rc, SBN_OK, "sbn254: sbn_group_create failed for devices {:?}", devs);
        GroupPtr(g)
    })
    .0
}
pub fn group_size() -> usize { unsafe { sbn_group_size(group()) } }

// ---- owned handles --------------------------------------------------------------------------------------------------
/// device-resident generator table (MultiCommitGens.{G_affine, h_affine}, commitments.rs:17-27)
pub struct Bases(pub *mut sbn_bases);
unsafe impl Send for Bases {}
unsafe impl Sync for Bases {}
impl Drop for Bases { fn drop(&mut self) { if !self.0.is_null() { unsafe { sbn_bases_free(ctx(), self.0) } } } }
impl std::fmt::Debug for Bases { fn fmt(&self, f: &mut std::fmt::Formatter<'_>) -> std::fmt::Result { write!(f, "Bases({:p})", self.0) } }

/// the same generator set on every device of the group
pub struct GroupBases(pub *mut sbn_group_bases);
unsafe impl Send for GroupBases {}
unsafe impl Sync for GroupBases {}
impl Drop for GroupBases { fn drop(&mut self) { if !self.0.is_null() { unsafe { sbn_group_bases_free(group(), self.0) } } } }
impl std::fmt::Debug for GroupBases { fn fmt(&self, f: &mut std::fmt::Formatter<'_>) -> std::fmt::Result { write!(f, "GroupBases({:p})", self.0) } }

/// device-resident Fr table (DensePolynomial.Z, hyrax.rs:155-160)
pub struct Table(pub *mut sbn_table);
impl Drop for Table { fn drop(&mut self) { if !self.0.is_null() { unsafe { sbn_table_free(ctx(), self.0) } } } }
impl Table {
    pub fn upload(z: &[Scalar]) -> Table {
        let bytes = scalars_mont_bytes(z);
        let mut t = null_mut();
        check(unsafe { sbn_table_upload(ctx(), bytes.as_ptr(), z.len(), SBN_SCALARS_MONT, &mut t) });
        Table(t)
    }
    pub fn of(p: &DensePolynomial) -> Table { Table::upload(&p.vec()[..p.len()]) }
    pub fn len(&self) -> usize { unsafe { sbn_table_len(self.0) } }
    pub fn is_empty(&self) -> bool { self.len() == 0 }
}
struct SumcheckState(*mut sbn_sumcheck);
impl Drop for SumcheckState { fn drop(&mut self) { if !self.0.is_null() { unsafe { sbn_sumcheck_free(ctx(), self.0) } } } }
struct BulletState(*mut sbn_bullet);
impl Drop for BulletState { fn drop(&mut self) { if !self.0.is_null() { unsafe { sbn_bullet_free(ctx(), self.0) } } } }

/// the lazily created device twin of a `MultiCommitGens` (the field `dev` the commitments.rs patch adds next to the
/// `#[serde(skip)]` affine cache): shared by clones, rebuilt after deserialisation, dropped with the last clone
#[derive(Clone, Debug, Default)]
pub struct GensDev {
    one: Arc<OnceLock<Bases>>,
    all: Arc<OnceLock<GroupBases>>,
}
impl GensDev {
    pub fn bases(&self, gens: &MultiCommitGens) -> *const sbn_bases {
        self.one.get_or_init(|| {
            let g: Vec<u8> = gens.G_affine.iter().flat_map(point_xy_mont).collect();
            let h = point_xy_mont(&gens.h_affine);
            let mut b = null_mut();
            check(unsafe { sbn_bases_upload(ctx(), g.as_ptr(), gens.n, h.as_ptr(), SBN_POINTS_MONT, &mut b) });
            // a generator set that serves every proof of a circuit gets its fixed-base lookup table (SBN_LOOKUP_GB, default 0 = bucket method)
            let gb: usize = std::env::var("SBN_LOOKUP_GB").ok().and_then(|s| s.parse().ok()).unwrap_or(0);
            if gb > 0 && gens.n >= 1024 { let mut cbits = 0; check(unsafe { sbn_bases_precompute(ctx(), b, gb << 30, &mut cbits) }); }
            Bases(b)
        })
        .0
    }
    pub fn group_bases(&self, gens: &MultiCommitGens) -> *const sbn_group_bases {
        self.all.get_or_init(|| {
            let g: Vec<u8> = gens.G_affine.iter().flat_map(point_xy_mont).collect();
            let h = point_xy_mont(&gens.h_affine);
            let mut b = null_mut();
            check_group(unsafe { sbn_group_bases_upload(group(), g.as_ptr(), gens.n, h.as_ptr(), SBN_POINTS_MONT, &mut b) });
            GroupBases(b)
        })
        .0
    }
}

// ---- data conversion at the boundary ---------------------------------------------------------------------------------
// ark-ff keeps Fr / Fq as Montgomery limbs (R = 2^256), 4 x u64 little-endian: `Fp(pub BigInt<4>, PhantomData)`, `BigInt(pub [u64; 4])`.
// The library takes exactly those 32 bytes with SBN_SCALARS_MONT / SBN_POINTS_MONT (it converts with one product per element as
// it reads them).  `Scalar` is `#[repr(transparent)]` over `Fr` after patches/0002; whether `Fr` itself lies in memory as its four
// limbs is checked ONCE at run time (below) — if it ever does not, the slice is copied limb by limb instead of being reinterpreted.
fn limbs_le(x: &[u64; 4]) -> [u8; 32] {
    let mut o = [0u8; 32];
    for (i, l) in x.iter().enumerate() { o[8 * i..8 * i + 8].copy_from_slice(&l.to_le_bytes()); }
    o
}
fn scalar_layout_is_raw_limbs() -> bool {
    static OK: OnceLock<bool> = OnceLock::new();
    *OK.get_or_init(|| {
        if std::mem::size_of::<Scalar>() != 32 || std::mem::align_of::<Scalar>() > 8 || cfg!(target_endian = "big") { return false; }
        let probe = [Scalar::from_u64(0x0123_4567_89ab_cdef), Scalar::one(), Scalar::zero() - Scalar::one()];
        let raw = unsafe { core::slice::from_raw_parts(probe.as_ptr() as *const u8, 32 * probe.len()) };
        probe.iter().enumerate().all(|(i, s)| raw[32 * i..32 * i + 32] == limbs_le(&(s.0).0 .0))
    })
}
/// the slice as the library's SBN_SCALARS_MONT input: borrowed when the layout allows it (no copy of a 1 GiB matrix), copied otherwise
pub fn scalars_mont_bytes(s: &[Scalar]) -> Cow<'_, [u8]> {
    if scalar_layout_is_raw_limbs() {
        Cow::Borrowed(unsafe { core::slice::from_raw_parts(s.as_ptr() as *const u8, 32 * s.len()) })
    } else {
        Cow::Owned(s.iter().flat_map(|x| limbs_le(&(x.0).0 .0)).collect())
    }
}
/// canonical 32-byte little-endian encodings (Scalar::to_bytes, scalar.rs:75-84): challenges, blinds, coefficients
pub fn scalars_canonical(s: &[Scalar]) -> Vec<u8> { s.iter().flat_map(|x| x.to_bytes()).collect() }
/// a canonical 32-byte little-endian value coming back from the device
pub fn sc(b: &[u8]) -> Scalar {
    let a: [u8; 32] = b[..32].try_into().unwrap();
    Scalar::from_bytes(&a).expect("sbn254 returned a non-canonical scalar")
}
/// {x, y, infinity} -> x || y in ark-ff's Montgomery limbs; all-zero for infinity
pub fn point_xy_mont(p: &G1Affine) -> [u8; 64] {
    let mut o = [0u8; 64];
    if !p.is_zero() {
        o[..32].copy_from_slice(&limbs_le(&(p.x.0).0));
        o[32..].copy_from_slice(&limbs_le(&(p.y.0).0));
    }
    o
}
/// canonical x || y (what every entry point returns) -> GroupElement
pub fn group_from_xy(xy: &[u8], inf: bool) -> GroupElement {
    if inf { return GroupElement::identity(); }
    let x = Fq::from_le_bytes_mod_order(&xy[..32]);
    let y = Fq::from_le_bytes_mod_order(&xy[32..64]);
    GroupElement::from_affine(G1Affine::new_unchecked(x, y))
}
fn affine_of(g: &GroupElement) -> G1Affine { g.inner().into_affine() }

// ---- B1: single MSM (group.rs:143-158, 171-175) -----------------------------------------------------------------------
/// `None` when the call should stay on arkworks (tiny MSMs, length mismatch: the reference maps that to the identity)
pub fn msm_affine(scalars: &[Scalar], points: &[G1Affine]) -> Option<GroupElement> {
    if scalars.len() != points.len() || scalars.len() < MIN_GPU_MSM { return None; }
    let pts: Vec<u8> = points.iter().flat_map(point_xy_mont).collect();
    let sb = scalars_mont_bytes(scalars);
    let mut xy = [0u8; 64];
    let mut inf: c_int = 0;
    if group_size() > 1 && scalars.len() >= (1 << 22) {
        // a LARGE MSM (config 4): contiguous base-point ranges, one per device, N partial sums folded on the host
        check_group(unsafe { sbn_group_msm(group(), sb.as_ptr(), pts.as_ptr(), scalars.len(), SBN_SCALARS_MONT | SBN_POINTS_MONT, xy.as_mut_ptr(), &mut inf) });
    } else {
        check(unsafe { sbn_msm(ctx(), sb.as_ptr(), pts.as_ptr(), scalars.len(), SBN_SCALARS_MONT | SBN_POINTS_MONT, xy.as_mut_ptr(), &mut inf) });
    }
    Some(group_from_xy(&xy, inf != 0))
}
/// vartime_multiscalar_mul takes projective points; the n Jacobian triples are normalised on the device (group.rs:153 inverts per point)
pub fn msm_projective(scalars: &[Scalar], points: &[G1Projective]) -> Option<GroupElement> {
    if scalars.len() != points.len() || scalars.len() < MIN_GPU_MSM { return None; }
    let mut xyz = Vec::with_capacity(96 * points.len());
    for p in points {
        xyz.extend_from_slice(&limbs_le(&(p.x.0).0)); xyz.extend_from_slice(&limbs_le(&(p.y.0).0)); xyz.extend_from_slice(&limbs_le(&(p.z.0).0));
    }
    let sb = scalars_mont_bytes(scalars);
    let mut xy = [0u8; 64];
    let mut inf: c_int = 0;
    check(unsafe { sbn_msm_jacobian(ctx(), sb.as_ptr(), xyz.as_ptr(), scalars.len(), SBN_SCALARS_MONT | SBN_POINTS_MONT, xy.as_mut_ptr(), &mut inf) });
    Some(group_from_xy(&xy, inf != 0))
}

// ---- B2: Pedersen / Hyrax commitments (commitments.rs:144-154, hyrax.rs:253-308) ----------------------------------------
/// <[Scalar] as Commitments>::commit: MSM(self || blind, G || h) — one row
pub fn commit_row(scalars: &[Scalar], blind: &Scalar, gens: &MultiCommitGens) -> Option<GroupElement> {
    assert_eq!(gens.n, scalars.len());                                          // commitments.rs:146
    if scalars.len() < MIN_GPU_MSM { return None; }
    let sb = scalars_mont_bytes(scalars);
    let bb = scalars_mont_bytes(core::slice::from_ref(blind));
    let mut xy = [0u8; 64];
    let mut inf = [0u8; 1];
    check(unsafe { sbn_commit_rows(ctx(), gens.dev.bases(gens), sb.as_ptr(), bb.as_ptr(), 1, scalars.len(), SBN_SCALARS_MONT, xy.as_mut_ptr(), inf.as_mut_ptr()) });
    Some(group_from_xy(&xy, inf[0] != 0))
}
/// DensePolynomial::commit_inner: ONE call for the L x R matrix (the reference spawns L rayon tasks, each cloning R bases).
/// With several devices the rows are dealt i mod N over the group (rows are independent: no reduction).
pub fn commit_rows(z: &[Scalar], blinds: &[Scalar], gens: &MultiCommitGens) -> Vec<GroupElement> {
    let l = blinds.len();
    let r = z.len() / l;
    assert_eq!(l * r, z.len());                                                 // hyrax.rs:257
    assert_eq!(gens.n, r);                                                      // commitments.rs:146
    let all_zero = blinds.iter().all(|b| *b == Scalar::zero());                  // random_tape == None (hyrax.rs:301-305)
    let zb = scalars_mont_bytes(z);
    let bb = scalars_mont_bytes(blinds);
    let bp = if all_zero { null() } else { bb.as_ptr() };
    let mut xy = vec![0u8; 64 * l];
    let mut inf = vec![0u8; l];
    if group_size() > 1 && l >= 2 * group_size() {
        check_group(unsafe { sbn_group_commit_rows(group(), gens.dev.group_bases(gens), zb.as_ptr(), bp, l, r, SBN_SCALARS_MONT, xy.as_mut_ptr(), inf.as_mut_ptr()) });
    } else {
        check(unsafe { sbn_commit_rows(ctx(), gens.dev.bases(gens), zb.as_ptr(), bp, l, r, SBN_SCALARS_MONT, xy.as_mut_ptr(), inf.as_mut_ptr()) });
    }
    (0..l).map(|i| group_from_xy(&xy[64 * i..64 * i + 64], inf[i] != 0)).collect()
}

// ---- B3: the sumcheck prover loops --------------------------------------------------------------------------------------
// The `comb_func` closures cannot cross FFI; only three are ever passed (A*B*C at product_tree.rs:178-181, 275-278;
// tau*(Az*Bz - Cz) at r1csproof.rs:288-292; z*ABC at r1csproof.rs:389-390), so each prover has its fixed kernel.

fn triple(ev: &[u8]) -> (Scalar, Scalar, Scalar) { (sc(&ev[..32]), sc(&ev[32..64]), sc(&ev[64..96])) }

/// SumcheckInstanceProof::prove_cubic_batched (sumcheck.rs:165-330), comb_func = A*B*C.  The device state returns per round what the
/// transcript absorbs — the coeffs-combined (e0, e2, e3) of :269-271 — and binds every table (:289-299).  The reference's
/// DensePolynomials are left with their single final entry, as its own loop leaves them.
pub fn prove_cubic_batched(
    claim: &Scalar,
    num_rounds: usize,
    poly_vec_par: (&mut Vec<&mut DensePolynomial>, &mut Vec<&mut DensePolynomial>, &mut DensePolynomial),
    poly_vec_seq: (&mut Vec<&mut DensePolynomial>, &mut Vec<&mut DensePolynomial>, &mut Vec<&mut DensePolynomial>),
    coeffs: &[Scalar],
    transcript: &mut Transcript,
) -> (SumcheckInstanceProof, Vec<Scalar>, (Vec<Scalar>, Vec<Scalar>, Scalar), (Vec<Scalar>, Vec<Scalar>, Vec<Scalar>)) {
    let (poly_A_vec_par, poly_B_vec_par, poly_C_par) = poly_vec_par;
    let (poly_A_vec_seq, poly_B_vec_seq, poly_C_vec_seq) = poly_vec_seq;
    let (n_par, n_seq) = (poly_A_vec_par.len(), poly_A_vec_seq.len());
    assert_eq!(coeffs.len(), n_par + n_seq);

    // the tables go up once; the state never writes them
    let ta_par: Vec<Table> = poly_A_vec_par.iter().map(|p| Table::of(p)).collect();
    let tb_par: Vec<Table> = poly_B_vec_par.iter().map(|p| Table::of(p)).collect();
    let tc_par = if n_par > 0 { Some(Table::of(poly_C_par)) } else { None };
    let ta_seq: Vec<Table> = poly_A_vec_seq.iter().map(|p| Table::of(p)).collect();
    let tb_seq: Vec<Table> = poly_B_vec_seq.iter().map(|p| Table::of(p)).collect();
    let tc_seq: Vec<Table> = poly_C_vec_seq.iter().map(|p| Table::of(p)).collect();
    let ptrs = |v: &Vec<Table>| -> Vec<*const sbn_table> { v.iter().map(|t| t.0 as *const sbn_table).collect() };
    let (pa, pb, sa, sb_, sc_) = (ptrs(&ta_par), ptrs(&tb_par), ptrs(&ta_seq), ptrs(&tb_seq), ptrs(&tc_seq));

    let mut ev = [0u8; 96];
    let mut st = null_mut();
    check(unsafe {
        sbn_sumcheck_begin(ctx(), pa.as_ptr(), pb.as_ptr(), tc_par.as_ref().map_or(null(), |t| t.0 as *const sbn_table), n_par,
                           sa.as_ptr(), sb_.as_ptr(), sc_.as_ptr(), n_seq, scalars_canonical(coeffs).as_ptr(), ev.as_mut_ptr(), &mut st)
    });
    let st = SumcheckState(st);

    let mut e = *claim;
    let mut r: Vec<Scalar> = Vec::new();
    let mut cubic_polys: Vec<CompressedUniPoly> = Vec::new();
    for _j in 0..num_rounds {
        let (c0, c2, c3) = triple(&ev);                                        // evals_combined_0 / _2 / _3 (:269-271)
        let poly = UniPoly::from_evals(&[c0, e - c0, c2, c3]);                  // :273-279
        poly.append_to_transcript(b"poly", transcript);                         // :282
        let r_j = transcript.challenge_scalar(b"challenge_nextround");          // :285
        r.push(r_j);
        check(unsafe { sbn_sumcheck_round(ctx(), st.0, r_j.to_bytes().as_ptr(), ev.as_mut_ptr()) });   // binds every table (:289-299), returns the next round's sums
        e = poly.evaluate(&r_j);
        cubic_polys.push(poly.compress());
    }
    // final claims (:302-318), in the order A_par.., B_par.., C_par, A_seq.., B_seq.., C_seq..
    let ntab = 2 * n_par + usize::from(n_par > 0) + 3 * n_seq;
    let mut fin = vec![0u8; 32 * ntab];
    check(unsafe { sbn_sumcheck_finish(ctx(), st.0, fin.as_mut_ptr()) });
    let f = |i: usize| sc(&fin[32 * i..32 * i + 32]);
    let a_par: Vec<Scalar> = (0..n_par).map(f).collect();
    let b_par: Vec<Scalar> = (0..n_par).map(|i| f(n_par + i)).collect();
    let c_par = if n_par > 0 { f(2 * n_par) } else { poly_C_par[0] };
    let o = 2 * n_par + usize::from(n_par > 0);
    let a_seq: Vec<Scalar> = (0..n_seq).map(|i| f(o + i)).collect();
    let b_seq: Vec<Scalar> = (0..n_seq).map(|i| f(o + n_seq + i)).collect();
    let c_seq: Vec<Scalar> = (0..n_seq).map(|i| f(o + 2 * n_seq + i)).collect();
    // leave the host polynomials as the reference's loop leaves them: one entry, the final claim
    for i in 0..n_par { poly_A_vec_par[i].set_final(a_par[i]); poly_B_vec_par[i].set_final(b_par[i]); }
    if n_par > 0 { poly_C_par.set_final(c_par); }
    for i in 0..n_seq { poly_A_vec_seq[i].set_final(a_seq[i]); poly_B_vec_seq[i].set_final(b_seq[i]); poly_C_vec_seq[i].set_final(c_seq[i]); }
    (SumcheckInstanceProof::new(cubic_polys), r, (a_par, b_par, c_par), (a_seq, b_seq, c_seq))
}

/// A Merlin v1.0 transcript held by the library (`sbn_transcript`), with merlin::Transcript's method names.  The device can only
/// continue a transcript whose state it can read, and the merlin crate does not expose its state: a prover that uses
/// `prove_cubic_batched_dev` holds one of these in place of `merlin::Transcript` from `Transcript::new` on.
pub struct DevTranscript(pub *mut sbn_transcript);
unsafe impl Send for DevTranscript {}
impl DevTranscript {
    pub fn new(label: &'static [u8]) -> Self {
        let mut t = null_mut();
        check(unsafe { sbn_transcript_new(label.as_ptr(), label.len(), &mut t) });
        DevTranscript(t)
    }
    pub fn append_message(&mut self, label: &'static [u8], message: &[u8]) {
        check(unsafe { sbn_transcript_append_message(self.0, label.as_ptr(), label.len(), message.as_ptr(), message.len()) });
    }
    pub fn challenge_bytes(&mut self, label: &'static [u8], dest: &mut [u8]) {
        check(unsafe { sbn_transcript_challenge_bytes(self.0, label.as_ptr(), label.len(), dest.as_mut_ptr(), dest.len()) });
    }
    /// ProofTranscript::append_scalar / challenge_scalar (transcript.rs:41-43, 56-67)
    pub fn append_scalar(&mut self, label: &'static [u8], scalar: &Scalar) { self.append_message(label, &scalar.to_bytes()); }
    pub fn challenge_scalar(&mut self, label: &'static [u8]) -> Scalar {
        let mut out = [0u8; 32];
        check(unsafe { sbn_transcript_challenge_scalar(self.0, label.as_ptr(), label.len(), out.as_mut_ptr()) });
        sc(&out)
    }
    pub fn state(&self) -> [u8; 203] {
        let mut out = [0u8; 203];
        check(unsafe { sbn_transcript_state(self.0, out.as_mut_ptr()) });
        out
    }
}
impl Clone for DevTranscript {
    fn clone(&self) -> Self {
        let mut t = null_mut();
        check(unsafe { sbn_transcript_clone(self.0, &mut t) });
        DevTranscript(t)
    }
}
impl Drop for DevTranscript {
    fn drop(&mut self) { unsafe { sbn_transcript_free(self.0) } }
}

/// prove_cubic_batched with the transcript on the device: ONE foreign call for all rounds (sbn_sumcheck_prove) instead of one per round.
/// Same proof, challenges and claims as `prove_cubic_batched` gives with a merlin::Transcript in the same state.
pub fn prove_cubic_batched_dev(
    claim: &Scalar,
    num_rounds: usize,
    poly_vec_par: (&mut Vec<&mut DensePolynomial>, &mut Vec<&mut DensePolynomial>, &mut DensePolynomial),
    poly_vec_seq: (&mut Vec<&mut DensePolynomial>, &mut Vec<&mut DensePolynomial>, &mut Vec<&mut DensePolynomial>),
    coeffs: &[Scalar],
    transcript: &mut DevTranscript,
) -> (SumcheckInstanceProof, Vec<Scalar>, (Vec<Scalar>, Vec<Scalar>, Scalar), (Vec<Scalar>, Vec<Scalar>, Vec<Scalar>)) {
    let (poly_A_vec_par, poly_B_vec_par, poly_C_par) = poly_vec_par;
    let (poly_A_vec_seq, poly_B_vec_seq, poly_C_vec_seq) = poly_vec_seq;
    let (n_par, n_seq) = (poly_A_vec_par.len(), poly_A_vec_seq.len());
    assert_eq!(coeffs.len(), n_par + n_seq);
    let ta_par: Vec<Table> = poly_A_vec_par.iter().map(|p| Table::of(p)).collect();
    let tb_par: Vec<Table> = poly_B_vec_par.iter().map(|p| Table::of(p)).collect();
    let tc_par = if n_par > 0 { Some(Table::of(poly_C_par)) } else { None };
    let ta_seq: Vec<Table> = poly_A_vec_seq.iter().map(|p| Table::of(p)).collect();
    let tb_seq: Vec<Table> = poly_B_vec_seq.iter().map(|p| Table::of(p)).collect();
    let tc_seq: Vec<Table> = poly_C_vec_seq.iter().map(|p| Table::of(p)).collect();
    let ptrs = |v: &Vec<Table>| -> Vec<*const sbn_table> { v.iter().map(|t| t.0 as *const sbn_table).collect() };
    let (pa, pb, sa, sb_, sc_) = (ptrs(&ta_par), ptrs(&tb_par), ptrs(&ta_seq), ptrs(&tb_seq), ptrs(&tc_seq));

    let mut ev = [0u8; 96];
    let mut st = null_mut();
    check(unsafe {
        sbn_sumcheck_begin(ctx(), pa.as_ptr(), pb.as_ptr(), tc_par.as_ref().map_or(null(), |t| t.0 as *const sbn_table), n_par,
                           sa.as_ptr(), sb_.as_ptr(), sc_.as_ptr(), n_seq, scalars_canonical(coeffs).as_ptr(), ev.as_mut_ptr(), &mut st)
    });
    let st = SumcheckState(st);
    assert_eq!(unsafe { sbn_sumcheck_len(st.0) }, 1usize << num_rounds);

    let ntab = 2 * n_par + usize::from(n_par > 0) + 3 * n_seq;
    let (mut polys, mut rs, mut fin) = (vec![0u8; 128 * num_rounds], vec![0u8; 32 * num_rounds], vec![0u8; 32 * ntab]);
    check(unsafe { sbn_sumcheck_prove(ctx(), st.0, transcript.0, claim.to_bytes().as_ptr(), polys.as_mut_ptr(), rs.as_mut_ptr(), fin.as_mut_ptr()) });
    let r: Vec<Scalar> = (0..num_rounds).map(|j| sc(&rs[32 * j..32 * j + 32])).collect();
    let cubic_polys: Vec<CompressedUniPoly> = (0..num_rounds)
        .map(|j| {
            // UniPoly keeps its coefficients private: rebuild it from its values at 0, 1, 2, 3 (from_evals inverts exactly)
            let c: Vec<Scalar> = (0..4).map(|k| sc(&polys[128 * j + 32 * k..128 * j + 32 * k + 32])).collect();
            let at = |x: u64| { let x = Scalar::from_u64(x); c[0] + x * (c[1] + x * (c[2] + x * c[3])) };
            UniPoly::from_evals(&[at(0), at(1), at(2), at(3)]).compress()
        })
        .collect();
    let f = |i: usize| sc(&fin[32 * i..32 * i + 32]);
    let a_par: Vec<Scalar> = (0..n_par).map(f).collect();
    let b_par: Vec<Scalar> = (0..n_par).map(|i| f(n_par + i)).collect();
    let c_par = if n_par > 0 { f(2 * n_par) } else { poly_C_par[0] };
    let o = 2 * n_par + usize::from(n_par > 0);
    let a_seq: Vec<Scalar> = (0..n_seq).map(|i| f(o + i)).collect();
    let b_seq: Vec<Scalar> = (0..n_seq).map(|i| f(o + n_seq + i)).collect();
    let c_seq: Vec<Scalar> = (0..n_seq).map(|i| f(o + 2 * n_seq + i)).collect();
    for i in 0..n_par { poly_A_vec_par[i].set_final(a_par[i]); poly_B_vec_par[i].set_final(b_par[i]); }
    if n_par > 0 { poly_C_par.set_final(c_par); }
    for i in 0..n_seq { poly_A_vec_seq[i].set_final(a_seq[i]); poly_B_vec_seq[i].set_final(b_seq[i]); poly_C_vec_seq[i].set_final(c_seq[i]); }
    (SumcheckInstanceProof::new(cubic_polys), r, (a_par, b_par, c_par), (a_seq, b_seq, c_seq))
}

/// SumcheckInstanceProof::prove_cubic (sumcheck.rs:89-161), comb_func = A*B*C: the batched prover with ONE "seq" instance and
/// coefficient one (its combined sums ARE the instance's sums)
pub fn prove_cubic(
    claim: &Scalar,
    num_rounds: usize,
    poly_A: &mut DensePolynomial,
    poly_B: &mut DensePolynomial,
    poly_C: &mut DensePolynomial,
    transcript: &mut Transcript,
) -> (SumcheckInstanceProof, Vec<Scalar>, Vec<Scalar>) {
    let mut none_a: Vec<&mut DensePolynomial> = Vec::new();
    let mut none_b: Vec<&mut DensePolynomial> = Vec::new();
    let mut dummy_c = DensePolynomial::new(vec![Scalar::zero()]);
    let (proof, r, _claims_prod, claims_dotp) = {
        let mut va = vec![&mut *poly_A];
        let mut vb = vec![&mut *poly_B];
        let mut vc = vec![&mut *poly_C];
        prove_cubic_batched(claim, num_rounds, (&mut none_a, &mut none_b, &mut dummy_c), (&mut va, &mut vb, &mut vc), &[Scalar::one()], transcript)
    };
    (proof, r, vec![claims_dotp.0[0], claims_dotp.1[0], claims_dotp.2[0]])
}

/// The table side of ZKSumcheckInstanceProof::prove_cubic_with_additive_term (sumcheck.rs:465-649): f = tau * (Az * Bz - Cz).
/// `evals()` is the loop of :502-530 for the current round; `bind(r_j)` is :551-554 and prepares the next round's sums in the same
/// pass.  Everything between (commitments, Σ-protocol, transcript: :531-548, :556-640) stays the reference's host code.
pub struct R1csRounds { t: [Table; 4], ev: [u8; 96] }
impl R1csRounds {
    pub fn new(tau: &DensePolynomial, az: &DensePolynomial, bz: &DensePolynomial, cz: &DensePolynomial) -> Self {
        let t = [Table::of(tau), Table::of(az), Table::of(bz), Table::of(cz)];
        let mut ev = [0u8; 96];
        check(unsafe { sbn_sc_eval_r1cs(ctx(), t[0].0, t[1].0, t[2].0, t[3].0, ev.as_mut_ptr()) });
        R1csRounds { t, ev }
    }
    /// (eval_point_0, eval_point_2, eval_point_3) of the current round
    pub fn evals(&self) -> (Scalar, Scalar, Scalar) { triple(&self.ev) }
    /// bound_poly_var_top(r_j) on all four tables; the next round's sums are ready afterwards
    pub fn bind(&mut self, r_j: &Scalar) {
        let rb = r_j.to_bytes();
        if self.t[0].len() >= 4 {
            check(unsafe { sbn_sc_bind_eval_r1cs(ctx(), self.t[0].0, self.t[1].0, self.t[2].0, self.t[3].0, rb.as_ptr(), self.ev.as_mut_ptr()) });
        } else {
            let ts: Vec<*mut sbn_table> = self.t.iter().map(|t| t.0).collect();
            check(unsafe { sbn_bind_top_many(ctx(), ts.as_ptr(), ts.len(), rb.as_ptr()) });
        }
    }
    /// [poly_tau[0], poly_Az[0], poly_Bz[0], poly_Cz[0]] after the last round (:645)
    pub fn finals(&self) -> Vec<Scalar> {
        let ts: Vec<*const sbn_table> = self.t.iter().map(|t| t.0 as *const sbn_table).collect();
        let mut out = [0u8; 128];
        check(unsafe { sbn_table_read0_many(ctx(), ts.as_ptr(), ts.len(), out.as_mut_ptr()) });
        (0..4).map(|i| sc(&out[32 * i..32 * i + 32])).collect()
    }
}
/// The table side of ZKSumcheckInstanceProof::prove_quad (sumcheck.rs:657-811): f = z * ABC, points 0 and 2 (:691-699), bind (:715-716)
pub struct QuadRounds { t: [Table; 2], ev: [u8; 64] }
impl QuadRounds {
    pub fn new(z: &DensePolynomial, abc: &DensePolynomial) -> Self {
        let t = [Table::of(z), Table::of(abc)];
        let mut ev = [0u8; 64];
        check(unsafe { sbn_sc_eval_quad(ctx(), t[0].0, t[1].0, ev.as_mut_ptr()) });
        QuadRounds { t, ev }
    }
    pub fn evals(&self) -> (Scalar, Scalar) { (sc(&self.ev[..32]), sc(&self.ev[32..64])) }
    pub fn bind(&mut self, r_j: &Scalar) {
        let rb = r_j.to_bytes();
        if self.t[0].len() >= 4 {
            check(unsafe { sbn_sc_bind_eval_quad(ctx(), self.t[0].0, self.t[1].0, rb.as_ptr(), self.ev.as_mut_ptr()) });
        } else {
            let ts: Vec<*mut sbn_table> = self.t.iter().map(|t| t.0).collect();
            check(unsafe { sbn_bind_top_many(ctx(), ts.as_ptr(), ts.len(), rb.as_ptr()) });
        }
    }
    pub fn finals(&self) -> Vec<Scalar> {
        let ts: Vec<*const sbn_table> = self.t.iter().map(|t| t.0 as *const sbn_table).collect();
        let mut out = [0u8; 64];
        check(unsafe { sbn_table_read0_many(ctx(), ts.as_ptr(), ts.len(), out.as_mut_ptr()) });
        vec![sc(&out[..32]), sc(&out[32..64])]
    }
}

// ---- the two ZK sumchecks of R1CSProof::prove in ONE foreign call each (sbn_zk_sumcheck_prove_r1cs / _quad) -----------------------
// The library runs the rounds, UniPoly::from_evals, the four commitments of a round, DotProductProof::prove and the transcript; this side
// draws the RandomTape in the reference's order (blinds_poly, blinds_evals, then per round d_vec, r_delta, r_beta: sumcheck.rs:483-484,
// nizk/mod.rs:326-328) and rebuilds ZKSumcheckInstanceProof from the bytes.  DotProductProof keeps its fields private: it is read back
// through its own CanonicalDeserialize (delta, beta as compressed points, z as a length-prefixed vector, z_delta, z_beta).
fn zk_draws(random_tape: &mut RandomTape, num_rounds: usize, n: usize) -> Vec<Scalar> {
    let mut rnd = random_tape.random_vector(b"blinds_poly", num_rounds);
    rnd.extend(random_tape.random_vector(b"blinds_evals", num_rounds));
    for _ in 0..num_rounds {
        rnd.extend(random_tape.random_vector(b"d_vec", n));
        rnd.push(random_tape.random_scalar(b"r_delta"));
        rnd.push(random_tape.random_scalar(b"r_beta"));
    }
    rnd
}
fn zk_proof_from_bytes(proof: &[u8], num_rounds: usize, n: usize) -> ZKSumcheckInstanceProof {
    let stride = (6 + n) * 32;
    let point = |b: &[u8]| CompressedGroup::from_bytes(b).decompress().expect("sbn254 returned a point that does not decompress");
    let (mut comm_polys, mut comm_evals, mut proofs) = (Vec::new(), Vec::new(), Vec::new());
    for j in 0..num_rounds {
        let p = &proof[stride * j..stride * (j + 1)];
        comm_polys.push(point(&p[..32]));
        comm_evals.push(point(&p[32..64]));
        let mut ser: Vec<u8> = p[64..128].to_vec();                                   // delta, beta
        ser.extend_from_slice(&(n as u64).to_le_bytes());                             // z: Vec<Scalar>
        ser.extend_from_slice(&p[128..stride]);                                       // z[n], z_delta, z_beta
        proofs.push(DotProductProof::deserialize_compressed(&ser[..]).expect("DotProductProof from the library's bytes"));
    }
    ZKSumcheckInstanceProof::new(comm_polys, comm_evals, proofs)
}
/// ZKSumcheckInstanceProof::prove_cubic_with_additive_term (sumcheck.rs:465-649), comb_func = tau * (Az * Bz - Cz), with a `DevTranscript`
#[allow(non_snake_case)]
pub fn zk_prove_r1cs(
    claim: &Scalar,
    blind_claim: &Scalar,
    num_rounds: usize,
    poly_tau: &mut DensePolynomial,
    poly_Az: &mut DensePolynomial,
    poly_Bz: &mut DensePolynomial,
    poly_Cz: &mut DensePolynomial,
    gens_1: &MultiCommitGens,
    gens_n: &MultiCommitGens,
    transcript: &mut DevTranscript,
    random_tape: &mut RandomTape,
) -> (ZKSumcheckInstanceProof, Vec<Scalar>, Vec<Scalar>, Scalar) {
    assert_eq!(poly_tau.len(), 1usize << num_rounds);
    let rnd = scalars_canonical(&zk_draws(random_tape, num_rounds, 4));
    let t = [Table::of(poly_tau), Table::of(poly_Az), Table::of(poly_Bz), Table::of(poly_Cz)];
    let (mut proof, mut rs, mut fin, mut bl) = (vec![0u8; 320 * num_rounds], vec![0u8; 32 * num_rounds], [0u8; 128], [0u8; 32]);
    check(unsafe {
        sbn_zk_sumcheck_prove_r1cs(ctx(), t[0].0, t[1].0, t[2].0, t[3].0, gens_1.dev.bases(gens_1), gens_n.dev.bases(gens_n), claim.to_bytes().as_ptr(),
                                   blind_claim.to_bytes().as_ptr(), rnd.as_ptr(), transcript.0, proof.as_mut_ptr(), rs.as_mut_ptr(), fin.as_mut_ptr(), bl.as_mut_ptr())
    });
    let r: Vec<Scalar> = (0..num_rounds).map(|j| sc(&rs[32 * j..32 * j + 32])).collect();
    let finals: Vec<Scalar> = (0..4).map(|i| sc(&fin[32 * i..32 * i + 32])).collect();
    poly_tau.set_final(finals[0]); poly_Az.set_final(finals[1]); poly_Bz.set_final(finals[2]); poly_Cz.set_final(finals[3]);
    (zk_proof_from_bytes(&proof, num_rounds, 4), r, finals, sc(&bl))
}
/// ZKSumcheckInstanceProof::prove_quad (sumcheck.rs:657-811), comb_func = z * ABC, with a `DevTranscript`
#[allow(non_snake_case)]
pub fn zk_prove_quad(
    claim: &Scalar,
    blind_claim: &Scalar,
    num_rounds: usize,
    poly_z: &mut DensePolynomial,
    poly_ABC: &mut DensePolynomial,
    gens_1: &MultiCommitGens,
    gens_n: &MultiCommitGens,
    transcript: &mut DevTranscript,
    random_tape: &mut RandomTape,
) -> (ZKSumcheckInstanceProof, Vec<Scalar>, Vec<Scalar>, Scalar) {
    assert_eq!(poly_z.len(), 1usize << num_rounds);
    let rnd = scalars_canonical(&zk_draws(random_tape, num_rounds, 3));
    let t = [Table::of(poly_z), Table::of(poly_ABC)];
    let (mut proof, mut rs, mut fin, mut bl) = (vec![0u8; 288 * num_rounds], vec![0u8; 32 * num_rounds], [0u8; 64], [0u8; 32]);
    check(unsafe {
        sbn_zk_sumcheck_prove_quad(ctx(), t[0].0, t[1].0, gens_1.dev.bases(gens_1), gens_n.dev.bases(gens_n), claim.to_bytes().as_ptr(),
                                   blind_claim.to_bytes().as_ptr(), rnd.as_ptr(), transcript.0, proof.as_mut_ptr(), rs.as_mut_ptr(), fin.as_mut_ptr(), bl.as_mut_ptr())
    });
    let r: Vec<Scalar> = (0..num_rounds).map(|j| sc(&rs[32 * j..32 * j + 32])).collect();
    let finals = vec![sc(&fin[..32]), sc(&fin[32..64])];
    poly_z.set_final(finals[0]); poly_ABC.set_final(finals[1]);
    (zk_proof_from_bytes(&proof, num_rounds, 3), r, finals, sc(&bl))
}

// ---- BulletReductionProof::prove (nizk/bullet.rs:41-126) ---------------------------------------------------------------------
// The generators arrive as a slice (`&gens.gens_n.G`); their device handle is cached by (address, length, first and last point), i.e.
// per MultiCommitGens in practice — built on the first opening over a generator set, with h = H.
fn bases_for_slice(G_vec: &[GroupElement], H: &GroupElement) -> Arc<Bases> {
    static CACHE: OnceLock<Mutex<HashMap<(usize, usize, [u8; 64], [u8; 64]), Arc<Bases>>>> = OnceLock::new();
    let first = point_xy_mont(&affine_of(&G_vec[0]));
    let last = point_xy_mont(&affine_of(&G_vec[G_vec.len() - 1]));
    let key = (G_vec.as_ptr() as usize, G_vec.len(), first, last);
    let mut m = CACHE.get_or_init(|| Mutex::new(HashMap::new())).lock().unwrap();
    if let Some(b) = m.get(&key) { return b.clone(); }
    let proj: Vec<G1Projective> = G_vec.iter().map(|g| *g.inner()).collect();
    let aff = G1Projective::normalize_batch(&proj);
    let g: Vec<u8> = aff.iter().flat_map(point_xy_mont).collect();
    let h = point_xy_mont(&affine_of(H));
    let mut b = null_mut();
    check(unsafe { sbn_bases_upload(ctx(), g.as_ptr(), G_vec.len(), h.as_ptr(), SBN_POINTS_MONT, &mut b) });
    let b = Arc::new(Bases(b));
    m.insert(key, b.clone());
    b
}

/// BulletReductionProof::prove with Q = q_scale * Q_base: DotProductProofLog::prove hands the reduction Q = gens_1.scale(r).G[0]
/// (nizk/mod.rs:478-494), a new point per proof over the FIXED base gens_1.G[0]; given as (base, scalar) the device builds its
/// derived generator set once per circuit.  Returns (L_vec, R_vec, Gamma, a_hat, b_hat, g_hat, rhat_Gamma) — the fields and values of
/// bullet.rs:118-125.  The generators are never folded on the device (bullet.rs:87-91 costs n scalar multiplications per round):
/// round j's L, R are MSMs over the ORIGINAL generators; same group elements.
pub fn bullet_prove(
    transcript: &mut Transcript,
    Q_base: &GroupElement,
    q_scale: &Scalar,
    G_vec: &[GroupElement],
    H: &GroupElement,
    a_vec: &[Scalar],
    b_vec: &[Scalar],
    blind: &Scalar,
    blinds_vec: &[(Scalar, Scalar)],
) -> (Vec<GroupElement>, Vec<GroupElement>, GroupElement, Scalar, Scalar, GroupElement, Scalar) {
    let n = G_vec.len();
    assert_eq!(a_vec.len(), n);                                                 // bullet.rs:42
    assert_eq!(b_vec.len(), n);                                                 // :43
    assert!(n.is_power_of_two());                                               // :44
    let lg_n = n.trailing_zeros() as usize;
    assert_eq!(blinds_vec.len(), lg_n);                                         // :47

    let bases = bases_for_slice(G_vec, H);
    let (ta, tb) = (Table::upload(a_vec), Table::upload(b_vec));                // the reference clones a and b too (:50-52)
    let qb = point_xy_canonical(&affine_of(Q_base));
    let mut gamma = [0u8; 64];
    let mut ginf: c_int = 0;
    let mut st = null_mut();
    check(unsafe {
        sbn_bullet_begin_scaled(ctx(), bases.0, qb.as_ptr(), q_scale.to_bytes().as_ptr(), ta.0, tb.0, blind.to_bytes().as_ptr(), gamma.as_mut_ptr(), &mut ginf, &mut st)
    });                                                                         // Gamma (:58-60)
    let st = BulletState(st);
    let Gamma = group_from_xy(&gamma, ginf != 0);

    let mut blind_Gamma = *blind;
    let mut L_vec: Vec<GroupElement> = Vec::with_capacity(lg_n);
    let mut R_vec: Vec<GroupElement> = Vec::with_capacity(lg_n);
    let (mut lxy, mut rxy, mut cl, mut cr) = ([0u8; 64], [0u8; 64], [0u8; 32], [0u8; 32]);
    let (mut li, mut ri): (c_int, c_int) = (0, 0);
    if lg_n > 0 {
        let (bl, br) = blinds_vec[0];
        check(unsafe {
            sbn_bullet_cross(ctx(), st.0, bl.to_bytes().as_ptr(), br.to_bytes().as_ptr(), lxy.as_mut_ptr(), &mut li, rxy.as_mut_ptr(), &mut ri, cl.as_mut_ptr(), cr.as_mut_ptr())
        });                                                                     // c_L, c_R, L, R of round 0 (:72-78)
    }
    for i in 0..lg_n {
        let L = group_from_xy(&lxy, li != 0);
        let R = group_from_xy(&rxy, ri != 0);
        L.append_to_transcript(b"L", transcript);                               // :80
        R.append_to_transcript(b"R", transcript);                               // :81
        let u = transcript.challenge_scalar(b"u");                              // :83
        let u_inv = u.invert().unwrap();                                        // :84
        let (blind_L, blind_R) = blinds_vec[i];
        if i + 1 < lg_n {
            // the folds with u (:86-106) and the NEXT round's cross terms in one call
            let (bl, br) = blinds_vec[i + 1];
            check(unsafe {
                sbn_bullet_fold_cross(ctx(), st.0, u.to_bytes().as_ptr(), u_inv.to_bytes().as_ptr(), bl.to_bytes().as_ptr(), br.to_bytes().as_ptr(),
                                      lxy.as_mut_ptr(), &mut li, rxy.as_mut_ptr(), &mut ri, cl.as_mut_ptr(), cr.as_mut_ptr())
            });
        } else {
            check(unsafe { sbn_bullet_fold(ctx(), st.0, u.to_bytes().as_ptr(), u_inv.to_bytes().as_ptr()) });
        }
        blind_Gamma = u * u * blind_L + blind_Gamma + u_inv * u_inv * blind_R;  // :108
        L_vec.push(L);
        R_vec.push(R);
    }
    let (mut ah, mut bh, mut gh) = ([0u8; 32], [0u8; 32], [0u8; 64]);
    let mut gi: c_int = 0;
    check(unsafe { sbn_bullet_finish(ctx(), st.0, ah.as_mut_ptr(), bh.as_mut_ptr(), gh.as_mut_ptr(), &mut gi) });   // :114-120
    (L_vec, R_vec, Gamma, sc(&ah), sc(&bh), group_from_xy(&gh, gi != 0), blind_Gamma)
}
/// canonical x || y (no *_MONT flag on this argument of the bullet entry points)
fn point_xy_canonical(p: &G1Affine) -> [u8; 64] {
    let mut o = [0u8; 64];
    if !p.is_zero() {
        o[..32].copy_from_slice(&limbs_le(&p.x.into_bigint().0));
        o[32..].copy_from_slice(&limbs_le(&p.y.into_bigint().0));
    }
    o
}

#[cfg(test)]
mod tests {
    use super::*;
    use crate::commitments::Commitments;

    /// the device MSM against arkworks on the reference's own generator derivation (two thirds of the points equal G)
    #[test]
    fn msm_matches_arkworks() {
        let n = 4096;
        let gens = MultiCommitGens::new(n, b"gens_r1cs_eval");
        let mut rng = rand::rngs::OsRng;
        let s: Vec<Scalar> = (0..n).map(|_| Scalar::random(&mut rng)).collect();
        let want = {
            let fr: Vec<ark_bn254::Fr> = s.iter().map(|x| x.0).collect();
            GroupElement(<G1Projective as ark_ec::VariableBaseMSM>::msm(&gens.G_affine, &fr).unwrap())
        };
        assert_eq!(msm_affine(&s, &gens.G_affine).unwrap(), want);
        let blind = Scalar::random(&mut rng);
        assert_eq!(commit_row(&s, &blind, &gens).unwrap(), want + blind * gens.h);
        assert_eq!(s.commit(&blind, &gens), want + blind * gens.h);
    }
}

// ---- KZG mode (--features hip,kzg; kzg.rs): the SRS stays resident, commitments and openings run over it ----------------------
/// KZGSrs.powers_g1 on the device (kzg.rs:25-31)
pub struct KzgSrs(pub *mut sbn_bases);
unsafe impl Send for KzgSrs {}
unsafe impl Sync for KzgSrs {}
impl Drop for KzgSrs { fn drop(&mut self) { if !self.0.is_null() { unsafe { sbn_bases_free(ctx(), self.0) } } } }
impl std::fmt::Debug for KzgSrs { fn fmt(&self, f: &mut std::fmt::Formatter<'_>) -> std::fmt::Result { write!(f, "KzgSrs({:p})", self.0) } }
impl KzgSrs {
    /// upload of the SRS points (no duplicate detection: an SRS has none)
    pub fn upload(powers_g1: &[G1Affine]) -> KzgSrs {
        let pts: Vec<u8> = powers_g1.iter().flat_map(point_xy_mont).collect();
        let mut b = null_mut();
        check(unsafe { sbn_kzg_srs_upload(ctx(), pts.as_ptr(), powers_g1.len(), SBN_POINTS_MONT, &mut b) });
        KzgSrs(b)
    }
    /// [tau^i]G1 for i < n, built on the device (kzg.rs:37-56 with tau supplied)
    pub fn from_tau(tau: &Scalar, n: usize) -> KzgSrs {
        let mut b = null_mut();
        check(unsafe { sbn_kzg_srs_from_tau(ctx(), tau.to_bytes().as_ptr(), n, &mut b) });
        KzgSrs(b)
    }
    pub fn len(&self) -> usize { unsafe { sbn_bases_len(self.0) } }
    pub fn is_empty(&self) -> bool { self.len() == 0 }
    /// KZGSrs::load_from_file (kzg.rs:79-88) on the file's bytes: the powers are decompressed on the device, the two G2 points on the host.
    /// -> (the SRS, the prepared g2, the prepared tau_g2).  A refusal is the library's text: it names the reason and, for a power, its index.
    /// `check_consistency`: also run the consistency check (SBN_SRS_CHECK), which arkworks' deserialisation does not.
    pub fn load(bytes: &[u8], check_consistency: bool) -> Result<(KzgSrs, G2Lines, G2Lines), String> {
        let (mut b, mut g2, mut tau_g2) = (null_mut(), null_mut(), null_mut());
        let mut bad: usize = usize::MAX;
        let flags = if check_consistency { SBN_SRS_CHECK } else { 0 };
        let rc = unsafe { sbn_kzg_srs_load(ctx(), bytes.as_ptr(), bytes.len(), flags, &mut b, &mut g2, &mut tau_g2, null_mut(), &mut bad) };
        if rc != SBN_OK {
            return Err(unsafe { std::ffi::CStr::from_ptr(sbn_last_error(ctx())) }.to_string_lossy().into_owned());
        }
        Ok((KzgSrs(b), G2Lines(g2), G2Lines(tau_g2)))
    }
    /// A powers-of-tau ceremony file (.ptau) as the SRS: the first `n` powers (0: all of them) of its tauG1 section and tauG2[0], tauG2[1].  `bytes`
    /// may be a memory map of the whole file: only the section table, 64 n bytes of section 2 and 256 bytes of section 3 are read.  Every point is
    /// validated on the device; a refusal is the library's text, as in `load`.
    pub fn load_ptau(bytes: &[u8], n: usize, check_consistency: bool) -> Result<(KzgSrs, G2Lines, G2Lines), String> {
        let (mut b, mut g2, mut tau_g2) = (null_mut(), null_mut(), null_mut());
        let mut bad: usize = usize::MAX;
        let flags = if check_consistency { SBN_SRS_CHECK } else { 0 };
        let rc = unsafe { sbn_kzg_srs_load_ptau(ctx(), bytes.as_ptr(), bytes.len(), n, flags, &mut b, &mut g2, &mut tau_g2, null_mut(), &mut bad) };
        if rc != SBN_OK {
            return Err(unsafe { std::ffi::CStr::from_ptr(sbn_last_error(ctx())) }.to_string_lossy().into_owned());
        }
        Ok((KzgSrs(b), G2Lines(g2), G2Lines(tau_g2)))
    }
    /// the header of a .ptau file (host only): None for a file `load_ptau` would refuse before it reads a point
    pub fn ptau_info(bytes: &[u8]) -> Option<sbn_ptau_info> {
        let mut info = sbn_ptau_info::default();
        if unsafe { sbn_ptau_scan(bytes.as_ptr(), bytes.len(), &mut info) } == SBN_OK { Some(info) } else { None }
    }
    /// KZGSrs::save_to_file (kzg.rs:66-77) as bytes; `g2_xy`, `tau_g2_xy`: G2Affine's in-memory x.c0, x.c1, y.c0, y.c1 (ark-ff Montgomery limbs)
    pub fn save(&self, g2_xy: &[u8; 128], tau_g2_xy: &[u8; 128]) -> Vec<u8> {
        let mut len: usize = 0;
        check(unsafe { sbn_kzg_srs_save(ctx(), self.0, null(), null(), 0, null_mut(), 0, &mut len) });
        let mut out = vec![0u8; len];
        check(unsafe { sbn_kzg_srs_save(ctx(), self.0, g2_xy.as_ptr(), tau_g2_xy.as_ptr(), SBN_POINTS_MONT, out.as_mut_ptr(), out.len(), &mut len) });
        out.truncate(len);
        out
    }
    /// are the points the powers of one tau that matches tau_g2?  `rho`: drawn by the caller AFTER the file is fixed (non-zero)
    pub fn check(&self, g2: &G2Lines, tau_g2: &G2Lines, rho: &Scalar) -> bool {
        let mut consistent: c_int = 0;
        check(unsafe { sbn_kzg_srs_check(ctx(), self.0, g2.0, tau_g2.0, rho.to_bytes().as_ptr(), &mut consistent) });
        consistent != 0
    }
}
/// KZGPolyCommitment::commit (kzg.rs:386-395) and KZGCommitment::commit (kzg.rs:132-147): the first min(n, srs len) coefficients
pub fn kzg_commit(coeffs: &Table, n: usize, srs: &KzgSrs) -> GroupElement {
    let mut xy = [0u8; 64];
    let mut inf: c_int = 0;
    check(unsafe { sbn_kzg_commit(ctx(), srs.0, coeffs.0, n, xy.as_mut_ptr(), &mut inf) });
    group_from_xy(&xy, inf != 0)
}
/// KZGProof::prove (kzg.rs:174-192) -> (proof, p(z))
pub fn kzg_open(coeffs: &Table, n: usize, point: &Scalar, srs: &KzgSrs) -> (GroupElement, Scalar) {
    let mut ev = [0u8; 32];
    let mut xy = [0u8; 64];
    let mut inf: c_int = 0;
    check(unsafe { sbn_kzg_open(ctx(), srs.0, coeffs.0, n, point.to_bytes().as_ptr(), ev.as_mut_ptr(), xy.as_mut_ptr(), &mut inf) });
    (group_from_xy(&xy, inf != 0), sc(&ev))
}
/// KZGBatchedEvalProof::prove -> KZGBatchProof::batch_prove (kzg.rs:478-500, 268-312) -> (proof, evals); gamma is what the caller drew
/// from the transcript (`Scalar::from_bytes(..).unwrap_or(Scalar::one())`, kzg.rs:275-277)
pub fn kzg_open_batched(polys: &[(&Table, usize)], point: &Scalar, gamma: &Scalar, srs: &KzgSrs) -> (GroupElement, Vec<Scalar>) {
    let ts: Vec<*const sbn_table> = polys.iter().map(|(t, _)| t.0 as *const sbn_table).collect();
    let ns: Vec<usize> = polys.iter().map(|(_, n)| *n).collect();
    let mut ev = vec![0u8; 32 * polys.len()];
    let mut xy = [0u8; 64];
    let mut inf: c_int = 0;
    check(unsafe {
        sbn_kzg_open_batched(ctx(), srs.0, ts.as_ptr(), ns.as_ptr(), polys.len(), point.to_bytes().as_ptr(), gamma.to_bytes().as_ptr(), ev.as_mut_ptr(), xy.as_mut_ptr(), &mut inf)
    });
    (group_from_xy(&xy, inf != 0), ev.chunks(32).map(sc).collect())
}
/// srs.g2 / srs.tau_g2 made ready for pairings (sbn_g2_prepare: what Bn254::pairing's G2Prepared::from does on every call, once per SRS).
/// `xy`: G2Affine's in-memory x.c0, x.c1, y.c0, y.c1 (ark-ff Montgomery limbs, 4 x 32 bytes)
pub struct G2Lines(pub *mut sbn_g2_lines);
unsafe impl Send for G2Lines {}
unsafe impl Sync for G2Lines {}
impl Drop for G2Lines { fn drop(&mut self) { if !self.0.is_null() { unsafe { sbn_g2_lines_free(ctx(), self.0) } } } }
impl G2Lines {
    pub fn from_mont_limbs(x_c0: &[u64; 4], x_c1: &[u64; 4], y_c0: &[u64; 4], y_c1: &[u64; 4]) -> G2Lines {
        let mut xy = [0u8; 128];
        for (i, l) in [x_c0, x_c1, y_c0, y_c1].iter().enumerate() { xy[32 * i..32 * i + 32].copy_from_slice(&limbs_le(l)); }
        let mut h = null_mut();
        check(unsafe { sbn_g2_prepare(ctx(), xy.as_ptr(), SBN_POINTS_MONT, &mut h) });
        G2Lines(h)
    }
}
/// canonical x || y of an affine point (64 zero bytes: the identity): what the verifier entry points take
pub fn point_xy_canonical(p: &G1Affine) -> [u8; 64] {
    let mut o = [0u8; 64];
    if !p.is_zero() {
        o[..32].copy_from_slice(&limbs_le(&ark_ff::PrimeField::into_bigint(p.x).0));
        o[32..].copy_from_slice(&limbs_le(&ark_ff::PrimeField::into_bigint(p.y).0));
    }
    o
}
/// KZGProof::verify (kzg.rs:196-217): e(C - y G + z pi, g2) * e(-pi, tau_g2) == 1 on the device
pub fn kzg_verify(g2: &G2Lines, tau_g2: &G2Lines, commitment: &G1Affine, point: &Scalar, eval: &Scalar, proof: &G1Affine) -> bool {
    let (c, p) = (point_xy_canonical(commitment), point_xy_canonical(proof));
    let mut accepted: c_int = 0;
    check(unsafe { sbn_kzg_verify(ctx(), g2.0, tau_g2.0, c.as_ptr(), point.to_bytes().as_ptr(), eval.to_bytes().as_ptr(), p.as_ptr(), &mut accepted) });
    accepted != 0
}
/// SparseMatPolyEvalProof::verify of the KZG build (sparse_mlpoly_full.rs:1815-1845) in ONE foreign call.  `proof`: the bytes in the library's layout
/// (what `sbn_sparse_eval_prove_kzg` wrote: include/sbn254.h); `comm_ops` / `comm_mem`: the computation commitment's row commitments, resident;
/// `transcript` moves on only when the proof is accepted.  With `sbn_r1cs_proof_verify` this is the whole of the KZG build's `SNARK::verify`.
#[cfg(feature = "kzg")]
pub fn sparse_eval_verify_kzg(
    num_vars_x: usize, num_vars_y: usize, num_ops: usize, num_cells: usize, comm_ops: &Bases, comm_mem: &Bases, rx: &[Scalar], ry: &[Scalar], evals: &[Scalar],
    gens: &SparseMatPolyCommitmentGens, g2: &G2Lines, tau_g2: &G2Lines, proof: &[u8], transcript: &mut DevTranscript,
) -> bool {
    let (rxb, ryb, evb) = (scalars_canonical(rx), scalars_canonical(ry), scalars_canonical(evals));
    let g_ops = pc_bases(&gens.gens_ops.gens.gens_n, &gens.gens_ops.gens.gens_1);
    let g_mem = pc_bases(&gens.gens_mem.gens.gens_n, &gens.gens_mem.gens.gens_1);
    let mut accepted: c_int = 0;
    check(unsafe {
        sbn_sparse_eval_verify_kzg(ctx(), num_vars_x, num_vars_y, num_ops, num_cells, evals.len(), comm_ops.0, comm_mem.0, rxb.as_ptr(), ryb.as_ptr(), evb.as_ptr(),
                                   g_ops.0, g_mem.0, g2.0, tau_g2.0, proof.as_ptr(), transcript.0, &mut accepted)
    });
    accepted != 0
}

// ---- the R1CS matrices on the device (r1cs.rs): uploaded once per circuit, next to the instance --------------------------------
/// R1CSShape (r1cs.rs:22-82) on the device: the field `dev` an R1CSInstance carries next to its shape, filled at encode time the way
/// GensDev is filled for a generator set; shared by clones, rebuilt after deserialisation, dropped with the last clone
pub struct R1csHandle(pub *mut sbn_r1cs);
unsafe impl Send for R1csHandle {}
unsafe impl Sync for R1csHandle {}
impl Drop for R1csHandle { fn drop(&mut self) { if !self.0.is_null() { unsafe { sbn_r1cs_free(ctx(), self.0) } } } }
impl std::fmt::Debug for R1csHandle { fn fmt(&self, f: &mut std::fmt::Formatter<'_>) -> std::fmt::Result { write!(f, "R1csHandle({:p})", self.0) } }
#[derive(Clone, Debug, Default)]
pub struct R1csDev {
    one: Arc<OnceLock<R1csHandle>>,
}
impl R1csDev {
    /// the triplets of A, B, C (SparseMatPolynomial.M, sparse_mlpoly.rs:36-40) as ark-ff limbs; columns >= 2 num_vars are dropped by the library
    pub fn get(&self, num_cons: usize, num_vars: usize, mats: [&SparseMatPolynomial; 3]) -> *const sbn_r1cs {
        self.one.get_or_init(|| {
            let rows: Vec<Vec<u32>> = mats.iter().map(|m| m.M.iter().map(|e| e.row as u32).collect()).collect();
            let cols: Vec<Vec<u32>> = mats.iter().map(|m| m.M.iter().map(|e| u32::try_from(e.col).unwrap_or(u32::MAX)).collect()).collect();
            let vals: Vec<Vec<u8>> = mats.iter().map(|m| { let v: Vec<Scalar> = m.M.iter().map(|e| e.val).collect(); scalars_mont_bytes(&v).into_owned() }).collect();
            let rp: Vec<*const u32> = rows.iter().map(|v| v.as_ptr()).collect();
            let cp: Vec<*const u32> = cols.iter().map(|v| v.as_ptr()).collect();
            let vp: Vec<*const u8> = vals.iter().map(|v| v.as_ptr()).collect();
            let nnz: Vec<usize> = rows.iter().map(|v| v.len()).collect();
            let mut h = null_mut();
            check(unsafe { sbn_r1cs_upload(ctx(), num_cons, num_vars, rp.as_ptr(), cp.as_ptr(), vp.as_ptr(), nnz.as_ptr(), SBN_SCALARS_MONT, &mut h) });
            R1csHandle(h)
        })
        .0
    }
}
/// R1CSShape::multiply_vec (r1cs.rs:132-146) on the witness table z (2 num_vars entries, already on the device for its commitment):
/// (Az, Bz, Cz) as tables, ready for R1csRounds without leaving the device
pub fn r1cs_multiply(m: *const sbn_r1cs, z: &Table) -> (Table, Table, Table) {
    let (mut a, mut b, mut c) = (null_mut(), null_mut(), null_mut());
    check(unsafe { sbn_r1cs_multiply(ctx(), m, z.0, &mut a, &mut b, &mut c) });
    (Table(a), Table(b), Table(c))
}
/// evals_ABC of r1csproof.rs:376-387: r_A evals_A + r_B evals_B + r_C evals_C with evals_M = compute_eval_table_sparse(eq(rx))
pub fn r1cs_eval_table(m: *const sbn_r1cs, rx: &[Scalar], r_a: &Scalar, r_b: &Scalar, r_c: &Scalar) -> Table {
    let rxb = scalars_canonical(rx);
    let mut t = null_mut();
    check(unsafe { sbn_r1cs_eval_table(ctx(), m, rxb.as_ptr(), rx.len(), r_a.to_bytes().as_ptr(), r_b.to_bytes().as_ptr(), r_c.to_bytes().as_ptr(), &mut t) });
    Table(t)
}
/// R1CSShape::evaluate (r1cs.rs:126-129; snark.rs:465 "Instance evaluations") -> (A(rx, ry), B(rx, ry), C(rx, ry))
pub fn r1cs_evaluate(m: *const sbn_r1cs, rx: &[Scalar], ry: &[Scalar]) -> (Scalar, Scalar, Scalar) {
    let (rxb, ryb) = (scalars_canonical(rx), scalars_canonical(ry));
    let mut out = [0u8; 96];
    check(unsafe { sbn_r1cs_evaluate(ctx(), m, rxb.as_ptr(), rx.len(), ryb.as_ptr(), ry.len(), out.as_mut_ptr()) });
    triple(&out)
}

// ---- R1CSProof::prove (r1csproof.rs:241-459) in ONE foreign call (sbn_r1cs_proof_prove) ------------------------------------------
// The library commits the witness, builds z, runs both ZK sumchecks, the three Σ-protocols between them (KnowledgeProof, ProductProof,
// EqualityProof::prove, nizk/mod.rs:34-59, :167-227, :96-124), the opening and the whole transcript.  This side draws the RandomTape in the
// reference's order and rebuilds R1CSProof from the bytes.  Every piece of R1CSProof keeps its fields private and derives
// CanonicalDeserialize, R1CSProof included, so the proof comes back through its own deserialisation: the library's fields in declaration
// order, with the u64 length ark-serialize puts in front of each Vec.
/// PolyCommitmentGens as ONE handle: gens_n.G ‖ gens_1.G[0] with their common h (DotProductProofGens::new cuts both out of
/// MultiCommitGens::new(n + 1, label), nizk/mod.rs:412-415); cached per generator set
fn pc_bases(gens_n: &MultiCommitGens, gens_1: &MultiCommitGens) -> Arc<Bases> {
    static CACHE: OnceLock<Mutex<HashMap<(usize, [u8; 64], [u8; 64]), Arc<Bases>>>> = OnceLock::new();
    let key = (gens_n.n, point_xy_mont(&gens_n.G_affine[0]), point_xy_mont(&gens_1.G_affine[0]));
    let mut m = CACHE.get_or_init(|| Mutex::new(HashMap::new())).lock().unwrap();
    if let Some(b) = m.get(&key) { return b.clone(); }
    let mut g: Vec<u8> = gens_n.G_affine.iter().flat_map(point_xy_mont).collect();
    g.extend_from_slice(&point_xy_mont(&gens_1.G_affine[0]));
    let h = point_xy_mont(&gens_n.h_affine);
    let mut b = null_mut();
    check(unsafe { sbn_bases_upload(ctx(), g.as_ptr(), gens_n.n + 1, h.as_ptr(), SBN_POINTS_MONT, &mut b) });
    let b = Arc::new(Bases(b));
    m.insert(key, b.clone());
    b
}
/// R1CSProof::prove with a `DevTranscript`; `inst_dev` is the instance's device handle (`R1csDev::get`, uploaded at encode time)
#[allow(non_snake_case)]
pub fn r1cs_prove(
    inst: &R1CSShape,
    inst_dev: *const sbn_r1cs,
    vars: Vec<Scalar>,
    input: &[Scalar],
    gens: &R1CSGens,
    transcript: &mut DevTranscript,
    random_tape: &mut RandomTape,
) -> (R1CSProof, Vec<Scalar>, Vec<Scalar>) {
    assert!(input.len() < vars.len());                                                // r1csproof.rs:253
    let (num_cons, num_vars) = (inst.get_num_cons(), inst.get_num_vars());
    let (nx, ell) = (num_cons.trailing_zeros() as usize, num_vars.trailing_zeros() as usize);
    let (ny, ml) = (ell + 1, ell / 2);
    let lg = ell - ml;
    let (mut n_rnd, mut n_proof) = (0usize, 0usize);
    check(unsafe { sbn_r1cs_proof_sizes(num_cons, num_vars, &mut n_rnd, &mut n_proof) });
    // the draws, in the order R1CSProof::prove and the functions it calls make them
    let mut rnd = random_tape.random_vector(b"poly_blinds", 1usize << ml);            // commit_poly, r1csproof.rs:225
    rnd.extend(zk_draws(random_tape, nx, 4));                                         // phase 1
    for label in [&b"Az_blind"[..], &b"Bz_blind"[..], &b"Cz_blind"[..], &b"prod_Az_Bz_blind"[..]] { rnd.push(draw(random_tape, label)); }      // :317-322
    for label in [&b"t1"[..], &b"t2"[..]] { rnd.push(draw(random_tape, label)); }     // KnowledgeProof::prove, nizk/mod.rs:44-45
    for label in [&b"b1"[..], &b"b2"[..], &b"b3"[..], &b"b4"[..], &b"b5"[..]] { rnd.push(draw(random_tape, label)); }                         // ProductProof::prove, :181-185
    rnd.push(random_tape.random_scalar(b"r"));                                        // EqualityProof::prove, :108
    rnd.extend(zk_draws(random_tape, ny, 3));                                         // phase 2
    rnd.push(random_tape.random_scalar(b"blind_eval"));                               // r1csproof.rs:410
    rnd.push(random_tape.random_scalar(b"d"));                                        // DotProductProofLog::prove, nizk/mod.rs:458-468:
    rnd.push(random_tape.random_scalar(b"r_delta"));
    rnd.push(random_tape.random_scalar(b"r_delta"));                                  //   (r_beta is drawn under the label "r_delta" there)
    let (v1, v2) = (random_tape.random_vector(b"blinds_vec_1", lg), random_tape.random_vector(b"blinds_vec_2", lg));
    for i in 0..lg { rnd.push(v1[i]); rnd.push(v2[i]); }                              //   the library takes the pairs (v1[i], v2[i])
    rnd.push(random_tape.random_scalar(b"r"));                                        // the last EqualityProof::prove
    assert_eq!(rnd.len(), n_rnd);
    let rnd = scalars_canonical(&rnd);
    let inp = scalars_canonical(input);
    let vt = Table::upload(&vars);
    let pc = pc_bases(&gens.gens_pc.gens.gens_n, &gens.gens_pc.gens.gens_1);
    let (g3, g4) = (&gens.gens_sc.gens_3, &gens.gens_sc.gens_4);
    let (mut proof, mut rx, mut ry) = (vec![0u8; n_proof], vec![0u8; 32 * nx], vec![0u8; 32 * ny]);
    check(unsafe {
        sbn_r1cs_proof_prove(ctx(), inst_dev, vt.0, if input.is_empty() { null() } else { inp.as_ptr() }, input.len(), pc.0, g3.dev.bases(g3), g4.dev.bases(g4),
                             rnd.as_ptr(), transcript.0, proof.as_mut_ptr(), rx.as_mut_ptr(), ry.as_mut_ptr())
    });
    // out_proof -> the stream R1CSProof's derived CanonicalDeserialize reads (r1csproof.rs:187-202)
    let mut ser: Vec<u8> = Vec::with_capacity(n_proof + 128);
    let mut at = 0usize;
    let mut take = |n: usize| { let s = &proof[at..at + n]; at += n; s };
    let len = |ser: &mut Vec<u8>, n: usize| ser.extend_from_slice(&(n as u64).to_le_bytes());
    let zk = |ser: &mut Vec<u8>, p: &[u8], rounds: usize, n: usize| {                 // ZKSumcheckInstanceProof: comm_polys, comm_evals, proofs
        let stride = (6 + n) * 32;
        len(ser, rounds); for j in 0..rounds { ser.extend_from_slice(&p[stride * j..stride * j + 32]); }
        len(ser, rounds); for j in 0..rounds { ser.extend_from_slice(&p[stride * j + 32..stride * j + 64]); }
        len(ser, rounds);
        for j in 0..rounds {
            let q = &p[stride * j..stride * (j + 1)];
            ser.extend_from_slice(&q[64..128]); len(ser, n); ser.extend_from_slice(&q[128..]);      // delta, beta, z: Vec<Scalar>, z_delta, z_beta
        }
    };
    len(&mut ser, 1usize << ml); ser.extend_from_slice(take(32usize << ml));          // comm_vars: PolyCommitment { C }
    zk(&mut ser, take(320 * nx), nx, 4);                                              // sc_proof_phase1
    ser.extend_from_slice(take(128 + 352 + 64));                                      // claims_phase2, pok_claims_phase2 ([Scalar; 5] has no length), proof_eq_sc_phase1
    zk(&mut ser, take(288 * ny), ny, 3);                                              // sc_proof_phase2
    ser.extend_from_slice(take(32));                                                  // comm_vars_at_ry
    let open = take(64 * lg + 128);                                                   // PolyEvalProof { DotProductProofLog { BulletReductionProof { L_vec, R_vec }, delta, beta, z1, z2 } }
    len(&mut ser, lg); ser.extend_from_slice(&open[..32 * lg]);
    len(&mut ser, lg); ser.extend_from_slice(&open[32 * lg..64 * lg]);
    ser.extend_from_slice(&open[64 * lg..]);
    ser.extend_from_slice(take(64));                                                  // proof_eq_sc_phase2
    let r1cs_proof = R1CSProof::deserialize_compressed(&ser[..]).expect("R1CSProof from the library's bytes");
    (r1cs_proof, rx.chunks(32).map(sc).collect(), ry.chunks(32).map(sc).collect())
}
fn draw(random_tape: &mut RandomTape, label: &'static [u8]) -> Scalar { random_tape.random_scalar(label) }

// ---- the dense representation on the device (sparse_mlpoly_full.rs:120-174): built once per circuit at encode, next to R1csDev -------
/// MultiSparseMatPolynomialAsDense on the device: padded addresses, read / audit timestamps, comb_ops and comb_mem, from the same triplets
/// R1csDev uploads.  Filled by R1CSShape::commit (r1cs.rs:375-400); shared by clones, dropped with the last clone.
pub struct DenseHandle(pub *mut sbn_dense);
unsafe impl Send for DenseHandle {}
unsafe impl Sync for DenseHandle {}
impl Drop for DenseHandle { fn drop(&mut self) { if !self.0.is_null() { unsafe { sbn_dense_free(ctx(), self.0) } } } }
impl std::fmt::Debug for DenseHandle { fn fmt(&self, f: &mut std::fmt::Formatter<'_>) -> std::fmt::Result { write!(f, "DenseHandle({:p})", self.0) } }
#[derive(Clone, Debug, Default)]
pub struct DenseDev {
    one: Arc<OnceLock<DenseHandle>>,
}
impl DenseDev {
    /// the triplets of the batch (SparseMatPolynomial.M) in entry order, values as ark-ff limbs
    pub fn get(&self, num_vars_x: usize, num_vars_y: usize, mats: &[&SparseMatPolynomial]) -> *const sbn_dense {
        self.one.get_or_init(|| {
            let rows: Vec<Vec<u32>> = mats.iter().map(|m| m.M.iter().map(|e| u32::try_from(e.row).unwrap_or(u32::MAX)).collect()).collect();
            let cols: Vec<Vec<u32>> = mats.iter().map(|m| m.M.iter().map(|e| u32::try_from(e.col).unwrap_or(u32::MAX)).collect()).collect();
            let vals: Vec<Vec<u8>> = mats.iter().map(|m| { let v: Vec<Scalar> = m.M.iter().map(|e| e.val).collect(); scalars_mont_bytes(&v).into_owned() }).collect();
            let rp: Vec<*const u32> = rows.iter().map(|v| v.as_ptr()).collect();
            let cp: Vec<*const u32> = cols.iter().map(|v| v.as_ptr()).collect();
            let vp: Vec<*const u8> = vals.iter().map(|v| v.as_ptr()).collect();
            let nnz: Vec<usize> = rows.iter().map(|v| v.len()).collect();
            let mut h = null_mut();
            check(unsafe { sbn_dense_build(ctx(), num_vars_x, num_vars_y, rp.as_ptr(), cp.as_ptr(), vp.as_ptr(), nnz.as_ptr(), mats.len(), SBN_SCALARS_MONT, &mut h) });
            DenseHandle(h)
        })
        .0
    }
}
/// (N, cells, batch) of the handle: SparseMatPolyCommitment's num_ops / num_mem_cells / batch_size (sparse_mlpoly_full.rs:186-193)
pub fn dense_shape(d: *const sbn_dense) -> (usize, usize, usize) { unsafe { (sbn_dense_num_ops(d), sbn_dense_num_cells(d), sbn_dense_batch(d)) } }
/// device arrays of one side (0 = row, 1 = col) for sbn_gather_merge / sbn_hash_layer_pair: (addr[k], read_ts[k]) per matrix, audit_ts
pub fn dense_side(d: *const sbn_dense, side: c_int) -> (Vec<(*const c_void, *const c_void)>, *const c_void) {
    let b = unsafe { sbn_dense_batch(d) };
    ((0..b).map(|k| unsafe { (sbn_dense_addr_dev(d, side, k), sbn_dense_read_ts_dev(d, side, k)) }).collect(), unsafe { sbn_dense_audit_ts_dev(d, side) })
}
/// comb_ops and comb_mem: read-only tables that belong to the handle (never wrapped in `Table`, whose Drop frees)
pub fn dense_tables(d: *const sbn_dense) -> (*const sbn_table, *const sbn_table) { unsafe { (sbn_dense_comb_ops(d), sbn_dense_comb_mem(d)) } }

// ---- SparseMatPolyEvalProof::prove (sparse_mlpoly_full.rs:1700-1755) in ONE foreign call (sbn_sparse_eval_prove) -----------------------
// The library runs equalize, the eq tables, derefs and their commitment, the network's hash layers and product circuits, both product proofs,
// the 7 b + 2 evaluations, the three joint openings and the whole transcript.  This side draws the RandomTape in the reference's order and
// rebuilds the proof from the bytes through its derived CanonicalDeserialize: the library's fields in declaration order, with the u64 length
// ark-serialize puts in front of each Vec (tuples are their members one after the other).
/// the RandomTape draws of one PolyEvalProof::prove with lg bullet rounds (DotProductProofLog::prove, nizk/mod.rs:458-468)
fn open_draws(random_tape: &mut RandomTape, lg: usize) -> Vec<Scalar> {
    let mut rnd = vec![random_tape.random_scalar(b"d"), random_tape.random_scalar(b"r_delta"), random_tape.random_scalar(b"r_delta")];      // (r_beta is drawn under "r_delta")
    let (v1, v2) = (random_tape.random_vector(b"blinds_vec_1", lg), random_tape.random_vector(b"blinds_vec_2", lg));
    for i in 0..lg { rnd.push(v1[i]); rnd.push(v2[i]); }
    rnd
}
/// out_proof (include/sbn254.h) -> the stream the derived CanonicalDeserialize of SparseMatPolyEvalProof reads.  hyrax_derefs: Some((bytes of
/// comm_derefs, lg_derefs)) in the Hyrax build, None in the KZG build (comm_derefs one point, proof_derefs [proof | eval])
fn sparse_eval_stream(proof: &[u8], b: usize, m: usize, n: usize, lg_o: usize, lg_m: usize, hyrax_derefs: Option<(usize, usize)>) -> Vec<u8> {
    let mut ser: Vec<u8> = Vec::with_capacity(2 * proof.len());
    let mut at = 0usize;
    let mut take = |k: usize| { let s = &proof[at..at + k]; at += k; s };
    let len = |ser: &mut Vec<u8>, k: usize| ser.extend_from_slice(&(k as u64).to_le_bytes());
    let vec32 = |ser: &mut Vec<u8>, p: &[u8]| { len(ser, p.len() / 32); ser.extend_from_slice(p); };
    // ProductCircuitEvalProofBatched { proof: Vec<LayerProofBatched { SumcheckInstanceProof, claims_prod_left, claims_prod_right }>, claims_dotp }
    let pcepb = |ser: &mut Vec<u8>, polys: &[u8], claims: &[u8], c: usize, l: usize, d: usize| {
        len(ser, l);
        let mut po = 0usize;
        for k in 0..l {
            len(ser, k);                                                              // compressed_polys: k rounds
            for _ in 0..k {
                let q = &polys[po..po + 128]; po += 128;
                len(ser, 3); ser.extend_from_slice(&q[..32]); ser.extend_from_slice(&q[64..128]);      // CompressedUniPoly: c0, c2, c3 (unipoly.rs:87-99)
            }
            let cl = &claims[64 * c * k..64 * c * (k + 1)];
            vec32(ser, &cl[..32 * c]); vec32(ser, &cl[32 * c..]);
        }
        let dp = &claims[64 * c * l..];
        for j in 0..3 { vec32(ser, &dp[32 * d * j..32 * d * (j + 1)]); }
    };
    let open = |ser: &mut Vec<u8>, p: &[u8], lg: usize| {                             // PolyEvalProof { DotProductProofLog { BulletReductionProof { L_vec, R_vec }, delta, beta, z1, z2 } }
        len(ser, lg); ser.extend_from_slice(&p[..32 * lg]);
        len(ser, lg); ser.extend_from_slice(&p[32 * lg..64 * lg]);
        ser.extend_from_slice(&p[64 * lg..]);
    };
    match hyrax_derefs {
        Some((l_d, _)) => vec32(&mut ser, take(l_d)),                                 // comm_derefs: DerefsCommitment { PolyCommitment { C } }
        None => ser.extend_from_slice(take(32)),                                      // KZG build: DerefsCommitment { KZGPolyCommitment { commitment } }, one point, no length
    }
    for _ in 0..2 {                                                                   // ProductLayerProof.eval_row, eval_col: (Scalar, Vec, Vec, Scalar)
        ser.extend_from_slice(take(32)); vec32(&mut ser, take(32 * b)); vec32(&mut ser, take(32 * b)); ser.extend_from_slice(take(32));
    }
    vec32(&mut ser, take(32 * b)); vec32(&mut ser, take(32 * b));                     // eval_val: (Vec, Vec)
    { let polys = take(64 * m * (m - 1)).to_vec(); let claims = take(256 * m); pcepb(&mut ser, &polys, claims, 4, m, 0); }                             // proof_mem
    { let polys = take(64 * n * (n - 1)).to_vec(); let claims = take(256 * b * n + 192 * b); pcepb(&mut ser, &polys, claims, 4 * b, n, 2 * b); }       // proof_ops
    for _ in 0..2 {                                                                   // HashLayerProof.eval_row, eval_col: (Vec, Vec, Scalar)
        vec32(&mut ser, take(32 * b)); vec32(&mut ser, take(32 * b)); ser.extend_from_slice(take(32));
    }
    vec32(&mut ser, take(32 * b));                                                    // eval_val
    vec32(&mut ser, take(32 * b)); vec32(&mut ser, take(32 * b));                     // eval_derefs
    open(&mut ser, take(64 * lg_o + 128), lg_o);                                      // proof_ops
    open(&mut ser, take(64 * lg_m + 128), lg_m);                                      // proof_mem
    match hyrax_derefs {
        Some((_, lg_d)) => open(&mut ser, take(64 * lg_d + 128), lg_d),               // proof_derefs: DerefsEvalProof { PolyEvalProof }
        None => ser.extend_from_slice(take(64)),                                      // KZG build: DerefsEvalProof { proof: G1Affine, eval: Scalar }
    }
    assert_eq!(at, proof.len());
    ser
}
/// SparseMatPolyEvalProof::prove with a `DevTranscript`; `dense_dev` is the dense representation's device handle (`DenseDev::get`, built at encode time).
/// The Hyrax build: with `--features kzg` gens has no gens_derefs and `sparse_eval_prove_kzg` below takes its place.
#[cfg(not(feature = "kzg"))]
pub fn sparse_eval_prove(
    dense_dev: *const sbn_dense,
    rx: &[Scalar],
    ry: &[Scalar],
    evals: &[Scalar],
    gens: &SparseMatPolyCommitmentGens,
    transcript: &mut DevTranscript,
    random_tape: &mut RandomTape,
) -> SparseMatPolyEvalProof {
    let (num_ops, num_cells, b) = dense_shape(dense_dev);
    assert_eq!(evals.len(), b);                                                       // sparse_mlpoly_full.rs:1711
    let (n, m) = (num_ops.trailing_zeros() as usize, num_cells.trailing_zeros() as usize);
    let lg_of = |g: &crate::hyrax::PolyCommitmentGens| g.gens.gens_n.n.trailing_zeros() as usize;
    let (lg_o, lg_m, lg_d) = (lg_of(&gens.gens_ops), lg_of(&gens.gens_mem), lg_of(&gens.gens_derefs));
    let (mut n_rnd, mut n_proof) = (0usize, 0usize);
    check(unsafe { sbn_sparse_eval_sizes(rx.len(), ry.len(), num_ops, b, &mut n_rnd, &mut n_proof) });
    // HashLayerProof::prove opens derefs, then comb_ops, then comb_mem (:945-1035)
    let mut rnd = open_draws(random_tape, lg_d);
    rnd.extend(open_draws(random_tape, lg_o));
    rnd.extend(open_draws(random_tape, lg_m));
    assert_eq!(rnd.len(), n_rnd);
    let (rnd, rxb, ryb, evb) = (scalars_canonical(&rnd), scalars_canonical(rx), scalars_canonical(ry), scalars_canonical(evals));
    let g_ops = pc_bases(&gens.gens_ops.gens.gens_n, &gens.gens_ops.gens.gens_1);
    let g_mem = pc_bases(&gens.gens_mem.gens.gens_n, &gens.gens_mem.gens.gens_1);
    let g_der = pc_bases(&gens.gens_derefs.gens.gens_n, &gens.gens_derefs.gens.gens_1);
    let mut proof = vec![0u8; n_proof];
    check(unsafe {
        sbn_sparse_eval_prove(ctx(), dense_dev, rxb.as_ptr(), rx.len(), ryb.as_ptr(), ry.len(), evb.as_ptr(), g_ops.0, g_mem.0, g_der.0, rnd.as_ptr(), transcript.0,
                              proof.as_mut_ptr())
    });
    let l_d = n_proof - (32 * (13 * b + 6) + 64 * (m * (m - 1) + n * (n - 1)) + 256 * (m + b * n) + 192 * b + 64 * (lg_o + lg_m + lg_d) + 384);
    let ser = sparse_eval_stream(&proof, b, m, n, lg_o, lg_m, Some((l_d, lg_d)));
    SparseMatPolyEvalProof::deserialize_compressed(&ser[..]).expect("SparseMatPolyEvalProof from the library's bytes")
}

// ---- the opening check: PolyEvalProof::verify / verify_plain (hyrax.rs:118-151) and the n-to-1 reduction in front of it
//      (DerefsEvalProof::verify_single, sparse_mlpoly_full.rs:434-457) in ONE foreign call each ------------------------------------------
/// PolyCommitment.C (or any commitment that arrives as compressed points: comm_vars, comm_derefs) as a resident point set without h
/// (sbn_bases_from_compressed).  Err(i): point i does not decompress — what GroupElement's deserialize_compressed reports (group.rs:323-329).
pub fn bases_from_compressed(compressed: &[u8]) -> Result<Bases, usize> {
    assert_eq!(compressed.len() % 32, 0);
    let (mut b, mut bad) = (null_mut(), usize::MAX);
    let rc = unsafe { sbn_bases_from_compressed(ctx(), compressed.as_ptr(), compressed.len() / 32, &mut b, &mut bad) };
    if rc != 0 && bad != usize::MAX { return Err(bad); }
    check(rc);
    Ok(Bases(b))
}
/// the points of a PolyCommitment as the bytes `bases_from_compressed` takes: ark-serialize's stream of the Vec without its u64 length
pub fn commitment_bytes(comm: &PolyCommitment) -> Vec<u8> {
    let mut ser = Vec::with_capacity(8 + 32 * comm.C.len());
    comm.C.serialize_compressed(&mut ser).expect("PolyCommitment to bytes");
    ser.split_off(8)
}
/// PolyEvalProof as the library lays it out (out_proof of sbn_polyeval_prove): L_vec, R_vec, delta, beta, z1, z2 without the two u64 lengths
fn open_bytes(proof: &PolyEvalProof) -> Vec<u8> {
    let mut ser = Vec::new();
    proof.serialize_compressed(&mut ser).expect("PolyEvalProof to bytes");
    let lg = (ser.len() - 16 - 128) / 64;
    let mut out = Vec::with_capacity(64 * lg + 128);
    out.extend_from_slice(&ser[8..8 + 32 * lg]);
    out.extend_from_slice(&ser[16 + 32 * lg..]);
    out
}
fn verdict(accepted: c_int) -> Result<(), ProofVerifyError> {
    if accepted == 1 { Ok(()) } else { Err(ProofVerifyError::InternalError) }         // what DotProductProofLog::verify returns (nizk/mod.rs:565)
}
/// PolyEvalProof::verify with a `DevTranscript`; `comm` is the commitment on the device (`bases_from_compressed`).  The transcript moves on
/// only behind Ok(()).
#[allow(non_snake_case)]
pub fn polyeval_verify(
    proof: &PolyEvalProof,
    gens: &PolyCommitmentGens,
    transcript: &mut DevTranscript,
    r: &[Scalar],
    C_Zr: &GroupElement,
    comm: &Bases,
) -> Result<(), ProofVerifyError> {
    let g = pc_bases(&gens.gens.gens_n, &gens.gens.gens_1);
    let (rb, pb) = (scalars_canonical(r), open_bytes(proof));
    let a = affine_of(C_Zr);
    let mut xy = [0u8; 64];
    if !a.is_zero() {
        xy[..32].copy_from_slice(&limbs_le(&a.x.into_bigint().0));
        xy[32..].copy_from_slice(&limbs_le(&a.y.into_bigint().0));
    }
    let mut accepted: c_int = 0;
    check(unsafe { sbn_polyeval_verify(ctx(), g.0, comm.0, rb.as_ptr(), r.len(), xy.as_ptr(), null(), pb.as_ptr(), transcript.0, &mut accepted) });
    verdict(accepted)
}
/// PolyEvalProof::verify_plain (hyrax.rs:139-151): C_Zr = Zr.commit(0, gens_1) is formed on the device
#[allow(non_snake_case)]
pub fn polyeval_verify_plain(
    proof: &PolyEvalProof,
    gens: &PolyCommitmentGens,
    transcript: &mut DevTranscript,
    r: &[Scalar],
    Zr: &Scalar,
    comm: &Bases,
) -> Result<(), ProofVerifyError> {
    let g = pc_bases(&gens.gens.gens_n, &gens.gens.gens_1);
    let (rb, pb, zb) = (scalars_canonical(r), open_bytes(proof), Zr.to_bytes());
    let mut accepted: c_int = 0;
    check(unsafe { sbn_polyeval_verify(ctx(), g.0, comm.0, rb.as_ptr(), r.len(), null(), zb.as_ptr(), pb.as_ptr(), transcript.0, &mut accepted) });
    verdict(accepted)
}
/// DerefsEvalProof::verify_single (sparse_mlpoly_full.rs:434-457) and its two siblings in HashLayerProof::verify, which differ in `labels`
/// = (evals, challenge, claim); `evals` padded to a power of two by the caller, as the reference pads them
pub fn joint_opening_verify(
    proof: &PolyEvalProof,
    comm: &Bases,
    r: &[Scalar],
    evals: Vec<Scalar>,
    gens: &PolyCommitmentGens,
    transcript: &mut DevTranscript,
    labels: (&'static [u8], &'static [u8], &'static [u8]),
) -> Result<(), ProofVerifyError> {
    let g = pc_bases(&gens.gens.gens_n, &gens.gens.gens_1);
    let (rb, pb, eb) = (scalars_canonical(r), open_bytes(proof), scalars_canonical(&evals));
    let mut accepted: c_int = 0;
    check(unsafe {
        sbn_joint_opening_verify(ctx(), g.0, comm.0, eb.as_ptr(), evals.len(), labels.0.as_ptr(), labels.0.len(), labels.1.as_ptr(), labels.1.len(),
                                 labels.2.as_ptr(), labels.2.len(), rb.as_ptr(), r.len(), pb.as_ptr(), transcript.0, null_mut(), &mut accepted)
    });
    verdict(accepted)
}

// ---- the KZG build (--features hip,kzg): SparseMatPolyEvalProof::prove (sparse_mlpoly_full.rs:1757-1813) in ONE foreign call ---------------
/// per-cell SRS sums of one (circuit, SRS) pair (sbn_derefs_key_build): built at encode time next to `DenseDev`, dropped BEFORE the dense
/// handle and the SRS it was built from
#[cfg(feature = "kzg")]
pub struct DerefsKey(pub *mut sbn_derefs_key);
#[cfg(feature = "kzg")]
unsafe impl Send for DerefsKey {}
#[cfg(feature = "kzg")]
unsafe impl Sync for DerefsKey {}
#[cfg(feature = "kzg")]
impl Drop for DerefsKey { fn drop(&mut self) { if !self.0.is_null() { unsafe { sbn_derefs_key_free(ctx(), self.0) } } } }
#[cfg(feature = "kzg")]
impl DerefsKey {
    pub fn build(dense_dev: *const sbn_dense, srs: &KzgSrs) -> DerefsKey {
        let mut k = null_mut();
        check(unsafe { sbn_derefs_key_build(ctx(), dense_dev, srs.0, &mut k) });
        DerefsKey(k)
    }
    pub fn len(&self) -> usize { unsafe { sbn_derefs_key_len(self.0) } }
    pub fn is_empty(&self) -> bool { self.len() == 0 }
}
/// SparseMatPolyEvalProof::prove of the KZG build with a `DevTranscript`.  `srs` is gens.gens_derefs_kzg.srs.powers_g1 on the device; `key` is
/// optional (the bytes are the same with and without it).  The derefs opening draws nothing from the RandomTape (:510); the whole
/// check of this proof is `sparse_eval_verify_kzg` above.
#[cfg(feature = "kzg")]
pub fn sparse_eval_prove_kzg(
    dense_dev: *const sbn_dense,
    rx: &[Scalar],
    ry: &[Scalar],
    evals: &[Scalar],
    gens: &SparseMatPolyCommitmentGens,
    srs: &KzgSrs,
    key: Option<&DerefsKey>,
    transcript: &mut DevTranscript,
    random_tape: &mut RandomTape,
) -> SparseMatPolyEvalProof {
    let (num_ops, num_cells, b) = dense_shape(dense_dev);
    assert_eq!(evals.len(), b);                                                       // sparse_mlpoly_full.rs:1769
    let (n, m) = (num_ops.trailing_zeros() as usize, num_cells.trailing_zeros() as usize);
    let lg_of = |g: &crate::hyrax::PolyCommitmentGens| g.gens.gens_n.n.trailing_zeros() as usize;
    let (lg_o, lg_m) = (lg_of(&gens.gens_ops), lg_of(&gens.gens_mem));
    let (mut n_rnd, mut n_proof) = (0usize, 0usize);
    check(unsafe { sbn_sparse_eval_kzg_sizes(rx.len(), ry.len(), num_ops, b, &mut n_rnd, &mut n_proof) });
    let mut rnd = open_draws(random_tape, lg_o);                                      // HashLayerProof::prove: comb_ops, then comb_mem (:978-1035)
    rnd.extend(open_draws(random_tape, lg_m));
    assert_eq!(rnd.len(), n_rnd);
    let (rnd, rxb, ryb, evb) = (scalars_canonical(&rnd), scalars_canonical(rx), scalars_canonical(ry), scalars_canonical(evals));
    let g_ops = pc_bases(&gens.gens_ops.gens.gens_n, &gens.gens_ops.gens.gens_1);
    let g_mem = pc_bases(&gens.gens_mem.gens.gens_n, &gens.gens_mem.gens.gens_1);
    let mut proof = vec![0u8; n_proof];
    check(unsafe {
        sbn_sparse_eval_prove_kzg(ctx(), dense_dev, rxb.as_ptr(), rx.len(), ryb.as_ptr(), ry.len(), evb.as_ptr(), g_ops.0, g_mem.0, srs.0 as *const sbn_bases,
                                  key.map_or(null(), |k| k.0 as *const sbn_derefs_key), rnd.as_ptr(), transcript.0, proof.as_mut_ptr())
    });
    let ser = sparse_eval_stream(&proof, b, m, n, lg_o, lg_m, None);
    SparseMatPolyEvalProof::deserialize_compressed(&ser[..]).expect("SparseMatPolyEvalProof (KZG) from the library's bytes")
}

/// One pair of hashed sets of Layers::build_hash_layer (sparse_mlpoly_full.rs:762-790) and the first layer of both product circuits
/// (ProductCircuit::compute_layer, product_tree.rs:21-37) in one pass: (out_a, out_b, prod_a, prod_b).  `addr` / `ts_*` are device arrays of
/// `dense_side` (null: the cell index / zeros); `val` must hold a power of two >= 2 of entries.
pub fn hash_layer_pair_product(addr: *const c_void, val: *const sbn_table, ts_a: *const c_void, ts_a_add: u32, ts_b: *const c_void, ts_b_add: u32,
                               r_hash: &Scalar, r_multiset: &Scalar) -> (Table, Table, Table, Table) {
    let (g, tau) = (r_hash.to_bytes(), r_multiset.to_bytes());
    let (mut a, mut b, mut pa, mut pb) = (null_mut(), null_mut(), null_mut(), null_mut());
    check(unsafe { sbn_hash_layer_pair_product(ctx(), addr, val, ts_a, ts_a_add, ts_b, ts_b_add, g.as_ptr(), tau.as_ptr(), &mut a, &mut b, &mut pa, &mut pb) });
    (Table(a), Table(b), Table(pa), Table(pb))
}
