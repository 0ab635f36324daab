"""ctypes binding of include/sbn254.h.  Device pointers are plain ints (torch `tensor.data_ptr()`)."""
import ctypes as C
import os
import subprocess

_HERE = os.path.dirname(os.path.abspath(__file__))
SBN_SCALARS_MONT = 1
SBN_POINTS_MONT = 2

EXPORTED_SYMBOLS = [
    "sbn_ctx_create", "sbn_ctx_destroy", "sbn_last_error", "sbn_ctx_set_stream", "sbn_ctx_sync", "sbn_version",
    "sbn_dev_alloc", "sbn_dev_free", "sbn_dev_upload", "sbn_dev_download",
    "sbn_msm", "sbn_msm_jacobian", "sbn_bases_split_at", "sbn_bases_scale", "sbn_bases_upload", "sbn_bases_precompute", "sbn_bases_free", "sbn_bases_len", "sbn_gens_new", "sbn_bases_synthetic", "sbn_scalars_synthetic", "sbn_bases_download",
    "sbn_msm_bases", "sbn_msm_bases_dev", "sbn_commit_rows", "sbn_commit_rows_dev", "sbn_g1_compress", "sbn_g1_sum", "sbn_unipoly_from_evals", "sbn_unipoly_eval", "sbn_factored_lens",
    "sbn_table_upload", "sbn_table_from_dev", "sbn_table_free", "sbn_table_len", "sbn_table_download", "sbn_table_read0", "sbn_table_read0_many",
    "sbn_bind_top", "sbn_bind_top_many", "sbn_sc_eval_cubic", "sbn_sc_eval_cubic_batched", "sbn_sc_eval_r1cs", "sbn_sc_eval_quad",
    "sbn_sc_bind_eval_cubic_batched", "sbn_sc_bind_eval_r1cs", "sbn_sc_bind_eval_quad",
    "sbn_sumcheck_begin", "sbn_sumcheck_begin_eq", "sbn_sumcheck_round", "sbn_sumcheck_len", "sbn_sumcheck_finish", "sbn_sumcheck_free",
    "sbn_transcript_new", "sbn_transcript_clone", "sbn_transcript_free", "sbn_transcript_append_message", "sbn_transcript_challenge_bytes", "sbn_transcript_challenge_scalar",
    "sbn_transcript_state", "sbn_transcript_from_state", "sbn_fr_from_wide", "sbn_sumcheck_prove", "sbn_product_proof_prove",
    "sbn_polyeval_prove", "sbn_joint_opening_prove", "sbn_prof_last_polyeval",
    "sbn_g1_decompress", "sbn_bases_from_compressed", "sbn_polyeval_verify", "sbn_joint_opening_verify", "sbn_zk_sumcheck_prove_r1cs", "sbn_zk_sumcheck_prove_quad",
    "sbn_group_create", "sbn_group_destroy", "sbn_group_size", "sbn_group_ctx", "sbn_group_last_error", "sbn_group_bases_upload", "sbn_group_gens_new", "sbn_group_bases_precompute",
    "sbn_group_bases_free", "sbn_group_commit_rows", "sbn_group_commit_rows_dev", "sbn_group_gather_commit", "sbn_group_msm", "sbn_group_bases_upload_ranges", "sbn_group_bases_synthetic_ranges", "sbn_group_range", "sbn_group_msm_bases", "sbn_group_msm_bases_dev",
    "sbn_eq_evals", "sbn_hash_layer", "sbn_hash_layer_pair", "sbn_hash_layer_pair_product", "sbn_product_layer", "sbn_product_circuit", "sbn_product_circuit_many", "sbn_table_halves", "sbn_table_slice", "sbn_table_dot", "sbn_table_evaluate", "sbn_table_evaluate_many", "sbn_table_bound", "sbn_gather_merge", "sbn_gather_merge_rows", "sbn_commit_table", "sbn_bullet_begin", "sbn_bullet_begin_scaled", "sbn_bullet_free", "sbn_bullet_len", "sbn_bullet_cross", "sbn_bullet_fold_cross", "sbn_bullet_fold", "sbn_bullet_finish", "sbn_prof_enable", "sbn_prof_reset", "sbn_prof_count", "sbn_prof_get", "sbn_prof_last_job", "sbn_prof_last_acc",
    "sbn_kzg_srs_upload", "sbn_kzg_srs_from_tau", "sbn_kzg_commit", "sbn_poly_div_linear", "sbn_kzg_open", "sbn_kzg_open_batched",
    "sbn_r1cs_upload", "sbn_r1cs_free", "sbn_r1cs_multiply", "sbn_r1cs_eval_table", "sbn_r1cs_evaluate",
    "sbn_r1cs_proof_sizes", "sbn_r1cs_proof_prove", "sbn_zk_sumcheck_verify", "sbn_r1cs_proof_verify", "sbn_g1_small_sums", "sbn_sparse_eval_verify", "sbn_sparse_eval_sizes", "sbn_sparse_eval_prove",
    "sbn_derefs_key_build", "sbn_derefs_key_free", "sbn_derefs_key_len", "sbn_derefs_key_download", "sbn_derefs_key_commit",
    "sbn_sparse_eval_kzg_sizes", "sbn_sparse_eval_prove_kzg",
    "sbn_g2_prepare", "sbn_g2_lines_free", "sbn_pairing_products", "sbn_kzg_verify", "sbn_kzg_verify_batched", "sbn_sparse_eval_verify_kzg",
    "sbn_dense_build", "sbn_dense_free", "sbn_dense_num_ops", "sbn_dense_num_cells", "sbn_dense_batch", "sbn_dense_addr_dev", "sbn_dense_read_ts_dev",
    "sbn_dense_audit_ts_dev", "sbn_dense_comb_ops", "sbn_dense_comb_mem",
    "sbn_r1cs_is_sat", "sbn_snark_gens_new", "sbn_snark_gens_get", "sbn_snark_gens_free", "sbn_snark_encode", "sbn_snark_key_from_comm", "sbn_snark_key_comm", "sbn_snark_key_dense",
    "sbn_snark_key_free", "sbn_snark_sizes", "sbn_snark_is_sat", "sbn_snark_prove", "sbn_snark_verify", "sbn_snark_prove_kzg", "sbn_snark_verify_kzg",
    "sbn_nizk_gens_new", "sbn_nizk_instance_new", "sbn_nizk_instance_free", "sbn_nizk_instance_r1cs", "sbn_nizk_sizes", "sbn_nizk_is_sat", "sbn_nizk_prove", "sbn_nizk_verify",
    "sbn_circom_r1cs_load", "sbn_circom_r1cs_info", "sbn_circom_r1cs_download", "sbn_circom_r1cs_free", "sbn_r1cs_from_circom", "sbn_nizk_instance_from_circom",
    "sbn_snark_encode_circom", "sbn_circom_wtns_load",
    "sbn_kzg_srs_load", "sbn_kzg_srs_check", "sbn_kzg_srs_save", "sbn_kzg_srs_g2_from_tau", "sbn_ptau_scan", "sbn_kzg_srs_load_ptau",
    "sbn_circom_r1cs_digest", "sbn_random_tape_new", "sbn_random_tape_scalars", "sbn_random_tape_free", "sbn_random_tape_last_error",
    "sbn_zk_sumcheck_draw_rnd", "sbn_polyeval_draw_rnd", "sbn_r1cs_proof_draw_rnd", "sbn_sparse_eval_draw_rnd", "sbn_snark_draw_rnd", "sbn_nizk_draw_rnd",
]
SBN_EUNSAT = -5
SBN_SNARK_CHECK_SAT = 1
SBN_SRS_CHECK = 1


class SbnError(RuntimeError):
    pass


class SbnUnsat(SbnError):
    """SBN_EUNSAT: snark_prove with check_sat met a witness that does not satisfy the instance"""


def lib_path():
    return os.path.join(_HERE, "libsbn254_hip.so")


def build_library():
    """hipcc --offload-arch=gfx950 (cross-compiles without a GPU)."""
    subprocess.run(["make", "-s", "-C", _HERE], check=True)
    return lib_path()


_LIB = None


def lib():
    global _LIB
    if _LIB is None:
        # torch bundles its own libamdhip64 (SONAME libamdhip64.so.7, like /opt/rocm's).  Import it FIRST so that this
        # library binds to the HIP runtime torch already loaded; the other order puts two runtimes in one process and
        # the second one finds no GPU.  Without torch (the Rust shim) /opt/rocm's runtime is used.
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
        p = lib_path()
        if not os.path.exists(p):
            raise SbnError(f"{p} is missing: run `make -C {_HERE}` (or __graft_entry__.build()); there is no CPU fallback")
        L = C.CDLL(p)
        L.sbn_last_error.restype = C.c_char_p
        L.sbn_version.restype = C.c_char_p
        missing = [s for s in EXPORTED_SYMBOLS if not hasattr(L, s)]
        if missing:
            raise SbnError(f"{p} does not export {missing}; rebuild it")
        L.sbn_bases_len.restype = C.c_size_t
        L.sbn_table_len.restype = C.c_size_t
        L.sbn_bullet_len.restype = C.c_size_t
        L.sbn_sumcheck_len.restype = C.c_size_t
        L.sbn_group_size.restype = C.c_size_t
        L.sbn_group_ctx.restype = C.c_void_p
        L.sbn_group_last_error.restype = C.c_char_p
        L.sbn_factored_lens.restype = None
        for name in ("sbn_ctx_destroy", "sbn_bases_free", "sbn_table_free", "sbn_bullet_free", "sbn_sumcheck_free", "sbn_group_destroy", "sbn_group_bases_free", "sbn_group_range", "sbn_r1cs_free", "sbn_dense_free", "sbn_transcript_free"):
            getattr(L, name).restype = None
        for name in ("sbn_dense_num_ops", "sbn_dense_num_cells", "sbn_dense_batch"):
            getattr(L, name).restype = C.c_size_t; getattr(L, name).argtypes = [C.c_void_p]
        for name in ("sbn_dense_addr_dev", "sbn_dense_read_ts_dev"):
            getattr(L, name).restype = C.c_void_p; getattr(L, name).argtypes = [C.c_void_p, C.c_int, C.c_size_t]
        L.sbn_transcript_free.argtypes = [C.c_void_p]
        L.sbn_sumcheck_prove.argtypes = [C.c_void_p] * 7
        L.sbn_product_proof_prove.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t] + [C.c_void_p] * 5
        L.sbn_polyeval_prove.argtypes = [C.c_void_p] * 5 + [C.c_size_t] + [C.c_void_p] * 9
        L.sbn_joint_opening_prove.argtypes = [C.c_void_p] * 4 + [C.c_size_t] + [C.c_void_p, C.c_size_t] * 3 + [C.c_void_p, C.c_size_t] + [C.c_void_p] * 9
        L.sbn_g1_decompress.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]
        L.sbn_bases_from_compressed.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]
        L.sbn_polyeval_verify.argtypes = [C.c_void_p] * 4 + [C.c_size_t] + [C.c_void_p] * 5
        L.sbn_joint_opening_verify.argtypes = [C.c_void_p] * 4 + [C.c_size_t] + [C.c_void_p, C.c_size_t] * 3 + [C.c_void_p, C.c_size_t] + [C.c_void_p] * 4
        L.sbn_zk_sumcheck_prove_r1cs.argtypes = [C.c_void_p] * 15
        L.sbn_zk_sumcheck_prove_quad.argtypes = [C.c_void_p] * 13
        L.sbn_r1cs_proof_sizes.argtypes = [C.c_size_t, C.c_size_t, C.c_void_p, C.c_void_p]
        L.sbn_r1cs_proof_prove.argtypes = [C.c_void_p] * 4 + [C.c_size_t] + [C.c_void_p] * 8
        L.sbn_zk_sumcheck_verify.argtypes = [C.c_void_p] * 4 + [C.c_size_t] * 2 + [C.c_void_p] * 5
        L.sbn_r1cs_proof_verify.argtypes = [C.c_void_p, C.c_size_t, C.c_size_t, C.c_void_p, C.c_size_t] + [C.c_void_p] * 9
        L.sbn_g1_small_sums.argtypes = [C.c_void_p] * 4 + [C.c_size_t] + [C.c_void_p] * 2
        L.sbn_sparse_eval_verify.argtypes = [C.c_void_p] + [C.c_size_t] * 5 + [C.c_void_p] * 11
        L.sbn_sparse_eval_sizes.argtypes = [C.c_size_t] * 4 + [C.c_void_p] * 2
        L.sbn_sparse_eval_prove.argtypes = [C.c_void_p] * 3 + [C.c_size_t, C.c_void_p, C.c_size_t] + [C.c_void_p] * 7
        L.sbn_sparse_eval_kzg_sizes.argtypes = [C.c_size_t] * 4 + [C.c_void_p] * 2
        L.sbn_sparse_eval_prove_kzg.argtypes = [C.c_void_p] * 3 + [C.c_size_t, C.c_void_p, C.c_size_t] + [C.c_void_p] * 8
        L.sbn_derefs_key_build.argtypes = [C.c_void_p] * 4
        L.sbn_derefs_key_free.restype = None; L.sbn_derefs_key_free.argtypes = [C.c_void_p] * 2
        L.sbn_derefs_key_len.restype = C.c_size_t; L.sbn_derefs_key_len.argtypes = [C.c_void_p]
        L.sbn_derefs_key_download.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t, C.c_void_p, C.c_void_p]
        L.sbn_derefs_key_commit.argtypes = [C.c_void_p] * 6
        L.sbn_g2_prepare.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p]
        L.sbn_g2_lines_free.restype = None; L.sbn_g2_lines_free.argtypes = [C.c_void_p] * 2
        L.sbn_pairing_products.argtypes = [C.c_void_p] * 4 + [C.c_size_t] + [C.c_void_p] * 2
        L.sbn_kzg_verify.argtypes = [C.c_void_p] * 8
        L.sbn_sparse_eval_verify_kzg.argtypes = [C.c_void_p] + [C.c_size_t] * 5 + [C.c_void_p] * 12
        L.sbn_kzg_verify_batched.argtypes = [C.c_void_p] * 4 + [C.c_size_t] + [C.c_void_p] * 5
        L.sbn_dense_audit_ts_dev.restype = C.c_void_p; L.sbn_dense_audit_ts_dev.argtypes = [C.c_void_p, C.c_int]
        for name in ("sbn_dense_comb_ops", "sbn_dense_comb_mem"):
            getattr(L, name).restype = C.c_void_p; getattr(L, name).argtypes = [C.c_void_p]
        L.sbn_r1cs_is_sat.argtypes = [C.c_void_p] * 4 + [C.c_size_t] + [C.c_void_p] * 3
        L.sbn_snark_gens_new.argtypes = [C.c_void_p] + [C.c_size_t] * 4 + [C.c_void_p]
        L.sbn_snark_gens_get.restype = C.c_void_p; L.sbn_snark_gens_get.argtypes = [C.c_void_p, C.c_int]
        L.sbn_snark_gens_free.restype = None; L.sbn_snark_gens_free.argtypes = [C.c_void_p] * 2
        L.sbn_snark_encode.argtypes = [C.c_void_p] + [C.c_size_t] * 3 + [C.c_void_p] * 4 + [C.c_uint32] + [C.c_void_p] * 2
        L.sbn_snark_key_from_comm.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
        L.sbn_snark_key_comm.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
        L.sbn_snark_key_dense.restype = C.c_void_p; L.sbn_snark_key_dense.argtypes = [C.c_void_p]
        L.sbn_snark_key_free.restype = None; L.sbn_snark_key_free.argtypes = [C.c_void_p] * 2
        L.sbn_snark_sizes.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
        L.sbn_snark_is_sat.argtypes = [C.c_void_p] * 4 + [C.c_size_t] + [C.c_void_p] * 3
        L.sbn_snark_prove.argtypes = [C.c_void_p] * 4 + [C.c_size_t, C.c_void_p, C.c_uint32] + [C.c_void_p] * 3
        L.sbn_snark_verify.argtypes = [C.c_void_p] * 3 + [C.c_size_t] + [C.c_void_p] * 2 + [C.c_size_t] + [C.c_void_p] * 2
        L.sbn_snark_prove_kzg.argtypes = [C.c_void_p] * 4 + [C.c_size_t] + [C.c_void_p] * 3 + [C.c_uint32] + [C.c_void_p] * 3
        L.sbn_snark_verify_kzg.argtypes = [C.c_void_p] * 3 + [C.c_size_t] + [C.c_void_p] * 4 + [C.c_size_t] + [C.c_void_p] * 2
        L.sbn_nizk_gens_new.argtypes = [C.c_void_p] + [C.c_size_t] * 3 + [C.c_void_p]
        L.sbn_nizk_instance_new.argtypes = [C.c_void_p] + [C.c_size_t] * 3 + [C.c_void_p] * 4 + [C.c_uint32, C.c_void_p, C.c_size_t, C.c_void_p]
        L.sbn_nizk_instance_free.restype = None; L.sbn_nizk_instance_free.argtypes = [C.c_void_p] * 2
        L.sbn_nizk_instance_r1cs.restype = C.c_void_p; L.sbn_nizk_instance_r1cs.argtypes = [C.c_void_p]
        L.sbn_nizk_sizes.argtypes = [C.c_void_p] * 3
        L.sbn_nizk_is_sat.argtypes = [C.c_void_p] * 4 + [C.c_size_t] + [C.c_void_p] * 3
        L.sbn_nizk_prove.argtypes = [C.c_void_p] * 4 + [C.c_size_t, C.c_void_p, C.c_uint32] + [C.c_void_p] * 3
        L.sbn_nizk_verify.argtypes = [C.c_void_p] * 3 + [C.c_size_t] + [C.c_void_p] * 2 + [C.c_size_t] + [C.c_void_p] * 2
        L.sbn_circom_r1cs_load.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
        L.sbn_circom_r1cs_info.argtypes = [C.c_void_p] * 2
        L.sbn_circom_r1cs_download.argtypes = [C.c_void_p, C.c_void_p, C.c_int] + [C.c_void_p] * 3
        L.sbn_circom_r1cs_free.restype = None; L.sbn_circom_r1cs_free.argtypes = [C.c_void_p] * 2
        L.sbn_r1cs_from_circom.argtypes = [C.c_void_p] * 3
        L.sbn_nizk_instance_from_circom.argtypes = [C.c_void_p] * 3 + [C.c_size_t, C.c_void_p]
        L.sbn_snark_encode_circom.argtypes = [C.c_void_p] * 4
        L.sbn_circom_wtns_load.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t] + [C.c_void_p] * 3
        L.sbn_kzg_srs_load.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_uint32] + [C.c_void_p] * 5
        L.sbn_kzg_srs_check.argtypes = [C.c_void_p] * 6
        L.sbn_kzg_srs_save.argtypes = [C.c_void_p] * 4 + [C.c_uint32, C.c_void_p, C.c_size_t, C.c_void_p]
        L.sbn_kzg_srs_g2_from_tau.argtypes = [C.c_void_p] * 3
        L.sbn_ptau_scan.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p]
        L.sbn_kzg_srs_load_ptau.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t, C.c_uint32] + [C.c_void_p] * 5
        L.sbn_circom_r1cs_digest.argtypes = [C.c_void_p] * 3
        L.sbn_random_tape_new.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]
        L.sbn_random_tape_scalars.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t, C.c_void_p]
        L.sbn_random_tape_free.restype = None; L.sbn_random_tape_free.argtypes = [C.c_void_p]
        L.sbn_random_tape_last_error.restype = C.c_char_p; L.sbn_random_tape_last_error.argtypes = [C.c_void_p]
        L.sbn_zk_sumcheck_draw_rnd.argtypes = [C.c_size_t] * 2 + [C.c_void_p] * 2 + [C.c_size_t]
        L.sbn_polyeval_draw_rnd.argtypes = [C.c_size_t] + [C.c_void_p] * 2 + [C.c_size_t]
        L.sbn_r1cs_proof_draw_rnd.argtypes = [C.c_size_t] * 2 + [C.c_void_p] * 2 + [C.c_size_t]
        L.sbn_sparse_eval_draw_rnd.argtypes = [C.c_size_t] * 4 + [C.c_int] + [C.c_void_p] * 2 + [C.c_size_t]
        L.sbn_snark_draw_rnd.argtypes = [C.c_void_p, C.c_int] + [C.c_void_p] * 2 + [C.c_size_t]
        L.sbn_nizk_draw_rnd.argtypes = [C.c_void_p] * 3 + [C.c_size_t]
        _LIB = L
    return _LIB


HARNESS_STAGES = ["r1cs_sat_proof", "eq_evals", "derefs_computation", "derefs_commitment", "network_construction", "network_proof",
                  "sub_witness_commit", "sub_phase1_sumcheck", "sub_phase2_sumcheck", "sub_witness_opening", "sub_ops_sumchecks", "sub_mem_sumchecks",
                  "sub_evaluations", "sub_openings"]


class HarnessParams(C.Structure):
    _fields_ = [("log_ops", C.c_int32), ("log_mem", C.c_int32), ("log_cons", C.c_int32), ("stateful_sumcheck", C.c_int32),
                ("lookup_bytes_sat", C.c_uint64), ("lookup_bytes_eval", C.c_uint64), ("seed", C.c_uint64), ("rounds_out", C.c_uint32 * 4),
                ("passes", C.c_uint32), ("trace_markers", C.c_uint32)]


_HARNESS = None


def harness_lib():
    """libsbn_prove_harness.so: the compiled caller of the C ABI (harness/prove_stages.cpp)"""
    global _HARNESS
    if _HARNESS is None:
        lib()                                                  # the product library first (the harness links against it)
        p = os.path.join(_HERE, "libsbn_prove_harness.so")
        if not os.path.exists(p):
            raise SbnError(f"{p} is missing: run `make -C {_HERE}`")
        _HARNESS = C.CDLL(p)
    return _HARNESS


def harness_prove(ctx, log_ops, log_mem, log_cons, stateful=True, lookup_bytes_sat=0, lookup_bytes_eval=0, seed=1, trace_cap=0, passes=1, trace_markers=False):
    """a keyless-shaped prove's device-side stages from compiled code -> (stage_ms dict, digest, trace bytes, rounds dict); with passes > 1
    the proves run back to back on one setup and the fastest pass's times are returned (the trace is the last pass's)"""
    prm = HarnessParams(log_ops, log_mem, log_cons, 1 if stateful else 0, lookup_bytes_sat, lookup_bytes_eval, seed)
    prm.passes = passes
    prm.trace_markers = 1 if trace_markers else 0
    ms = (C.c_double * 16)(); dig = (C.c_uint8 * 32)(); err = C.create_string_buffer(512)
    tr = (C.c_uint8 * trace_cap)() if trace_cap else None; tl = C.c_size_t(0)
    rc = harness_lib().sbn_harness_prove(ctx.h, C.byref(prm), ms, dig, tr, C.c_size_t(trace_cap), C.byref(tl), err, C.c_size_t(512))
    if rc:
        raise SbnError("sbn_harness_prove: " + err.value.decode())
    stages = {n: ms[i] for i, n in enumerate(HARNESS_STAGES)}
    rounds = {"sumcheck_rounds_ops": prm.rounds_out[0], "sumcheck_rounds_mem": prm.rounds_out[1], "bullet_rounds": prm.rounds_out[2], "layers": prm.rounds_out[3]}
    return stages, bytes(dig), (bytes(tr[:tl.value]) if trace_cap else b""), rounds


def _three_mats(what, mats):
    """A, B, C as (rows, cols, vals) triplets -> (the arrays to keep alive, rows[3], cols[3], vals[3], nnz[3]) as the C ABI takes a circuit"""
    import numpy as np
    if len(mats) != 3:
        raise ValueError(f"{what}: mats must hold A, B and C")
    keep, rows, cols, vals, nnz = [], (C.c_void_p * 3)(), (C.c_void_p * 3)(), (C.c_void_p * 3)(), (C.c_size_t * 3)()
    for m, (r, c, v) in enumerate(mats):
        r = np.ascontiguousarray(r, dtype=np.uint32); c = np.ascontiguousarray(c, dtype=np.uint32)
        v = np.frombuffer(v, dtype=np.uint8) if isinstance(v, (bytes, bytearray)) else np.ascontiguousarray(v, dtype=np.uint8).reshape(-1)
        n = len(r)
        if len(c) != n or len(v) != 32 * n:
            raise ValueError(f"{what}: matrix {m}: {n} rows, {len(c)} cols, {len(v)} value bytes")
        keep += [r, c, v]
        nnz[m] = n
        rows[m] = r.ctypes.data if n else None; cols[m] = c.ctypes.data if n else None; vals[m] = v.ctypes.data if n else None
    return keep, rows, cols, vals, nnz


def _ptr(x):
    """host bytes-like -> char pointer; None -> NULL"""
    if x is None:
        return None
    if isinstance(x, (bytes, bytearray)):
        return (C.c_uint8 * len(x)).from_buffer_copy(x) if isinstance(x, bytes) else (C.c_uint8 * len(x)).from_buffer(x)
    if hasattr(x, "ctypes"):  # numpy array
        return x.ctypes.data_as(C.POINTER(C.c_uint8))
    raise TypeError(type(x))


def g1_compress(xy):
    n = len(xy) // 64
    out = (C.c_uint8 * (32 * n))()
    rc = lib().sbn_g1_compress(_ptr(xy), C.c_size_t(n), out)
    if rc:
        raise SbnError(f"sbn_g1_compress rc={rc}")
    return bytes(out)


def kzg_srs_g2_from_tau(tau):
    """sbn_kzg_srs_g2_from_tau (host only) -> (g2_xy, tau_g2_xy): arkworks' G2 generator and [tau] of it, 128 canonical bytes each"""
    g2 = (C.c_uint8 * 128)(); tg2 = (C.c_uint8 * 128)()
    rc = lib().sbn_kzg_srs_g2_from_tau(_ptr(tau), g2, tg2)
    if rc:
        raise SbnError(f"sbn_kzg_srs_g2_from_tau rc={rc}: tau must be canonical and non-zero")
    return bytes(g2), bytes(tg2)


class PtauInfo(C.Structure):
    """sbn_ptau_info: what sbn_ptau_scan reads from a .ptau file's section table and header section"""
    _fields_ = [("power", C.c_uint32), ("ceremony_power", C.c_uint32), ("n_g1", C.c_uint64), ("n_g2", C.c_uint64), ("off_g1", C.c_uint64), ("off_g2", C.c_uint64)]


def ptau_scan(data):
    """sbn_ptau_scan (host only) -> PtauInfo; SbnError for a file the load would refuse before it reads a point"""
    info = PtauInfo()
    rc = lib().sbn_ptau_scan(_ptr(data) if len(data) else None, C.c_size_t(len(data)), C.byref(info))
    if rc:
        raise SbnError(f"sbn_ptau_scan rc={rc}: not a .ptau file this library loads")
    return info


class RandomTape:
    """RandomTape (random.rs) behind the C ABI, host only: no Context.  name: b"snark_proof" for snark_prove, b"proof" for nizk_prove (snark.rs:438, :210).
    init: 32 canonical bytes — a tape started from the same init gives the draws the reference's tape gives; a fixed init is for tests — or None:
    the library takes it from the operating system.  Every draw_* fills rnd exactly as the matching prove call takes it and advances the tape"""

    def __init__(self, name, init=None):
        self.h = C.c_void_p()
        rc = lib().sbn_random_tape_new(_ptr(name) if name else None, C.c_size_t(len(name)), _ptr(init), C.byref(self.h))
        if rc:
            self.h = None
            raise SbnError(f"sbn_random_tape_new rc={rc}: {lib().sbn_random_tape_last_error(None).decode()}")

    def _chk(self, rc, what):
        if rc:
            raise SbnError(f"{what} rc={rc}: {lib().sbn_random_tape_last_error(self.h).decode()}")

    def scalars(self, label, n=1):
        """random_scalar / random_vector: n x challenge_scalar(label) -> n x 32 canonical bytes"""
        out = (C.c_uint8 * (32 * max(n, 1)))()
        self._chk(lib().sbn_random_tape_scalars(self.h, _ptr(label) if label else None, C.c_size_t(len(label)), C.c_size_t(n), out), "sbn_random_tape_scalars")
        return bytes(out)[:32 * n]

    def _plan(self, fn, what, args, count):
        out = (C.c_uint8 * (32 * max(count, 1)))()
        self._chk(fn(*args, self.h, out, C.c_size_t(count)), what)
        return bytes(out)[:32 * count]

    def draw_zk_sumcheck(self, num_rounds, n):
        return self._plan(lib().sbn_zk_sumcheck_draw_rnd, "sbn_zk_sumcheck_draw_rnd", (C.c_size_t(num_rounds), C.c_size_t(n)), num_rounds * (n + 4))

    def draw_polyeval(self, ell):
        return self._plan(lib().sbn_polyeval_draw_rnd, "sbn_polyeval_draw_rnd", (C.c_size_t(ell),), 3 + 2 * factored_lens(ell)[1])

    def draw_r1cs_proof(self, num_cons, num_vars):
        n = C.c_size_t(0)
        if lib().sbn_r1cs_proof_sizes(C.c_size_t(num_cons), C.c_size_t(num_vars), C.byref(n), None):
            raise SbnError(f"sbn_r1cs_proof_sizes refuses {num_cons} x {num_vars}")
        return self._plan(lib().sbn_r1cs_proof_draw_rnd, "sbn_r1cs_proof_draw_rnd", (C.c_size_t(num_cons), C.c_size_t(num_vars)), n.value)

    def draw_sparse_eval(self, nx, ny, num_ops, batch, kzg=False):
        n = C.c_size_t(0)
        if (lib().sbn_sparse_eval_kzg_sizes if kzg else lib().sbn_sparse_eval_sizes)(C.c_size_t(nx), C.c_size_t(ny), C.c_size_t(num_ops), C.c_size_t(batch), C.byref(n), None):
            raise SbnError(f"sbn_sparse_eval_sizes refuses ({nx}, {ny}, {num_ops}, {batch})")
        return self._plan(lib().sbn_sparse_eval_draw_rnd, "sbn_sparse_eval_draw_rnd", (C.c_size_t(nx), C.c_size_t(ny), C.c_size_t(num_ops), C.c_size_t(batch), int(kzg)), n.value)

    def draw_snark(self, key, kzg=False):
        """the rnd of Context.snark_prove / snark_prove_kzg on this SnarkKey"""
        return self._plan(lib().sbn_snark_draw_rnd, "sbn_snark_draw_rnd", (key.h, int(kzg)), key.sizes(kzg)[0])

    def draw_nizk(self, inst):
        """the rnd of Context.nizk_prove on this NizkInst"""
        return self._plan(lib().sbn_nizk_draw_rnd, "sbn_nizk_draw_rnd", (inst.h,), inst.sizes()[0])

    def free(self):
        if self.h:
            lib().sbn_random_tape_free(self.h)
            self.h = None


def g1_sum(xy):
    """host-side sum of canonical affine points (the fold after the all-gather of per-GPU partials)"""
    n = len(xy) // 64
    out = (C.c_uint8 * 64)(); inf = C.c_int()
    rc = lib().sbn_g1_sum(_ptr(xy), C.c_size_t(n), out, C.byref(inf))
    if rc:
        raise SbnError(f"sbn_g1_sum rc={rc}")
    return bytes(out), bool(inf.value)


def unipoly_from_evals(evals):
    """UniPoly::from_evals (unipoly.rs:28-59), host side"""
    n = len(evals) // 32; out = (C.c_uint8 * (32 * n))()
    rc = lib().sbn_unipoly_from_evals(_ptr(evals), C.c_size_t(n), out)
    if rc:
        raise SbnError(f"sbn_unipoly_from_evals rc={rc}")
    return bytes(out)


def unipoly_eval(coeffs, r):
    out = (C.c_uint8 * 32)()
    rc = lib().sbn_unipoly_eval(_ptr(coeffs), C.c_size_t(len(coeffs) // 32), _ptr(r), out)
    if rc:
        raise SbnError(f"sbn_unipoly_eval rc={rc}")
    return bytes(out)


def r1cs_proof_sizes(num_cons, num_vars):
    """sbn_r1cs_proof_sizes -> (scalars of rnd, bytes of the proof) of sbn_r1cs_proof_prove at this shape"""
    a, b = C.c_size_t(0), C.c_size_t(0)
    rc = lib().sbn_r1cs_proof_sizes(C.c_size_t(num_cons), C.c_size_t(num_vars), C.byref(a), C.byref(b))
    if rc != 0:
        raise SbnError(f"sbn_r1cs_proof_sizes: {num_cons} x {num_vars} is a shape the call refuses (rc={rc})")
    return a.value, b.value


def factored_lens(ell):
    a, b = C.c_size_t(), C.c_size_t()
    lib().sbn_factored_lens(C.c_size_t(ell), C.byref(a), C.byref(b))
    return a.value, b.value


class Bases:
    def __init__(self, ctx, handle):
        self.ctx, self.h = ctx, handle

    def __len__(self):
        return lib().sbn_bases_len(self.h)

    def free(self):
        if self.h:
            lib().sbn_bases_free(self.ctx.h, self.h)
            self.h = None


class Bullet:
    def __init__(self, ctx, handle):
        self.ctx, self.h = ctx, handle

    def __len__(self):
        return lib().sbn_bullet_len(self.h)

    def free(self):
        if self.h:
            lib().sbn_bullet_free(self.ctx.h, self.h)
            self.h = None


def fr_from_wide(b64):
    """Fr::from_le_bytes_mod_order on 64 bytes -> 32 canonical bytes (host side)"""
    if len(b64) != 64:
        raise ValueError("64 bytes are needed")
    out = (C.c_uint8 * 32)()
    rc = lib().sbn_fr_from_wide(_ptr(b64), out)
    if rc:
        raise SbnError(f"sbn_fr_from_wide rc={rc}")
    return bytes(out)


class Transcript:
    """Merlin v1.0 transcript on the host (sbn_transcript_*), with Merlin's method names; no device needed"""

    def __init__(self, label=None, _handle=None):
        if _handle is None:
            _handle = C.c_void_p()
            self._chk(lib().sbn_transcript_new(_ptr(label), C.c_size_t(len(label)), C.byref(_handle)), "sbn_transcript_new")
        self.h = _handle

    @staticmethod
    def _chk(rc, what):
        if rc:
            raise SbnError(f"{what} rc={rc}")

    def append_message(self, label, msg):
        self._chk(lib().sbn_transcript_append_message(self.h, _ptr(label), C.c_size_t(len(label)), _ptr(msg), C.c_size_t(len(msg))), "sbn_transcript_append_message")

    def append_scalar(self, label, scalar32):
        self.append_message(label, scalar32)

    def challenge_bytes(self, label, n):
        out = (C.c_uint8 * max(n, 1))()
        self._chk(lib().sbn_transcript_challenge_bytes(self.h, _ptr(label), C.c_size_t(len(label)), out, C.c_size_t(n)), "sbn_transcript_challenge_bytes")
        return bytes(out[:n])

    def challenge_scalar(self, label):
        out = (C.c_uint8 * 32)()
        self._chk(lib().sbn_transcript_challenge_scalar(self.h, _ptr(label), C.c_size_t(len(label)), out), "sbn_transcript_challenge_scalar")
        return bytes(out)

    def state(self):
        out = (C.c_uint8 * 203)()
        self._chk(lib().sbn_transcript_state(self.h, out), "sbn_transcript_state")
        return bytes(out)

    @classmethod
    def from_state(cls, rec):
        if len(rec) != 203:
            raise ValueError("a transcript state record has 203 bytes")
        h = C.c_void_p()
        cls._chk(lib().sbn_transcript_from_state(_ptr(rec), C.byref(h)), "sbn_transcript_from_state")
        return cls(_handle=h)

    def clone(self):
        h = C.c_void_p()
        self._chk(lib().sbn_transcript_clone(self.h, C.byref(h)), "sbn_transcript_clone")
        return Transcript(_handle=h)

    def free(self):
        if self.h:
            lib().sbn_transcript_free(self.h)
            self.h = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class Sumcheck:
    """prove_cubic_batched (sumcheck.rs:165-330) as a device-resident state (sbn_sumcheck_*)"""

    def __init__(self, ctx, handle, n_par, n_seq):
        self.ctx, self.h, self.ntab = ctx, handle, 2 * n_par + (1 if n_par else 0) + 3 * n_seq

    def __len__(self):
        return lib().sbn_sumcheck_len(self.h)

    def round(self, r):
        out = (C.c_uint8 * 96)()
        self.ctx._chk(lib().sbn_sumcheck_round(self.ctx.h, self.h, _ptr(r), out), "sbn_sumcheck_round")
        return bytes(out)

    def finish(self):
        out = (C.c_uint8 * (32 * self.ntab))()
        self.ctx._chk(lib().sbn_sumcheck_finish(self.ctx.h, self.h, out), "sbn_sumcheck_finish")
        return [bytes(out[32 * t:32 * t + 32]) for t in range(self.ntab)]

    def free(self):
        if self.h:
            lib().sbn_sumcheck_free(self.ctx.h, self.h)
            self.h = None


class Table:
    def __init__(self, ctx, handle):
        self.ctx, self.h = ctx, handle

    def __len__(self):
        return lib().sbn_table_len(self.h)

    def free(self):
        if self.h:
            lib().sbn_table_free(self.ctx.h, self.h)
            self.h = None


class _BorrowedTable(Table):
    """a table owned by another handle: never passed to sbn_table_free"""

    def free(self):
        self.h = None


class R1cs:
    """R1CSShape (r1cs.rs:22-82) resident on the device (sbn_r1cs_upload)"""

    def __init__(self, ctx, handle, num_cons, num_vars):
        self.ctx, self.h, self.num_cons, self.num_vars = ctx, handle, num_cons, num_vars

    def free(self):
        if self.h:
            lib().sbn_r1cs_free(self.ctx.h, self.h)
            self.h = None


def sparse_eval_sizes(num_vars_x, num_vars_y, num_ops, batch):
    """sbn_sparse_eval_sizes -> (scalars of rnd, bytes of the proof) of sbn_sparse_eval_prove at this shape"""
    a, b = C.c_size_t(0), C.c_size_t(0)
    rc = lib().sbn_sparse_eval_sizes(C.c_size_t(num_vars_x), C.c_size_t(num_vars_y), C.c_size_t(num_ops), C.c_size_t(batch), C.byref(a), C.byref(b))
    if rc:
        raise SbnError(f"sbn_sparse_eval_sizes: ({num_vars_x}, {num_vars_y}, N = {num_ops}, batch = {batch}) is a shape the call refuses (rc={rc})")
    return a.value, b.value


def sparse_eval_kzg_sizes(num_vars_x, num_vars_y, num_ops, batch):
    """sbn_sparse_eval_kzg_sizes -> (scalars of rnd, bytes of the proof) of sbn_sparse_eval_prove_kzg at this shape"""
    a, b = C.c_size_t(0), C.c_size_t(0)
    rc = lib().sbn_sparse_eval_kzg_sizes(C.c_size_t(num_vars_x), C.c_size_t(num_vars_y), C.c_size_t(num_ops), C.c_size_t(batch), C.byref(a), C.byref(b))
    if rc:
        raise SbnError(f"sbn_sparse_eval_kzg_sizes: ({num_vars_x}, {num_vars_y}, N = {num_ops}, batch = {batch}) is a shape the call refuses (rc={rc})")
    return a.value, b.value


class G2Lines:
    """a fixed G2 point made ready for pairings (sbn_g2_prepare): srs.g2 or srs.tau_g2.  Belongs to its Context."""

    def __init__(self, ctx, handle):
        self.ctx, self.h = ctx, handle

    def free(self):
        if self.h:
            lib().sbn_g2_lines_free(self.ctx.h, self.h)
            self.h = None


class DerefsKey:
    """the per-cell SRS sums of one (Dense, SRS) pair (sbn_derefs_key_build).  Free it before the Dense and the SRS."""

    def __init__(self, ctx, handle):
        self.ctx, self.h = ctx, handle

    def __len__(self):
        return lib().sbn_derefs_key_len(self.h)

    def download(self, first=0, count=None):
        """-> ([side << 31 | a], [64-byte canonical affine S[side][a]]) of cells [first, first + count)"""
        count = len(self) - first if count is None else count
        ids = (C.c_uint32 * max(count, 1))(); xy = (C.c_uint8 * (64 * max(count, 1)))()
        self.ctx._chk(lib().sbn_derefs_key_download(self.ctx.h, self.h, C.c_size_t(first), C.c_size_t(count), ids, xy), "sbn_derefs_key_download")
        raw = bytes(xy)
        return [int(ids[j]) for j in range(count)], [raw[64 * j:64 * j + 64] for j in range(count)]

    def free(self):
        if self.h:
            lib().sbn_derefs_key_free(self.ctx.h, self.h)
            self.h = None


class Dense:
    """MultiSparseMatPolynomialAsDense (sparse_mlpoly_full.rs:120-174) resident on the device (sbn_dense_build).  Device pointers are ints;
    comb_ops / comb_mem are Tables that belong to the handle: their free() does nothing, and free() of the handle ends them."""

    def __init__(self, ctx, handle):
        self.ctx, self.h = ctx, handle
        self.num_ops = lib().sbn_dense_num_ops(handle); self.num_cells = lib().sbn_dense_num_cells(handle); self.batch = lib().sbn_dense_batch(handle)
        self.comb_ops = _BorrowedTable(ctx, C.c_void_p(lib().sbn_dense_comb_ops(handle)))
        self.comb_mem = _BorrowedTable(ctx, C.c_void_p(lib().sbn_dense_comb_mem(handle)))

    def addr_dev(self, side, k):
        return lib().sbn_dense_addr_dev(self.h, side, k)

    def read_ts_dev(self, side, k):
        return lib().sbn_dense_read_ts_dev(self.h, side, k)

    def audit_ts_dev(self, side):
        return lib().sbn_dense_audit_ts_dev(self.h, side)

    def ops_slice(self, group, j):
        """polynomial j of group 0..4 (row addr, row read_ts, col addr, col read_ts, val) inside comb_ops, as a view to free before the handle"""
        return self.ctx.table_slice(self.comb_ops, (group * self.batch + j) * self.num_ops, self.num_ops)

    def free(self):
        if self.h:
            self.comb_ops.h = self.comb_mem.h = None
            lib().sbn_dense_free(self.ctx.h, self.h)
            self.h = None


class _BorrowedBases(Bases):
    """a generator set owned by another handle: never passed to sbn_bases_free"""

    def free(self):
        self.h = None


class _BorrowedDense(Dense):
    """the dense representation a SnarkKey owns: never passed to sbn_dense_free"""

    def free(self):
        self.comb_ops.h = self.comb_mem.h = None
        self.h = None


class SnarkGens:
    """SNARKGens (snark.rs:290-328) resident on the device (sbn_snark_gens_new): pc, g3, g4, ops, mem, derefs are Bases that belong to the bundle.
    A bundle from nizk_gens_new (NIZKGens, snark.rs:162-181) holds pc, g3 and g4 alone: ops, mem and derefs are None"""
    KINDS = ("pc", "g3", "g4", "ops", "mem", "derefs")

    def __init__(self, ctx, handle):
        self.ctx, self.h = ctx, handle
        for i, k in enumerate(self.KINDS):
            b = lib().sbn_snark_gens_get(handle, i)
            setattr(self, k, _BorrowedBases(ctx, C.c_void_p(b)) if b else None)

    def free(self):
        if self.h:
            for k in self.KINDS:
                if getattr(self, k) is not None:
                    getattr(self, k).h = None
            lib().sbn_snark_gens_free(self.ctx.h, self.h)
            self.h = None


class SnarkKey:
    """what SNARK::encode returns, resident (sbn_snark_encode), or its verifier's half made of the commitment's bytes (sbn_snark_key_from_comm)"""

    def __init__(self, ctx, handle):
        self.ctx, self.h = ctx, handle
        d = lib().sbn_snark_key_dense(handle)
        self.dense = _BorrowedDense(ctx, C.c_void_p(d)) if d else None

    def comm(self):
        """R1CSCommitment as bytes (include/sbn254.h has the layout)"""
        n = C.c_size_t(0)
        self.ctx._chk(lib().sbn_snark_key_comm(self.h, None, C.c_size_t(0), C.byref(n)), "sbn_snark_key_comm")
        out = (C.c_uint8 * n.value)()
        self.ctx._chk(lib().sbn_snark_key_comm(self.h, out, n, C.byref(n)), "sbn_snark_key_comm")
        return bytes(out)

    def sizes(self, kzg=False):
        """-> (scalars of rnd, bytes of the proof) of snark_prove / snark_prove_kzg"""
        a, b = C.c_size_t(0), C.c_size_t(0)
        self.ctx._chk(lib().sbn_snark_sizes(self.h, int(kzg), C.byref(a), C.byref(b)), "sbn_snark_sizes")
        return a.value, b.value

    def free(self):
        if self.h:
            if self.dense is not None:
                self.dense.free()
            lib().sbn_snark_key_free(self.ctx.h, self.h)
            self.h = None


class _BorrowedR1cs(R1cs):
    """the matrices a NizkInst owns: never passed to sbn_r1cs_free"""

    def free(self):
        self.h = None


class NizkInst:
    """Instance (snark.rs:59-128) for NIZK mode, resident (sbn_nizk_instance_new): the padded matrices and the caller's digest bytes.  r1cs is the
    R1cs that belongs to the handle (what r1cs_evaluate takes)"""

    def __init__(self, ctx, handle, num_cons, num_vars, num_inputs):
        self.ctx, self.h, self.raw = ctx, handle, (num_cons, num_vars, num_inputs)
        npo2 = lambda n: 1 << max(n - 1, 0).bit_length()             # noqa: E731 (snark.rs:74-90)
        self.r1cs = _BorrowedR1cs(ctx, C.c_void_p(lib().sbn_nizk_instance_r1cs(handle)), npo2(max(num_cons, 2)), npo2(max(num_vars, num_inputs + 1)))

    def sizes(self):
        """-> (scalars of rnd, bytes of the proof) of nizk_prove"""
        a, b = C.c_size_t(0), C.c_size_t(0)
        self.ctx._chk(lib().sbn_nizk_sizes(self.h, C.byref(a), C.byref(b)), "sbn_nizk_sizes")
        return a.value, b.value

    def free(self):
        if self.h:
            self.r1cs.free()
            lib().sbn_nizk_instance_free(self.ctx.h, self.h)
            self.h = None


class CircomInfo(C.Structure):
    """sbn_circom_info"""
    _fields_ = [(k, C.c_uint64) for k in ("num_constraints", "num_variables", "num_pub_inputs", "num_prv_inputs", "num_labels")] + \
               [("nnz", C.c_uint64 * 3), ("dropped", C.c_uint64 * 3)] + [(k, C.c_uint64) for k in ("num_vars", "num_cons_padded", "num_vars_padded")]


class CircomR1cs:
    """a circom .r1cs file parsed onto the device (sbn_circom_r1cs_load): per matrix (row, remapped column, canonical value) in file order.  The handles
    made from it (r1cs_from_circom, nizk_instance_from_circom, snark_encode_circom) keep nothing of it"""

    def __init__(self, ctx, handle):
        self.ctx, self.h = ctx, handle

    def info(self):
        """-> dict of sbn_circom_info's fields (nnz and dropped as 3-tuples)"""
        o = CircomInfo()
        self.ctx._chk(lib().sbn_circom_r1cs_info(self.h, C.byref(o)), "sbn_circom_r1cs_info")
        return {k: (tuple(int(x) for x in getattr(o, k)) if k in ("nnz", "dropped") else int(getattr(o, k))) for k, _ in CircomInfo._fields_}

    def download(self, m):
        """matrix m as to_sparse_matrices_padded(num_vars_padded) returns it -> (rows, cols, [32-byte values])"""
        n = self.info()["nnz"][m] if 0 <= m <= 2 else 0
        rows, cols, vals = (C.c_uint32 * max(n, 1))(), (C.c_uint32 * max(n, 1))(), (C.c_uint8 * (32 * max(n, 1)))()
        self.ctx._chk(lib().sbn_circom_r1cs_download(self.ctx.h, self.h, m, rows, cols, vals), "sbn_circom_r1cs_download")
        raw = bytes(vals)
        return [int(rows[i]) for i in range(n)], [int(cols[i]) for i in range(n)], [raw[32 * i:32 * i + 32] for i in range(n)]

    def digest(self):
        """the library's own circuit digest (sbn_circom_r1cs_digest; NOT the reference's get_digest): 32 bytes for nizk_instance_from_circom"""
        out = (C.c_uint8 * 32)()
        self.ctx._chk(lib().sbn_circom_r1cs_digest(self.ctx.h, self.h, out), "sbn_circom_r1cs_digest")
        return bytes(out)

    def free(self):
        if self.h:
            lib().sbn_circom_r1cs_free(self.ctx.h, self.h)
            self.h = None


class GroupBases:
    def __init__(self, group, handle):
        self.group, self.h = group, handle

    def range(self, device):
        lo, hi = C.c_size_t(), C.c_size_t()
        lib().sbn_group_range(self.h, C.c_size_t(device), C.byref(lo), C.byref(hi)); return lo.value, hi.value

    def free(self):
        if self.h:
            lib().sbn_group_bases_free(self.group.h, self.h); self.h = None


class Group:
    """sbn_group_*: one process, several devices behind one call (a device may be listed more than once)"""

    def __init__(self, devices):
        self.h = C.c_void_p()
        arr = (C.c_int * len(devices))(*devices)
        rc = lib().sbn_group_create(arr, C.c_size_t(len(devices)), C.byref(self.h))
        if rc:
            raise SbnError(f"sbn_group_create failed rc={rc}")

    def close(self):
        if self.h:
            lib().sbn_group_destroy(self.h); self.h = None

    def __len__(self):
        return lib().sbn_group_size(self.h)

    def _chk(self, rc, what):
        if rc:
            raise SbnError(f"{what}: rc={rc}: {lib().sbn_group_last_error(self.h).decode()}")

    def ctx(self, i):
        """the i-th device's context as a (non-owning) Context"""
        c = Context.__new__(Context); c.h = C.c_void_p(lib().sbn_group_ctx(self.h, C.c_size_t(i))); c.owned = False
        return c

    def bases_upload(self, G_xy, h_xy=None, flags=0):
        o = C.c_void_p()
        self._chk(lib().sbn_group_bases_upload(self.h, _ptr(G_xy), C.c_size_t(len(G_xy) // 64), _ptr(h_xy), C.c_uint32(flags), C.byref(o)), "sbn_group_bases_upload")
        return GroupBases(self, o)

    def gens_new(self, n, label, want_points=True):
        o = C.c_void_p(); out = (C.c_uint8 * (64 * (n + 1)))() if want_points else None
        self._chk(lib().sbn_group_gens_new(self.h, C.c_size_t(n), _ptr(label), C.c_size_t(len(label)), out, C.byref(o)), "sbn_group_gens_new")
        return GroupBases(self, o), (bytes(out) if want_points else None)

    def bases_precompute(self, gb, max_bytes_per_device):
        cw = C.c_int(0)
        self._chk(lib().sbn_group_bases_precompute(self.h, gb.h, C.c_size_t(max_bytes_per_device), C.byref(cw)), "sbn_group_bases_precompute"); return cw.value

    def commit_rows(self, gb, Z, blinds, L, R, flags=0):
        out = (C.c_uint8 * (64 * L))(); inf = (C.c_uint8 * L)()
        self._chk(lib().sbn_group_commit_rows(self.h, gb.h, _ptr(Z), _ptr(blinds), C.c_size_t(L), C.c_size_t(R), C.c_uint32(flags), out, inf), "sbn_group_commit_rows")
        return bytes(out), bytes(inf)

    def commit_rows_dev(self, gb, z_ptrs, blind_ptrs, L, R, flags=0):
        """z_ptrs[d]: device pointer on device d to its interleaved rows (d, d + N, ...), blind_ptrs likewise or None"""
        N = len(self)
        za = (C.c_void_p * N)(*z_ptrs); ba = (C.c_void_p * N)(*blind_ptrs) if blind_ptrs is not None else None
        out = (C.c_uint8 * (64 * L))(); inf = (C.c_uint8 * L)()
        self._chk(lib().sbn_group_commit_rows_dev(self.h, gb.h, za, ba, C.c_size_t(L), C.c_size_t(R), C.c_uint32(flags), out, inf), "sbn_group_commit_rows_dev")
        return bytes(out), bytes(inf)

    def gather_commit(self, gb, mem, addr_ptrs, n, L, R):
        """mem[d][k]: Table on device d, addr_ptrs[d][k]: device pointer to its n uint32 addresses -> (L x 64 B, L flags)"""
        N = len(self); count = len(mem[0])
        ma = (C.c_void_p * (N * count))(*[t.h for row in mem for t in row])
        aa = (C.c_void_p * (N * count))(*[a for row in addr_ptrs for a in row])
        out = (C.c_uint8 * (64 * L))(); inf = (C.c_uint8 * L)()
        self._chk(lib().sbn_group_gather_commit(self.h, gb.h, ma, aa, C.c_size_t(count), C.c_size_t(n), C.c_size_t(L), C.c_size_t(R), out, inf), "sbn_group_gather_commit")
        return bytes(out), bytes(inf)

    def msm(self, scalars, points, flags=0):
        out = (C.c_uint8 * 64)(); inf = C.c_int()
        self._chk(lib().sbn_group_msm(self.h, _ptr(scalars), _ptr(points), C.c_size_t(len(scalars) // 32), C.c_uint32(flags), out, C.byref(inf)), "sbn_group_msm")
        return bytes(out), bool(inf.value)

    def bases_upload_ranges(self, G_xy, flags=0):
        o = C.c_void_p()
        self._chk(lib().sbn_group_bases_upload_ranges(self.h, _ptr(G_xy), C.c_size_t(len(G_xy) // 64), C.c_uint32(flags), C.byref(o)), "sbn_group_bases_upload_ranges")
        return GroupBases(self, o)

    def bases_synthetic_ranges(self, n, s0, d):
        o = C.c_void_p()
        self._chk(lib().sbn_group_bases_synthetic_ranges(self.h, C.c_size_t(n), _ptr(s0), _ptr(d), C.byref(o)), "sbn_group_bases_synthetic_ranges")
        return GroupBases(self, o)

    def msm_bases(self, gb, scalars, flags=0):
        out = (C.c_uint8 * 64)(); inf = C.c_int()
        self._chk(lib().sbn_group_msm_bases(self.h, gb.h, _ptr(scalars), C.c_size_t(len(scalars) // 32), C.c_uint32(flags), out, C.byref(inf)), "sbn_group_msm_bases")
        return bytes(out), bool(inf.value)

    def msm_bases_dev(self, gb, dev_ptrs, flags=0):
        arr = (C.c_void_p * len(dev_ptrs))(*dev_ptrs); out = (C.c_uint8 * 64)(); inf = C.c_int()
        self._chk(lib().sbn_group_msm_bases_dev(self.h, gb.h, arr, C.c_uint32(flags), out, C.byref(inf)), "sbn_group_msm_bases_dev")
        return bytes(out), bool(inf.value)


class Context:
    owned = True

    def __init__(self, device=0):
        self.h = C.c_void_p()
        rc = lib().sbn_ctx_create(device, C.byref(self.h))
        if rc:
            raise SbnError(f"sbn_ctx_create failed rc={rc} (no gfx950 device? there is no CPU fallback)")

    def close(self):
        if self.h and self.owned:
            lib().sbn_ctx_destroy(self.h)
        self.h = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def _chk(self, rc, what):
        if rc:
            raise SbnError(f"{what}: rc={rc}: {lib().sbn_last_error(self.h).decode()}")

    def set_stream(self, stream_ptr):
        self._chk(lib().sbn_ctx_set_stream(self.h, C.c_void_p(stream_ptr)), "set_stream")

    def sync(self):
        self._chk(lib().sbn_ctx_sync(self.h), "sync")

    # ---- B1
    def msm(self, scalars, points, flags=0):
        n = len(scalars) // 32
        assert len(points) == 64 * n
        out = (C.c_uint8 * 64)(); inf = C.c_int()
        self._chk(lib().sbn_msm(self.h, _ptr(scalars), _ptr(points), C.c_size_t(n), C.c_uint32(flags), out, C.byref(inf)), "sbn_msm")
        return bytes(out), bool(inf.value)

    def msm_jacobian(self, scalars, points_xyz, flags=0):
        n = len(scalars) // 32
        assert len(points_xyz) == 96 * n
        out = (C.c_uint8 * 64)(); inf = C.c_int()
        self._chk(lib().sbn_msm_jacobian(self.h, _ptr(scalars), _ptr(points_xyz), C.c_size_t(n), C.c_uint32(flags), out, C.byref(inf)), "sbn_msm_jacobian")
        return bytes(out), bool(inf.value)

    def bases_precompute(self, bases, max_bytes):
        """build the fixed-base lookup table within max_bytes of HBM; returns the window bits chosen"""
        cw = C.c_int(0)
        self._chk(lib().sbn_bases_precompute(self.h, bases.h, C.c_size_t(max_bytes), C.byref(cw)), "sbn_bases_precompute")
        return cw.value

    def bases_split_at(self, bases, mid):
        l, r = C.c_void_p(), C.c_void_p()
        self._chk(lib().sbn_bases_split_at(self.h, bases.h, C.c_size_t(mid), C.byref(l), C.byref(r)), "sbn_bases_split_at")
        return Bases(self, l), Bases(self, r)

    def bases_scale(self, bases, s):
        o = C.c_void_p()
        self._chk(lib().sbn_bases_scale(self.h, bases.h, _ptr(s), C.byref(o)), "sbn_bases_scale")
        return Bases(self, o)

    def bases_upload(self, G_xy, h_xy=None, flags=0):
        n = len(G_xy) // 64
        hb = C.c_void_p()
        self._chk(lib().sbn_bases_upload(self.h, _ptr(G_xy), C.c_size_t(n), _ptr(h_xy), C.c_uint32(flags), C.byref(hb)), "sbn_bases_upload")
        return Bases(self, hb)

    def gens_new(self, n, label, want_points=True):
        hb = C.c_void_p()
        out = (C.c_uint8 * (64 * (n + 1)))() if want_points else None
        self._chk(lib().sbn_gens_new(self.h, C.c_size_t(n), _ptr(label), C.c_size_t(len(label)), out, C.byref(hb)), "sbn_gens_new")
        return Bases(self, hb), (bytes(out) if want_points else None)

    def bases_synthetic(self, n, first, s0, d):
        hb = C.c_void_p()
        self._chk(lib().sbn_bases_synthetic(self.h, C.c_size_t(n), C.c_uint64(first), _ptr(s0), _ptr(d), C.byref(hb)), "sbn_bases_synthetic")
        return Bases(self, hb)

    def scalars_synthetic(self, seed, first, n, out_dev_ptr):
        self._chk(lib().sbn_scalars_synthetic(self.h, C.c_uint64(seed), C.c_uint64(first), C.c_size_t(n), C.c_void_p(out_dev_ptr)), "sbn_scalars_synthetic")

    def bases_download(self, bases, first, count):
        out = (C.c_uint8 * (64 * count))()
        self._chk(lib().sbn_bases_download(self.h, bases.h, C.c_size_t(first), C.c_size_t(count), out), "sbn_bases_download")
        return bytes(out)

    def msm_bases(self, bases, scalars, flags=0):
        n = len(scalars) // 32
        out = (C.c_uint8 * 64)(); inf = C.c_int()
        self._chk(lib().sbn_msm_bases(self.h, bases.h, _ptr(scalars), C.c_size_t(n), C.c_uint32(flags), out, C.byref(inf)), "sbn_msm_bases")
        return bytes(out), bool(inf.value)

    def msm_bases_dev(self, bases, scalars_dev_ptr, n, flags=0):
        out = (C.c_uint8 * 64)(); inf = C.c_int()
        self._chk(lib().sbn_msm_bases_dev(self.h, bases.h, C.c_void_p(scalars_dev_ptr), C.c_size_t(n), C.c_uint32(flags), out, C.byref(inf)), "sbn_msm_bases_dev")
        return bytes(out), bool(inf.value)

    # ---- B2
    def commit_rows(self, bases, Z, blinds, L, R, flags=0):
        out = (C.c_uint8 * (64 * L))(); inf = (C.c_uint8 * L)()
        self._chk(lib().sbn_commit_rows(self.h, bases.h, _ptr(Z), _ptr(blinds), C.c_size_t(L), C.c_size_t(R), C.c_uint32(flags), out, inf), "sbn_commit_rows")
        return bytes(out), bytes(inf)

    def commit_rows_dev(self, bases, Z_dev_ptr, blinds_dev_ptr, L, R, flags=0):
        out = (C.c_uint8 * (64 * L))(); inf = (C.c_uint8 * L)()
        self._chk(lib().sbn_commit_rows_dev(self.h, bases.h, C.c_void_p(Z_dev_ptr), C.c_void_p(blinds_dev_ptr or 0), C.c_size_t(L), C.c_size_t(R), C.c_uint32(flags), out, inf), "sbn_commit_rows_dev")
        return bytes(out), bytes(inf)

    # ---- raw device memory
    def dev_alloc(self, nbytes):
        p = C.c_void_p(); self._chk(lib().sbn_dev_alloc(self.h, C.c_size_t(nbytes), C.byref(p)), "sbn_dev_alloc"); return p.value

    def dev_free(self, p):
        self._chk(lib().sbn_dev_free(self.h, C.c_void_p(p)), "sbn_dev_free")

    def dev_upload(self, dst, data):
        self._chk(lib().sbn_dev_upload(self.h, C.c_void_p(dst), _ptr(data), C.c_size_t(len(data) if not hasattr(data, "nbytes") else data.nbytes)), "sbn_dev_upload")

    def dev_download(self, src, nbytes):
        out = (C.c_uint8 * nbytes)(); self._chk(lib().sbn_dev_download(self.h, out, C.c_void_p(src), C.c_size_t(nbytes)), "sbn_dev_download"); return bytes(out)

    # ---- B3
    def table_upload(self, Z, flags=0):
        n = len(Z) // 32; ht = C.c_void_p()
        self._chk(lib().sbn_table_upload(self.h, _ptr(Z), C.c_size_t(n), C.c_uint32(flags), C.byref(ht)), "sbn_table_upload")
        return Table(self, ht)

    def table_from_dev(self, dev_ptr, n, flags=0):
        ht = C.c_void_p()
        self._chk(lib().sbn_table_from_dev(self.h, C.c_void_p(dev_ptr), C.c_size_t(n), C.c_uint32(flags), C.byref(ht)), "sbn_table_from_dev")
        return Table(self, ht)

    def table_download(self, t):
        n = len(t); out = (C.c_uint8 * (32 * n))()
        self._chk(lib().sbn_table_download(self.h, t.h, out), "sbn_table_download"); return bytes(out)

    def table_read0(self, t):
        out = (C.c_uint8 * 32)(); self._chk(lib().sbn_table_read0(self.h, t.h, out), "sbn_table_read0"); return bytes(out)

    def table_read0_many(self, ts):
        """entry 0 of every table in `ts`: one launch, one wait (sbn_table_read0_many)"""
        n = len(ts)
        arr = (C.c_void_p * max(n, 1))(*[t.h for t in ts]); out = (C.c_uint8 * (32 * max(n, 1)))()
        self._chk(lib().sbn_table_read0_many(self.h, arr, C.c_size_t(n), out), "sbn_table_read0_many")
        return [bytes(out[32 * i:32 * i + 32]) for i in range(n)]

    def bind_top(self, t, r):
        self._chk(lib().sbn_bind_top(self.h, t.h, _ptr(r)), "sbn_bind_top")

    def bind_top_many(self, ts, r):
        arr = (C.c_void_p * len(ts))(*[t.h for t in ts])
        self._chk(lib().sbn_bind_top_many(self.h, arr, C.c_size_t(len(ts)), _ptr(r)), "sbn_bind_top_many")

    def sc_eval_cubic(self, A, B, Cc):
        out = (C.c_uint8 * 96)(); self._chk(lib().sbn_sc_eval_cubic(self.h, A.h, B.h, Cc.h, out), "sbn_sc_eval_cubic"); return bytes(out)

    def sc_eval_cubic_batched(self, As, Bs, Cs):
        k = len(As); mk = lambda ts: (C.c_void_p * k)(*[t.h for t in ts])
        out = (C.c_uint8 * (96 * k))()
        self._chk(lib().sbn_sc_eval_cubic_batched(self.h, mk(As), mk(Bs), mk(Cs), C.c_size_t(k), out), "sbn_sc_eval_cubic_batched"); return bytes(out)

    def sc_eval_r1cs(self, T, A, B, Cc):
        out = (C.c_uint8 * 96)(); self._chk(lib().sbn_sc_eval_r1cs(self.h, T.h, A.h, B.h, Cc.h, out), "sbn_sc_eval_r1cs"); return bytes(out)

    def sc_eval_quad(self, Z, ABC):
        out = (C.c_uint8 * 64)(); self._chk(lib().sbn_sc_eval_quad(self.h, Z.h, ABC.h, out), "sbn_sc_eval_quad"); return bytes(out)

    def sc_bind_eval_cubic_batched(self, As, Bs, Cs, r):
        k = len(As); mk = lambda ts: (C.c_void_p * k)(*[t.h for t in ts])
        out = (C.c_uint8 * (96 * k))()
        self._chk(lib().sbn_sc_bind_eval_cubic_batched(self.h, mk(As), mk(Bs), mk(Cs), C.c_size_t(k), _ptr(r), out), "sbn_sc_bind_eval_cubic_batched"); return bytes(out)

    def sc_bind_eval_r1cs(self, T, A, B, Cc, r):
        out = (C.c_uint8 * 96)(); self._chk(lib().sbn_sc_bind_eval_r1cs(self.h, T.h, A.h, B.h, Cc.h, _ptr(r), out), "sbn_sc_bind_eval_r1cs"); return bytes(out)

    def sc_bind_eval_quad(self, Z, ABC, r):
        out = (C.c_uint8 * 64)(); self._chk(lib().sbn_sc_bind_eval_quad(self.h, Z.h, ABC.h, _ptr(r), out), "sbn_sc_bind_eval_quad"); return bytes(out)

    def sumcheck_begin(self, A_par, B_par, C_par, A_seq, B_seq, C_seq, coeffs):
        """-> (Sumcheck state, the combined (e0, e2, e3) of round 0)"""
        mk = lambda ts: (C.c_void_p * max(1, len(ts)))(*[t.h for t in ts])
        st = C.c_void_p(); out = (C.c_uint8 * 96)()
        self._chk(lib().sbn_sumcheck_begin(self.h, mk(A_par), mk(B_par), C_par.h if C_par is not None else None, C.c_size_t(len(A_par)),
                                           mk(A_seq), mk(B_seq), mk(C_seq), C.c_size_t(len(A_seq)), _ptr(coeffs), out, C.byref(st)), "sbn_sumcheck_begin")
        return Sumcheck(self, st, len(A_par), len(A_seq)), bytes(out)

    def sumcheck_begin_eq(self, A_par, B_par, rand, A_seq, B_seq, C_seq, coeffs):
        """poly_C_par = eq(rand) built inside the call -> (Sumcheck state, the combined (e0, e2, e3) of round 0)"""
        mk = lambda ts: (C.c_void_p * max(1, len(ts)))(*[t.h for t in ts])
        st = C.c_void_p(); out = (C.c_uint8 * 96)()
        self._chk(lib().sbn_sumcheck_begin_eq(self.h, mk(A_par), mk(B_par), C.c_size_t(len(A_par)), _ptr(rand), C.c_size_t(len(rand) // 32),
                                              mk(A_seq), mk(B_seq), mk(C_seq), C.c_size_t(len(A_seq)), _ptr(coeffs), out, C.byref(st)), "sbn_sumcheck_begin_eq")
        return Sumcheck(self, st, len(A_par), len(A_seq)), bytes(out)

    def sumcheck_prove(self, st, tr, claim):
        """the whole sumcheck in one call (sbn_sumcheck_prove): -> (polys: rounds x [c0..c3], challenges: rounds x 32 B, finals); `tr` (Transcript) moves on"""
        n = len(st)
        rounds = n.bit_length() - 1
        polys = (C.c_uint8 * (128 * max(rounds, 1)))(); rs = (C.c_uint8 * (32 * max(rounds, 1)))(); fin = (C.c_uint8 * (32 * st.ntab))()
        self._chk(lib().sbn_sumcheck_prove(self.h, st.h, tr.h, _ptr(claim), polys, rs, fin), "sbn_sumcheck_prove")
        pb, rb = bytes(polys), bytes(rs)
        return ([[pb[128 * j + 32 * k:128 * j + 32 * k + 32] for k in range(4)] for j in range(rounds)], [rb[32 * j:32 * j + 32] for j in range(rounds)],
                [bytes(fin[32 * t:32 * t + 32]) for t in range(st.ntab)])

    def product_proof_prove(self, layers, dotps, tr):
        """ProductCircuitEvalProofBatched::prove in one call (sbn_product_proof_prove).  layers[i][j]: circuit i's layer j (Table, left || right, the input
        first: what product_circuit{,_many} return behind their input); dotps: [(left, right, weight)] Tables; `tr` (Transcript) moves on.
        -> (out_polys, out_claims, out_rand, out_claims_final) as bytes, laid out as include/sbn254.h describes"""
        n, L, nd = len(layers), len(layers[0]), len(dotps)
        arr = (C.c_void_p * (n * L))(*[layers[i][j].h for i in range(n) for j in range(L)])
        mk = lambda k: (C.c_void_p * max(1, nd))(*[d[k].h for d in dotps])
        polys = (C.c_uint8 * (128 * max(1, L * (L - 1) // 2)))(); claims = (C.c_uint8 * (32 * (2 * n * L + 3 * nd)))()
        rand = (C.c_uint8 * (32 * L))(); fin = (C.c_uint8 * (32 * n))()
        self._chk(lib().sbn_product_proof_prove(self.h, arr, C.c_size_t(n), C.c_size_t(L), mk(0), mk(1), mk(2), C.c_size_t(nd), tr.h, polys, claims, rand, fin),
                  "sbn_product_proof_prove")
        return bytes(polys)[:128 * (L * (L - 1) // 2)], bytes(claims), bytes(rand), bytes(fin)

    def eq_evals(self, r):
        ell = len(r) // 32; ht = C.c_void_p()
        self._chk(lib().sbn_eq_evals(self.h, _ptr(r), C.c_size_t(ell), C.byref(ht)), "sbn_eq_evals"); return Table(self, ht)

    def hash_layer(self, addr_dev_ptr, val, ts_dev_ptr, ts_add, r_hash, r_multiset):
        ht = C.c_void_p()
        self._chk(lib().sbn_hash_layer(self.h, C.c_void_p(addr_dev_ptr or 0), val.h, C.c_void_p(ts_dev_ptr or 0), C.c_uint32(ts_add), _ptr(r_hash), _ptr(r_multiset), C.byref(ht)), "sbn_hash_layer")
        return Table(self, ht)

    def hash_layer_pair(self, addr_dev_ptr, val, ts_a_ptr, ts_a_add, ts_b_ptr, ts_b_add, r_hash, r_multiset):
        ha, hb = C.c_void_p(), C.c_void_p()
        self._chk(lib().sbn_hash_layer_pair(self.h, C.c_void_p(addr_dev_ptr or 0), val.h, C.c_void_p(ts_a_ptr or 0), C.c_uint32(ts_a_add), C.c_void_p(ts_b_ptr or 0), C.c_uint32(ts_b_add),
                                            _ptr(r_hash), _ptr(r_multiset), C.byref(ha), C.byref(hb)), "sbn_hash_layer_pair")
        return Table(self, ha), Table(self, hb)

    def hash_layer_pair_product(self, addr_dev_ptr, val, ts_a_ptr, ts_a_add, ts_b_ptr, ts_b_add, r_hash, r_multiset):
        """hash_layer_pair and the first product layer of both sets in one pass -> (out_a, out_b, prod_a, prod_b)"""
        hs = [C.c_void_p() for _ in range(4)]
        self._chk(lib().sbn_hash_layer_pair_product(self.h, C.c_void_p(addr_dev_ptr or 0), val.h, C.c_void_p(ts_a_ptr or 0), C.c_uint32(ts_a_add), C.c_void_p(ts_b_ptr or 0),
                                                    C.c_uint32(ts_b_add), _ptr(r_hash), _ptr(r_multiset), *[C.byref(h) for h in hs]), "sbn_hash_layer_pair_product")
        return tuple(Table(self, h) for h in hs)

    def product_layer(self, t):
        ht = C.c_void_p(); self._chk(lib().sbn_product_layer(self.h, t.h, C.byref(ht)), "sbn_product_layer"); return Table(self, ht)

    def product_circuit(self, t):
        """all layers above t (ProductCircuit::new): list of Tables of len/2, len/4, ..., 1 entries"""
        cap = max(1, len(t).bit_length())
        arr = (C.c_void_p * cap)(); cnt = C.c_size_t(0)
        self._chk(lib().sbn_product_circuit(self.h, t.h, arr, C.c_size_t(cap), C.byref(cnt)), "sbn_product_circuit")
        return [Table(self, C.c_void_p(arr[i])) for i in range(cnt.value)]

    def product_circuit_many(self, ts):
        """the circuits of several tables of one length, one launch per layer for all -> [[layers of ts[0]], [layers of ts[1]], ...]"""
        n = len(ts); cap = max(1, len(ts[0]).bit_length())
        ins = (C.c_void_p * n)(*[t.h for t in ts]); arr = (C.c_void_p * (n * cap))(); cnt = C.c_size_t(0)
        self._chk(lib().sbn_product_circuit_many(self.h, ins, C.c_size_t(n), arr, C.c_size_t(cap), C.byref(cnt)), "sbn_product_circuit_many")
        return [[Table(self, C.c_void_p(arr[i * cap + k])) for k in range(cnt.value)] for i in range(n)]

    def table_halves(self, t):
        l, r = C.c_void_p(), C.c_void_p()
        self._chk(lib().sbn_table_halves(self.h, t.h, C.byref(l), C.byref(r)), "sbn_table_halves"); return Table(self, l), Table(self, r)

    def table_dot(self, a, b):
        out = (C.c_uint8 * 32)(); self._chk(lib().sbn_table_dot(self.h, a.h, b.h, out), "sbn_table_dot"); return bytes(out)

    def table_evaluate(self, Z, r):
        out = (C.c_uint8 * 32)(); self._chk(lib().sbn_table_evaluate(self.h, Z.h, _ptr(r), C.c_size_t(len(r) // 32), out), "sbn_table_evaluate"); return bytes(out)

    def table_evaluate_many(self, Zs, r):
        k = len(Zs); arr = (C.c_void_p * k)(*[t.h for t in Zs]); out = (C.c_uint8 * (32 * k))()
        self._chk(lib().sbn_table_evaluate_many(self.h, arr, C.c_size_t(k), _ptr(r), C.c_size_t(len(r) // 32), out), "sbn_table_evaluate_many")
        return bytes(out)

    def table_bound(self, Z, Lvec):
        ht = C.c_void_p(); self._chk(lib().sbn_table_bound(self.h, Z.h, Lvec.h, C.byref(ht)), "sbn_table_bound"); return Table(self, ht)

    def table_slice(self, t, first, length):
        ht = C.c_void_p()
        self._chk(lib().sbn_table_slice(self.h, t.h, C.c_size_t(first), C.c_size_t(length), C.byref(ht)), "sbn_table_slice")
        return Table(self, ht)

    def gather_merge(self, mems, addr_dev_ptrs, n):
        k = len(mems)
        ma = (C.c_void_p * k)(*[t.h for t in mems]); aa = (C.c_void_p * k)(*addr_dev_ptrs)
        ht = C.c_void_p()
        self._chk(lib().sbn_gather_merge(self.h, ma, aa, C.c_size_t(k), C.c_size_t(n), C.byref(ht)), "sbn_gather_merge")
        return Table(self, ht)

    def gather_merge_rows(self, mems, addr_dev_ptrs, n, R, row0, rstep, nrows):
        k = len(mems)
        ma = (C.c_void_p * k)(*[t.h for t in mems]); aa = (C.c_void_p * k)(*addr_dev_ptrs)
        ht = C.c_void_p()
        self._chk(lib().sbn_gather_merge_rows(self.h, ma, aa, C.c_size_t(k), C.c_size_t(n), C.c_size_t(R), C.c_size_t(row0), C.c_size_t(rstep), C.c_size_t(nrows), C.byref(ht)), "sbn_gather_merge_rows")
        return Table(self, ht)

    def commit_table(self, bases, t, blinds, L, R):
        out = (C.c_uint8 * (64 * L))(); inf = (C.c_uint8 * L)()
        self._chk(lib().sbn_commit_table(self.h, bases.h, t.h, _ptr(blinds), C.c_size_t(L), C.c_size_t(R), out, inf), "sbn_commit_table")
        return bytes(out), bytes(inf)

    # ---- BulletReductionProof::prove (nizk/bullet.rs:41-126) as a device-resident state
    def bullet_begin(self, G, Q_xy, a, b, blind=None, want_gamma=True):
        """-> (Bullet state, Gamma_xy or None)"""
        st = C.c_void_p(); gm = (C.c_uint8 * 64)() if want_gamma else None; gi = C.c_int(0)
        self._chk(lib().sbn_bullet_begin(self.h, G.h, _ptr(Q_xy), a.h, b.h, _ptr(blind), gm, C.byref(gi), C.byref(st)), "sbn_bullet_begin")
        return Bullet(self, st), (bytes(gm) if want_gamma else None)

    def bullet_begin_scaled(self, G, Q_base_xy, q_scale, a, b, blind=None, want_gamma=True):
        """Q = q_scale * Q_base -> (Bullet state, Gamma_xy or None)"""
        st = C.c_void_p(); gm = (C.c_uint8 * 64)() if want_gamma else None; gi = C.c_int(0)
        self._chk(lib().sbn_bullet_begin_scaled(self.h, G.h, _ptr(Q_base_xy), _ptr(q_scale), a.h, b.h, _ptr(blind), gm, C.byref(gi), C.byref(st)), "sbn_bullet_begin_scaled")
        return Bullet(self, st), (bytes(gm) if want_gamma else None)

    def bullet_cross(self, st, blind_L=None, blind_R=None):
        """-> (L_xy, L_inf, R_xy, R_inf, c_L, c_R)"""
        Lo, Ro = (C.c_uint8 * 64)(), (C.c_uint8 * 64)(); li, ri = C.c_int(0), C.c_int(0)
        cl, cr = (C.c_uint8 * 32)(), (C.c_uint8 * 32)()
        self._chk(lib().sbn_bullet_cross(self.h, st.h, _ptr(blind_L), _ptr(blind_R), Lo, C.byref(li), Ro, C.byref(ri), cl, cr), "sbn_bullet_cross")
        return bytes(Lo), bool(li.value), bytes(Ro), bool(ri.value), bytes(cl), bytes(cr)

    def bullet_fold_cross(self, st, u, u_inv, blind_L=None, blind_R=None):
        """fold with u, then the next round's cross terms -> (L_xy, L_inf, R_xy, R_inf, c_L, c_R)"""
        Lo, Ro = (C.c_uint8 * 64)(), (C.c_uint8 * 64)(); li, ri = C.c_int(0), C.c_int(0)
        cl, cr = (C.c_uint8 * 32)(), (C.c_uint8 * 32)()
        self._chk(lib().sbn_bullet_fold_cross(self.h, st.h, _ptr(u), _ptr(u_inv), _ptr(blind_L), _ptr(blind_R), Lo, C.byref(li), Ro, C.byref(ri), cl, cr), "sbn_bullet_fold_cross")
        return bytes(Lo), bool(li.value), bytes(Ro), bool(ri.value), bytes(cl), bytes(cr)

    def bullet_fold(self, st, u, u_inv):
        self._chk(lib().sbn_bullet_fold(self.h, st.h, _ptr(u), _ptr(u_inv)), "sbn_bullet_fold")

    def bullet_finish(self, st):
        """-> (a_hat, b_hat, g_hat_xy)"""
        ah, bh, gh = (C.c_uint8 * 32)(), (C.c_uint8 * 32)(), (C.c_uint8 * 64)(); gi = C.c_int(0)
        self._chk(lib().sbn_bullet_finish(self.h, st.h, ah, bh, gh, C.byref(gi)), "sbn_bullet_finish")
        return bytes(ah), bytes(bh), bytes(gh)

    # ---- the Hyrax opening in one call (hyrax.rs:65-116, nizk/mod.rs:439-522, nizk/bullet.rs:24-126)
    def polyeval_prove(self, gens, Z, r, Zr, rnd, tr, blinds=None, blind_Zr=None):
        """PolyEvalProof::prove (sbn_polyeval_prove) -> (proof bytes, Cx_xy, Cy_xy); gens: R_size + 1 generators with h; `tr` (Transcript) moves on"""
        ell = len(r) // 32
        lg = ell - ell // 2
        proof = (C.c_uint8 * (64 * lg + 128))(); cx, cy = (C.c_uint8 * 64)(), (C.c_uint8 * 64)(); xi, yi = C.c_int(0), C.c_int(0)
        self._chk(lib().sbn_polyeval_prove(self.h, gens.h, Z.h, _ptr(blinds), _ptr(r), C.c_size_t(ell), _ptr(Zr), _ptr(blind_Zr), _ptr(rnd), tr.h,
                                           proof, cx, C.byref(xi), cy, C.byref(yi)), "sbn_polyeval_prove")
        return bytes(proof), bytes(cx), bytes(cy)

    def joint_opening_prove(self, gens, Z, evals, labels, r, rnd, tr):
        """the n-to-1 reduction + opening of sparse_mlpoly_full.rs:384-407 (sbn_joint_opening_prove); labels = (evals, challenge, claim)
        -> (challenges, joint_claim, proof bytes, Cx_xy, Cy_xy)"""
        count = len(evals) // 32
        lc = count.bit_length() - 1
        ell = lc + len(r) // 32
        lg = ell - ell // 2
        ch = (C.c_uint8 * max(32 * lc, 1))(); claim = (C.c_uint8 * 32)()
        proof = (C.c_uint8 * (64 * lg + 128))(); cx, cy = (C.c_uint8 * 64)(), (C.c_uint8 * 64)(); xi, yi = C.c_int(0), C.c_int(0)
        le, lch, lcl = labels
        self._chk(lib().sbn_joint_opening_prove(self.h, gens.h, Z.h, _ptr(evals), C.c_size_t(count), _ptr(le), C.c_size_t(len(le)), _ptr(lch), C.c_size_t(len(lch)),
                                                _ptr(lcl), C.c_size_t(len(lcl)), _ptr(r), C.c_size_t(len(r) // 32), _ptr(rnd), tr.h, ch, claim, proof,
                                                cx, C.byref(xi), cy, C.byref(yi)), "sbn_joint_opening_prove")
        return bytes(ch[:32 * lc]), bytes(claim), bytes(proof), bytes(cx), bytes(cy)

    # ---- the Hyrax opening check in one call (hyrax.rs:118-151, nizk/mod.rs:525-567, nizk/bullet.rs:130-173)
    def g1_decompress(self, comp32):
        """deserialize_compressed of n points on the device (sbn_g1_decompress) -> (n x 64 canonical affine bytes, n flags: 0 = does not decompress)"""
        n = len(comp32) // 32
        xy, ok = (C.c_uint8 * max(64 * n, 1))(), (C.c_uint8 * max(n, 1))()
        self._chk(lib().sbn_g1_decompress(self.h, _ptr(comp32), C.c_size_t(n), xy, ok), "sbn_g1_decompress")
        return bytes(xy[:64 * n]), bytes(ok[:n])

    def bases_from_compressed(self, comp32):
        """a resident point set (no h) from compressed bytes (sbn_bases_from_compressed); a point that does not decompress raises SbnError
        with its index in `.bad_index`"""
        n = len(comp32) // 32
        hb = C.c_void_p(); bad = C.c_size_t(n)
        rc = lib().sbn_bases_from_compressed(self.h, _ptr(comp32), C.c_size_t(n), C.byref(hb), C.byref(bad))
        if rc:
            err = SbnError(f"sbn_bases_from_compressed: rc={rc}: {lib().sbn_last_error(self.h).decode()}")
            err.bad_index = bad.value if bad.value < n else None
            raise err
        return Bases(self, hb)

    def polyeval_verify(self, gens, comm, r, proof, tr, C_Zr_xy=None, Zr=None):
        """PolyEvalProof::verify (C_Zr_xy) / verify_plain (Zr) in one call (sbn_polyeval_verify) -> accepted; comm: the L_size row commitments as a
        Bases without h; `tr` moves on only when the proof is accepted.  Misuse raises SbnError"""
        acc = C.c_int(0)
        self._chk(lib().sbn_polyeval_verify(self.h, gens.h, comm.h, _ptr(r), C.c_size_t(len(r) // 32), _ptr(C_Zr_xy), _ptr(Zr), _ptr(proof), tr.h, C.byref(acc)),
                  "sbn_polyeval_verify")
        return bool(acc.value)

    def joint_opening_verify(self, gens, comm, evals, labels, r, proof, tr):
        """the n-to-1 reduction + verify_plain of sparse_mlpoly_full.rs:434-457 (sbn_joint_opening_verify); labels = (evals, challenge, claim)
        -> (accepted, challenges)"""
        count = len(evals) // 32
        lc = count.bit_length() - 1
        ch = (C.c_uint8 * max(32 * lc, 1))(); acc = C.c_int(0)
        le, lch, lcl = labels
        self._chk(lib().sbn_joint_opening_verify(self.h, gens.h, comm.h, _ptr(evals), C.c_size_t(count), _ptr(le), C.c_size_t(len(le)), _ptr(lch), C.c_size_t(len(lch)),
                                                 _ptr(lcl), C.c_size_t(len(lcl)), _ptr(r), C.c_size_t(len(r) // 32), _ptr(proof), tr.h, ch, C.byref(acc)),
                  "sbn_joint_opening_verify")
        return bool(acc.value), bytes(ch[:32 * lc])

    def prof_last_polyeval(self):
        """host microseconds of the most recent opening: (R on the host, wait for the first commit, Cx + Cy + a_vec absorbed)"""
        out = (C.c_double * 3)()
        self._chk(lib().sbn_prof_last_polyeval(self.h, out), "sbn_prof_last_polyeval")
        return tuple(out)

    # ---- the two ZK sumchecks of R1CSProof::prove in one call each (sumcheck.rs:465-811, nizk/mod.rs:306-366)
    def _zk_sumcheck_prove(self, fn, name, tables, n, gens_1, gens_n, claim, blind_claim, rnd, tr):
        rounds = max(len(tables[0]).bit_length() - 1, 0)
        proof = (C.c_uint8 * max((6 + n) * 32 * rounds, 1))(); rs = (C.c_uint8 * max(32 * rounds, 1))()
        fin = (C.c_uint8 * (32 * len(tables)))(); bl = (C.c_uint8 * 32)()
        self._chk(fn(self.h, *[t.h for t in tables], gens_1.h, gens_n.h, _ptr(claim), _ptr(blind_claim), _ptr(rnd), tr.h, proof, rs, fin, bl), name)
        return bytes(proof[:(6 + n) * 32 * rounds]), bytes(rs[:32 * rounds]), bytes(fin), bytes(bl)

    def zk_sumcheck_prove_r1cs(self, tau, Az, Bz, Cz, gens_1, gens_4, claim, blind_claim, rnd, tr):
        """prove_cubic_with_additive_term (sbn_zk_sumcheck_prove_r1cs) -> (proof: rounds x 10 x 32, challenges, finals [tau, Az, Bz, Cz], blinds_evals[-1]);
        the tables are bound in place down to length 1; rnd: rounds x 8 scalars; `tr` (Transcript) moves on"""
        return self._zk_sumcheck_prove(lib().sbn_zk_sumcheck_prove_r1cs, "sbn_zk_sumcheck_prove_r1cs", (tau, Az, Bz, Cz), 4, gens_1, gens_4, claim, blind_claim, rnd, tr)

    def zk_sumcheck_prove_quad(self, Z, ABC, gens_1, gens_3, claim, blind_claim, rnd, tr):
        """prove_quad (sbn_zk_sumcheck_prove_quad) -> (proof: rounds x 9 x 32, challenges, finals [Z, ABC], blinds_evals[-1]); rnd: rounds x 7 scalars"""
        return self._zk_sumcheck_prove(lib().sbn_zk_sumcheck_prove_quad, "sbn_zk_sumcheck_prove_quad", (Z, ABC), 3, gens_1, gens_3, claim, blind_claim, rnd, tr)

    # ---- R1CSProof::prove in one call (r1csproof.rs:241-459)
    def r1cs_proof_prove(self, inst, vars, inputs, gens_pc, gens_3, gens_4, rnd, tr):
        """R1CSProof::prove (sbn_r1cs_proof_prove) -> (proof bytes, rx, ry); vars: a Table of num_vars entries (only read); inputs: canonical
        scalars, 32 bytes each (b"" for none); gens_pc: R + 1 generators with h; rnd: r1cs_proof_sizes(...)[0] scalars; `tr` (Transcript) moves on"""
        n_rnd, n_proof = r1cs_proof_sizes(inst.num_cons, inst.num_vars)
        if len(rnd) != 32 * n_rnd:
            raise ValueError(f"r1cs_proof_prove: rnd holds {len(rnd)} bytes, the shape needs {32 * n_rnd}")
        nx, ny = inst.num_cons.bit_length() - 1, inst.num_vars.bit_length()
        proof = (C.c_uint8 * n_proof)(); rx = (C.c_uint8 * (32 * nx))(); ry = (C.c_uint8 * (32 * ny))()
        self._chk(lib().sbn_r1cs_proof_prove(self.h, inst.h, vars.h, _ptr(inputs) if inputs else None, C.c_size_t(len(inputs) // 32 if inputs else 0),
                                             gens_pc.h, gens_3.h, gens_4.h, _ptr(rnd), tr.h, proof, rx, ry), "sbn_r1cs_proof_prove")
        return bytes(proof), bytes(rx), bytes(ry)

    # ---- R1CSProof::verify and ZKSumcheckInstanceProof::verify in one call each (r1csproof.rs:463-619, sumcheck.rs:366-457)
    def zk_sumcheck_verify(self, gens_1, gens_n, comm_claim_xy, num_rounds, degree_bound, proof, tr):
        """ZKSumcheckInstanceProof::verify (sbn_zk_sumcheck_verify) -> (comm_evals[-1] as 64 canonical affine bytes, challenges), or None when the
        proof is refused; proof: the out_proof of zk_sumcheck_prove_r1cs (degree_bound 3) / _quad (2); `tr` moves on only when the proof is accepted.
        Misuse raises SbnError"""
        n = degree_bound + 1
        if len(proof) != (6 + n) * 32 * num_rounds:
            raise ValueError(f"zk_sumcheck_verify: the proof holds {len(proof)} bytes, {num_rounds} rounds of degree {degree_bound} need {(6 + n) * 32 * num_rounds}")
        rs = (C.c_uint8 * max(32 * num_rounds, 1))(); xy = (C.c_uint8 * 64)(); acc = C.c_int(0)
        self._chk(lib().sbn_zk_sumcheck_verify(self.h, gens_1.h, gens_n.h, _ptr(comm_claim_xy), C.c_size_t(num_rounds), C.c_size_t(degree_bound), _ptr(proof), tr.h,
                                               rs, xy, C.byref(acc)), "sbn_zk_sumcheck_verify")
        return (bytes(xy), bytes(rs[:32 * num_rounds])) if acc.value else None

    def r1cs_proof_verify(self, num_cons, num_vars, inputs, evals, gens_pc, gens_3, gens_4, proof, tr):
        """R1CSProof::verify (sbn_r1cs_proof_verify) -> (rx, ry), or None when the proof is refused; inputs: canonical scalars, 32 bytes each (b"" for
        none); evals: A, B, C(rx, ry), 96 bytes; proof: the out_proof of r1cs_proof_prove; `tr` moves on only when the proof is accepted.  Misuse raises
        SbnError"""
        n_proof = r1cs_proof_sizes(num_cons, num_vars)[1]
        if len(proof) != n_proof:
            raise ValueError(f"r1cs_proof_verify: the proof holds {len(proof)} bytes, the shape needs {n_proof}")
        if len(evals) != 96:
            raise ValueError(f"r1cs_proof_verify: evals holds {len(evals)} bytes, A, B, C(rx, ry) are 96")
        nx, ny = num_cons.bit_length() - 1, num_vars.bit_length()
        rx = (C.c_uint8 * (32 * nx))(); ry = (C.c_uint8 * (32 * ny))(); acc = C.c_int(0)
        self._chk(lib().sbn_r1cs_proof_verify(self.h, C.c_size_t(num_cons), C.c_size_t(num_vars), _ptr(inputs) if inputs else None, C.c_size_t(len(inputs) // 32 if inputs else 0),
                                              _ptr(evals), gens_pc.h, gens_3.h, gens_4.h, _ptr(proof), tr.h, rx, ry, C.byref(acc)), "sbn_r1cs_proof_verify")
        return (bytes(rx), bytes(ry)) if acc.value else None

    # ---- many short sums of fresh points in one launch (the verifier's vartime_multiscalar_mul over a handful of proof points)
    def g1_small_sums(self, points_xy, scalars, counts):
        """sbn_g1_small_sums: sum i = sum of scalars[j] * points[j] over the next counts[i] entries -> (len(counts) x 64 canonical affine bytes, flags:
        1 = the identity).  points_xy: 64 bytes each, all-zero = the identity; scalars: canonical, 32 bytes each; at most 64 terms a sum and 256 sums.
        Misuse raises SbnError"""
        total = sum(counts)
        if len(points_xy) != 64 * total or len(scalars) != 32 * total:
            raise ValueError(f"g1_small_sums: {len(points_xy)} point bytes and {len(scalars)} scalar bytes, the counts need {64 * total} and {32 * total}")
        n = len(counts)
        cn = (C.c_uint32 * max(n, 1))(*counts)
        xy, inf = (C.c_uint8 * max(64 * n, 1))(), (C.c_uint8 * max(n, 1))()
        self._chk(lib().sbn_g1_small_sums(self.h, _ptr(points_xy), _ptr(scalars), cn, C.c_size_t(n), xy, inf), "sbn_g1_small_sums")
        return bytes(xy[:64 * n]), bytes(inf[:n])

    # ---- SparseMatPolyEvalProof::verify in one call (sparse_mlpoly_full.rs:1815-1845)
    def sparse_eval_verify(self, nx, ny, num_ops, num_cells, batch, comm_ops, comm_mem, rx, ry, evals, gens_ops, gens_mem, gens_derefs, proof, tr):
        """SparseMatPolyEvalProof::verify (sbn_sparse_eval_verify) -> True, or False when the proof is refused.  comm_ops / comm_mem: Bases of the row
        commitments of comb_ops / comb_mem; rx, ry, evals: canonical scalars, 32 bytes each; proof: the out_proof of sparse_eval_prove; `tr` moves on only
        when the proof is accepted.  Misuse raises SbnError"""
        n_proof = sparse_eval_sizes(nx, ny, num_ops, batch)[1]
        if len(proof) != n_proof:
            raise ValueError(f"sparse_eval_verify: the proof holds {len(proof)} bytes, the shape needs {n_proof}")
        if len(rx) != 32 * nx or len(ry) != 32 * ny or len(evals) != 32 * batch:
            raise ValueError("sparse_eval_verify: rx, ry or evals does not have the shape's length")
        acc = C.c_int(0)
        self._chk(lib().sbn_sparse_eval_verify(self.h, C.c_size_t(nx), C.c_size_t(ny), C.c_size_t(num_ops), C.c_size_t(num_cells), C.c_size_t(batch), comm_ops.h, comm_mem.h,
                                               _ptr(rx), _ptr(ry), _ptr(evals), gens_ops.h, gens_mem.h, gens_derefs.h, _ptr(proof), tr.h, C.byref(acc)), "sbn_sparse_eval_verify")
        return bool(acc.value)

    # ---- SparseMatPolyEvalProof::prove in one call (sparse_mlpoly_full.rs:1700-1755)
    def sparse_eval_prove(self, dense, rx, ry, evals, gens_ops, gens_mem, gens_derefs, rnd, tr):
        """SparseMatPolyEvalProof::prove (sbn_sparse_eval_prove) -> proof bytes, laid out as include/sbn254.h describes.  dense: a Dense (only read);
        rx, ry, evals: canonical scalars, 32 bytes each; gens_*: R + 1 generators with h; rnd: sparse_eval_sizes(...)[0] scalars; `tr` (Transcript) moves on"""
        nx, ny = len(rx) // 32, len(ry) // 32
        n_rnd, n_proof = sparse_eval_sizes(nx, ny, dense.num_ops, dense.batch)
        if len(rnd) != 32 * n_rnd:
            raise ValueError(f"sparse_eval_prove: rnd holds {len(rnd)} bytes, the shape needs {32 * n_rnd}")
        if len(evals) != 32 * dense.batch:
            raise ValueError(f"sparse_eval_prove: evals holds {len(evals)} bytes, the batch needs {32 * dense.batch}  [sparse_mlpoly_full.rs:1711 assert_eq]")
        proof = (C.c_uint8 * n_proof)()
        self._chk(lib().sbn_sparse_eval_prove(self.h, dense.h, _ptr(rx) if rx else None, C.c_size_t(nx), _ptr(ry) if ry else None, C.c_size_t(ny), _ptr(evals),
                                              gens_ops.h, gens_mem.h, gens_derefs.h, _ptr(rnd), tr.h, proof), "sbn_sparse_eval_prove")
        return bytes(proof)

    # ---- the KZG build's SparseMatPolyEvalProof::prove in one call (sparse_mlpoly_full.rs:1757-1813) and its derefs key
    def derefs_key_build(self, dense, srs):
        """S[side][a] = the sum of the SRS powers at the ops of cell a (sbn_derefs_key_build) -> DerefsKey"""
        h = C.c_void_p()
        self._chk(lib().sbn_derefs_key_build(self.h, dense.h, srs.h, C.byref(h)), "sbn_derefs_key_build")
        return DerefsKey(self, h)

    def derefs_key_commit(self, key, mem_rx, mem_ry):
        """Derefs::commit_kzg from the two eq tables -> (xy, is_inf): the point kzg_commit gives on the gathered, merged table"""
        out = (C.c_uint8 * 64)(); inf = C.c_int()
        self._chk(lib().sbn_derefs_key_commit(self.h, key.h, mem_rx.h, mem_ry.h, out, C.byref(inf)), "sbn_derefs_key_commit")
        return bytes(out), bool(inf.value)

    def sparse_eval_prove_kzg(self, dense, rx, ry, evals, gens_ops, gens_mem, srs, key, rnd, tr):
        """SparseMatPolyEvalProof::prove of the KZG build (sbn_sparse_eval_prove_kzg) -> proof bytes, laid out as include/sbn254.h describes.
        srs: a KZG SRS (no h) of at least npo2(2 batch) N - 1 points; key: a DerefsKey of (dense, srs) or None; rnd: sparse_eval_kzg_sizes(...)[0]
        scalars; `tr` (Transcript) moves on"""
        nx, ny = len(rx) // 32, len(ry) // 32
        n_rnd, n_proof = sparse_eval_kzg_sizes(nx, ny, dense.num_ops, dense.batch)
        if len(rnd) != 32 * n_rnd:
            raise ValueError(f"sparse_eval_prove_kzg: rnd holds {len(rnd)} bytes, the shape needs {32 * n_rnd}")
        if len(evals) != 32 * dense.batch:
            raise ValueError(f"sparse_eval_prove_kzg: evals holds {len(evals)} bytes, the batch needs {32 * dense.batch}  [sparse_mlpoly_full.rs:1769 assert_eq]")
        proof = (C.c_uint8 * n_proof)()
        self._chk(lib().sbn_sparse_eval_prove_kzg(self.h, dense.h, _ptr(rx) if rx else None, C.c_size_t(nx), _ptr(ry) if ry else None, C.c_size_t(ny), _ptr(evals),
                                                  gens_ops.h, gens_mem.h, srs.h, key.h if key is not None else None, _ptr(rnd), tr.h, proof), "sbn_sparse_eval_prove_kzg")
        return bytes(proof)

    # ---- KZG mode (kzg.rs): the SRS is a Bases handle, polynomials are the first n entries of a Table
    def kzg_srs_upload(self, powers_xy, flags=0):
        hb = C.c_void_p()
        self._chk(lib().sbn_kzg_srs_upload(self.h, _ptr(powers_xy), C.c_size_t(len(powers_xy) // 64), C.c_uint32(flags), C.byref(hb)), "sbn_kzg_srs_upload")
        return Bases(self, hb)

    def kzg_srs_from_tau(self, tau, n):
        """[tau^i]G1 for i < n, built on the device"""
        hb = C.c_void_p()
        self._chk(lib().sbn_kzg_srs_from_tau(self.h, _ptr(tau), C.c_size_t(n), C.byref(hb)), "sbn_kzg_srs_from_tau")
        return Bases(self, hb)

    def kzg_srs_load(self, data, flags=0, want_lines=True):
        """sbn_kzg_srs_load on the bytes of an SRS file -> (Bases, G2Lines of g2 or None, G2Lines of tau_g2 or None, g2_xy, tau_g2_xy).  A refusal
        raises SbnError with the index of the refused power in `.bad_index` (None where the refusal is not a power's)"""
        hb, hg, ht = C.c_void_p(), C.c_void_p(), C.c_void_p()
        xy = (C.c_uint8 * 256)(); bad = C.c_size_t(0)
        rc = lib().sbn_kzg_srs_load(self.h, _ptr(data) if len(data) else None, C.c_size_t(len(data)), C.c_uint32(flags), C.byref(hb),
                                    C.byref(hg) if want_lines else None, C.byref(ht) if want_lines else None, xy, C.byref(bad))
        if rc:
            err = SbnError(f"sbn_kzg_srs_load: rc={rc}: {lib().sbn_last_error(self.h).decode()}")
            err.bad_index = bad.value if bad.value != C.c_size_t(-1).value else None
            err.handles = (hb.value, hg.value, ht.value)
            raise err
        raw = bytes(xy)
        return Bases(self, hb), (G2Lines(self, hg) if want_lines else None), (G2Lines(self, ht) if want_lines else None), raw[:128], raw[128:]

    def kzg_srs_load_ptau(self, data, n=0, flags=0, want_lines=True):
        """sbn_kzg_srs_load_ptau on the bytes of a .ptau file: the first n powers (0: all) -> what kzg_srs_load returns, with its SbnError on a refusal"""
        hb, hg, ht = C.c_void_p(), C.c_void_p(), C.c_void_p()
        xy = (C.c_uint8 * 256)(); bad = C.c_size_t(0)
        rc = lib().sbn_kzg_srs_load_ptau(self.h, _ptr(data) if len(data) else None, C.c_size_t(len(data)), C.c_size_t(n), C.c_uint32(flags), C.byref(hb),
                                         C.byref(hg) if want_lines else None, C.byref(ht) if want_lines else None, xy, C.byref(bad))
        if rc:
            err = SbnError(f"sbn_kzg_srs_load_ptau: rc={rc}: {lib().sbn_last_error(self.h).decode()}")
            err.bad_index = bad.value if bad.value != C.c_size_t(-1).value else None
            err.handles = (hb.value, hg.value, ht.value)
            raise err
        raw = bytes(xy)
        return Bases(self, hb), (G2Lines(self, hg) if want_lines else None), (G2Lines(self, ht) if want_lines else None), raw[:128], raw[128:]

    def kzg_srs_check(self, srs, g2, tau_g2, rho):
        """sbn_kzg_srs_check -> True when the handle's points are the powers of one tau that matches tau_g2 (batched by the powers of rho)"""
        ok = C.c_int(0)
        self._chk(lib().sbn_kzg_srs_check(self.h, srs.h, g2.h, tau_g2.h, _ptr(rho), C.byref(ok)), "sbn_kzg_srs_check")
        return bool(ok.value)

    def kzg_srs_save_size(self, srs):
        n = C.c_size_t(0)
        self._chk(lib().sbn_kzg_srs_save(self.h, srs.h, None, None, C.c_uint32(0), None, C.c_size_t(0), C.byref(n)), "sbn_kzg_srs_save")
        return n.value

    def kzg_srs_save(self, srs, g2_xy, tau_g2_xy, flags=0, out=None):
        """sbn_kzg_srs_save -> the file's bytes.  `out`: a writable buffer (bytearray or numpy uint8) to fill instead; its length is the cap"""
        buf = bytearray(self.kzg_srs_save_size(srs)) if out is None else out
        n = C.c_size_t(0)
        self._chk(lib().sbn_kzg_srs_save(self.h, srs.h, _ptr(g2_xy), _ptr(tau_g2_xy), C.c_uint32(flags), _ptr(buf), C.c_size_t(len(buf)), C.byref(n)), "sbn_kzg_srs_save")
        return bytes(buf[:n.value]) if out is None else n.value

    def kzg_commit(self, srs, t, n=None):
        out = (C.c_uint8 * 64)(); inf = C.c_int()
        self._chk(lib().sbn_kzg_commit(self.h, srs.h, t.h, C.c_size_t(len(t) if n is None else n), out, C.byref(inf)), "sbn_kzg_commit")
        return bytes(out), bool(inf.value)

    def poly_div_linear(self, t, n, z):
        """-> (p(z), quotient Table or None when n <= 1)"""
        ev = (C.c_uint8 * 32)(); q = C.c_void_p()
        self._chk(lib().sbn_poly_div_linear(self.h, t.h, C.c_size_t(n), _ptr(z), ev, C.byref(q)), "sbn_poly_div_linear")
        return bytes(ev), (Table(self, q) if q.value else None)

    def kzg_open(self, srs, t, n, z):
        """-> (p(z), proof_xy, proof_is_inf)"""
        ev = (C.c_uint8 * 32)(); out = (C.c_uint8 * 64)(); inf = C.c_int()
        self._chk(lib().sbn_kzg_open(self.h, srs.h, t.h, C.c_size_t(n), _ptr(z), ev, out, C.byref(inf)), "sbn_kzg_open")
        return bytes(ev), bytes(out), bool(inf.value)

    def kzg_open_batched(self, srs, ts, ns, z, gamma):
        """-> ([p_k(z)], proof_xy, proof_is_inf)"""
        k = len(ts)
        arr = (C.c_void_p * max(k, 1))(*[t.h for t in ts]); nn = (C.c_size_t * max(k, 1))(*ns)
        ev = (C.c_uint8 * (32 * max(k, 1)))(); out = (C.c_uint8 * 64)(); inf = C.c_int()
        self._chk(lib().sbn_kzg_open_batched(self.h, srs.h, arr, nn, C.c_size_t(k), _ptr(z), _ptr(gamma), ev, out, C.byref(inf)), "sbn_kzg_open_batched")
        return [bytes(ev[32 * i:32 * i + 32]) for i in range(k)], bytes(out), bool(inf.value)

    # ---- pairings and KZG verification (kzg.rs:196-217, :315-352)
    def g2_prepare(self, q_xy, flags=0):
        """sbn_g2_prepare: 128 bytes x.c0 | x.c1 | y.c0 | y.c1 -> G2Lines.  A point that is not canonical, the identity, off E' or outside the
        r-torsion raises SbnError"""
        if len(q_xy) != 128:
            raise ValueError(f"g2_prepare: a G2 point is 128 bytes, got {len(q_xy)}")
        h = C.c_void_p()
        self._chk(lib().sbn_g2_prepare(self.h, _ptr(q_xy), C.c_uint32(flags), C.byref(h)), "sbn_g2_prepare")
        return G2Lines(self, h)

    def pairing_products(self, p_xy, qs, counts, want_gt=True):
        """sbn_pairing_products: check i = the product of e(P, Q) over the next counts[i] entries of p_xy (64 bytes each) and qs (G2Lines)
        -> (is_one bytes, [384 GT bytes a check] or None).  One launch, one wave a check; at most 4 terms a check.  Misuse raises SbnError"""
        total, n = sum(counts), len(counts)
        if len(p_xy) != 64 * total or len(qs) != total:
            raise ValueError(f"pairing_products: {len(p_xy)} point bytes and {len(qs)} handles, the counts need {64 * total} and {total}")
        cn = (C.c_uint32 * max(n, 1))(*counts)
        arr = (C.c_void_p * max(total, 1))(*[q.h for q in qs])
        one = (C.c_uint8 * max(n, 1))(); gt = (C.c_uint8 * max(384 * n, 1))() if want_gt else None
        self._chk(lib().sbn_pairing_products(self.h, _ptr(p_xy) if total else None, arr, cn, C.c_size_t(n), one, gt), "sbn_pairing_products")
        raw = bytes(gt) if want_gt else None
        return bytes(one[:n]), ([raw[384 * i:384 * i + 384] for i in range(n)] if want_gt else None)

    def kzg_verify(self, g2, tau_g2, comm_xy, z, eval_, proof_xy):
        """KZGProof::verify (sbn_kzg_verify) -> True / False.  comm_xy, proof_xy: 64 canonical affine bytes (all-zero: the identity)"""
        acc = C.c_int(0)
        self._chk(lib().sbn_kzg_verify(self.h, g2.h, tau_g2.h, _ptr(comm_xy), _ptr(z), _ptr(eval_), _ptr(proof_xy), C.byref(acc)), "sbn_kzg_verify")
        return bool(acc.value)

    def kzg_verify_batched(self, g2, tau_g2, comms_xy, z, gamma, evals, proof_xy):
        """KZGBatchProof::batch_verify (sbn_kzg_verify_batched) -> True / False.  comms_xy: count x 64 bytes, evals: count x 32 bytes (or a list)"""
        if isinstance(evals, (list, tuple)):
            evals = b"".join(evals)
        k = len(comms_xy) // 64
        if len(comms_xy) != 64 * k or len(evals) != 32 * k:
            raise ValueError(f"kzg_verify_batched: {len(comms_xy)} commitment bytes and {len(evals)} eval bytes")
        acc = C.c_int(0)
        self._chk(lib().sbn_kzg_verify_batched(self.h, g2.h, tau_g2.h, _ptr(comms_xy) if k else None, C.c_size_t(k), _ptr(z), _ptr(gamma),
                                               _ptr(evals) if k else None, _ptr(proof_xy), C.byref(acc)), "sbn_kzg_verify_batched")
        return bool(acc.value)

    def sparse_eval_verify_kzg(self, nx, ny, num_ops, num_cells, batch, comm_ops, comm_mem, rx, ry, evals, gens_ops, gens_mem, g2, tau_g2, proof, tr):
        """SparseMatPolyEvalProof::verify of the KZG build (sbn_sparse_eval_verify_kzg) -> True, or False when the proof is refused.  As
        sparse_eval_verify with G2Lines of srs.g2 / srs.tau_g2 in place of gens_derefs; proof: the out_proof of sparse_eval_prove_kzg; `tr` moves on
        only when the proof is accepted.  Misuse raises SbnError"""
        n_proof = sparse_eval_kzg_sizes(nx, ny, num_ops, batch)[1]
        if len(proof) != n_proof:
            raise ValueError(f"sparse_eval_verify_kzg: the proof holds {len(proof)} bytes, the shape needs {n_proof}")
        if len(rx) != 32 * nx or len(ry) != 32 * ny or len(evals) != 32 * batch:
            raise ValueError("sparse_eval_verify_kzg: rx, ry or evals does not have the shape's length")
        acc = C.c_int(0)
        self._chk(lib().sbn_sparse_eval_verify_kzg(self.h, C.c_size_t(nx), C.c_size_t(ny), C.c_size_t(num_ops), C.c_size_t(num_cells), C.c_size_t(batch), comm_ops.h, comm_mem.h,
                                                   _ptr(rx), _ptr(ry), _ptr(evals), gens_ops.h, gens_mem.h, g2.h, tau_g2.h, _ptr(proof), tr.h, C.byref(acc)), "sbn_sparse_eval_verify_kzg")
        return bool(acc.value)

    # ---- R1CS matrices on the device (r1cs.rs): multiply_vec, the phase-2 table, evaluate
    def r1cs_upload(self, num_cons, num_vars, mats, flags=0):
        """mats: three (rows, cols, vals) triplets for A, B, C; rows / cols: sequences or numpy arrays of uint32,
        vals: 32 bytes per entry (bytes or a numpy uint8 array)"""
        import numpy as np
        if len(mats) != 3:
            raise ValueError("r1cs_upload: mats must hold A, B and C")
        keep, rows, cols, vals, nnz = [], (C.c_void_p * 3)(), (C.c_void_p * 3)(), (C.c_void_p * 3)(), (C.c_size_t * 3)()
        for m, (r, c, v) in enumerate(mats):
            r = np.ascontiguousarray(r, dtype=np.uint32); c = np.ascontiguousarray(c, dtype=np.uint32)
            v = np.frombuffer(v, dtype=np.uint8) if isinstance(v, (bytes, bytearray)) else np.ascontiguousarray(v, dtype=np.uint8).reshape(-1)
            n = len(r)
            if len(c) != n or len(v) != 32 * n:
                raise ValueError(f"r1cs_upload: matrix {m}: {n} rows, {len(c)} cols, {len(v)} value bytes")
            keep += [r, c, v]
            nnz[m] = n
            rows[m] = r.ctypes.data if n else None; cols[m] = c.ctypes.data if n else None; vals[m] = v.ctypes.data if n else None
        h = C.c_void_p()
        self._chk(lib().sbn_r1cs_upload(self.h, C.c_size_t(num_cons), C.c_size_t(num_vars), rows, cols, vals, nnz, C.c_uint32(flags), C.byref(h)),
                  "sbn_r1cs_upload")
        return R1cs(self, h, num_cons, num_vars)

    def r1cs_multiply(self, m, z):
        """-> (Az, Bz, Cz) tables of num_cons entries"""
        a, b, c = C.c_void_p(), C.c_void_p(), C.c_void_p()
        self._chk(lib().sbn_r1cs_multiply(self.h, m.h, z.h, C.byref(a), C.byref(b), C.byref(c)), "sbn_r1cs_multiply")
        return Table(self, a), Table(self, b), Table(self, c)

    def r1cs_eval_table(self, m, rx, rA, rB, rC):
        """r_A evals_A + r_B evals_B + r_C evals_C at eq(rx): a table of 2 num_vars entries"""
        ht = C.c_void_p()
        self._chk(lib().sbn_r1cs_eval_table(self.h, m.h, _ptr(rx), C.c_size_t(len(rx) // 32), _ptr(rA), _ptr(rB), _ptr(rC), C.byref(ht)),
                  "sbn_r1cs_eval_table")
        return Table(self, ht)

    def r1cs_evaluate(self, m, rx, ry):
        """-> (A(rx, ry), B(rx, ry), C(rx, ry)) as canonical 32-byte scalars"""
        out = (C.c_uint8 * 96)()
        self._chk(lib().sbn_r1cs_evaluate(self.h, m.h, _ptr(rx), C.c_size_t(len(rx) // 32), _ptr(ry), C.c_size_t(len(ry) // 32), out),
                  "sbn_r1cs_evaluate")
        return bytes(out[0:32]), bytes(out[32:64]), bytes(out[64:96])

    # ---- the dense representation of the R1CS matrices (sparse_mlpoly_full.rs:120-174): addresses, timestamps, comb_ops, comb_mem
    def dense_build(self, num_vars_x, num_vars_y, mats, flags=0):
        """mats: 1 .. 8 (rows, cols, vals) triplets as for r1cs_upload, in the caller's entry order"""
        import numpy as np
        b = len(mats); nb = max(b, 1)
        keep, rows, cols, vals, nnz = [], (C.c_void_p * nb)(), (C.c_void_p * nb)(), (C.c_void_p * nb)(), (C.c_size_t * nb)()
        for m, (r, c, v) in enumerate(mats):
            r = np.ascontiguousarray(r, dtype=np.uint32); c = np.ascontiguousarray(c, dtype=np.uint32)
            v = np.frombuffer(v, dtype=np.uint8) if isinstance(v, (bytes, bytearray)) else np.ascontiguousarray(v, dtype=np.uint8).reshape(-1)
            n = len(r)
            if len(c) != n or len(v) != 32 * n:
                raise ValueError(f"dense_build: matrix {m}: {n} rows, {len(c)} cols, {len(v)} value bytes")
            keep += [r, c, v]
            nnz[m] = n
            rows[m] = r.ctypes.data if n else None; cols[m] = c.ctypes.data if n else None; vals[m] = v.ctypes.data if n else None
        h = C.c_void_p()
        self._chk(lib().sbn_dense_build(self.h, C.c_size_t(num_vars_x), C.c_size_t(num_vars_y), rows, cols, vals, nnz, C.c_size_t(b), C.c_uint32(flags),
                                        C.byref(h)), "sbn_dense_build")
        return Dense(self, h)

    # ---- the witness check and the reference's public surface in one call each (snark.rs:59-158, :290-529)
    def r1cs_is_sat(self, m, vars_, input_):
        """R1CSShape::is_sat (sbn_r1cs_is_sat) -> (sat, violated rows, the lowest of them).  vars_: a Table of at most num_vars entries; input_: bytes"""
        sat, nb, fb = C.c_int(-1), C.c_uint64(0), C.c_uint64(0)
        self._chk(lib().sbn_r1cs_is_sat(self.h, m.h, vars_.h, _ptr(input_) if input_ else None, C.c_size_t(len(input_) // 32), C.byref(sat), C.byref(nb), C.byref(fb)), "sbn_r1cs_is_sat")
        return bool(sat.value), nb.value, fb.value

    def snark_gens_new(self, num_cons, num_vars, num_inputs, num_nz_entries):
        """SNARKGens::new on the raw sizes (sbn_snark_gens_new) -> SnarkGens"""
        h = C.c_void_p()
        self._chk(lib().sbn_snark_gens_new(self.h, C.c_size_t(num_cons), C.c_size_t(num_vars), C.c_size_t(num_inputs), C.c_size_t(num_nz_entries), C.byref(h)), "sbn_snark_gens_new")
        return SnarkGens(self, h)

    def snark_encode(self, num_cons, num_vars, num_inputs, mats, gens, flags=0):
        """Instance::new + SNARK::encode (sbn_snark_encode) -> SnarkKey.  The shape and the columns are raw; mats: A, B, C as for r1cs_upload"""
        keep, rows, cols, vals, nnz = _three_mats("snark_encode", mats)      # noqa: F841 (keep: the arrays live until the call returns)
        h = C.c_void_p()
        self._chk(lib().sbn_snark_encode(self.h, C.c_size_t(num_cons), C.c_size_t(num_vars), C.c_size_t(num_inputs), rows, cols, vals, nnz, C.c_uint32(flags), gens.h, C.byref(h)),
                  "sbn_snark_encode")
        return SnarkKey(self, h)

    def snark_key_from_comm(self, comm):
        """the verifier's half of a key from R1CSCommitment's bytes (sbn_snark_key_from_comm); malformed bytes raise SbnError"""
        h = C.c_void_p()
        self._chk(lib().sbn_snark_key_from_comm(self.h, _ptr(comm) if comm else None, C.c_size_t(len(comm)), C.byref(h)), "sbn_snark_key_from_comm")
        return SnarkKey(self, h)

    def snark_is_sat(self, key, vars_, input_):
        """Instance::is_sat (sbn_snark_is_sat) -> (sat, violated rows, the lowest of them)"""
        sat, nb, fb = C.c_int(-1), C.c_uint64(0), C.c_uint64(0)
        self._chk(lib().sbn_snark_is_sat(self.h, key.h, vars_.h, _ptr(input_) if input_ else None, C.c_size_t(len(input_) // 32), C.byref(sat), C.byref(nb), C.byref(fb)), "sbn_snark_is_sat")
        return bool(sat.value), nb.value, fb.value

    def snark_prove(self, key, vars_, input_, gens, rnd, tr, check_sat=False, srs=None, derefs_key=None):
        """SNARK::prove (sbn_snark_prove; with srs: sbn_snark_prove_kzg) -> proof bytes.  vars_: a Table of at most num_vars_padded entries; rnd:
        key.sizes(kzg)[0] scalars; `tr` (Transcript) moves on.  check_sat: an unsatisfied witness raises SbnUnsat before any proving launch"""
        kzg = srs is not None
        n_rnd, n_proof = key.sizes(kzg)
        if len(rnd) != 32 * n_rnd:
            raise ValueError(f"snark_prove: rnd holds {len(rnd)} bytes, the shape needs {32 * n_rnd}")
        proof = (C.c_uint8 * n_proof)()
        flags = C.c_uint32(SBN_SNARK_CHECK_SAT if check_sat else 0)
        inp, ni = (_ptr(input_) if input_ else None), C.c_size_t(len(input_) // 32)
        if kzg:
            rc = lib().sbn_snark_prove_kzg(self.h, key.h, vars_.h, inp, ni, gens.h, srs.h, derefs_key.h if derefs_key is not None else None, flags, _ptr(rnd), tr.h, proof)
        else:
            rc = lib().sbn_snark_prove(self.h, key.h, vars_.h, inp, ni, gens.h, flags, _ptr(rnd), tr.h, proof)
        if rc == SBN_EUNSAT:
            raise SbnUnsat(f"sbn_snark_prove: rc={rc}: {lib().sbn_last_error(self.h).decode()}")
        self._chk(rc, "sbn_snark_prove_kzg" if kzg else "sbn_snark_prove")
        return bytes(proof)

    def snark_verify(self, key, input_, gens, proof, tr, g2=None, tau_g2=None):
        """SNARK::verify (sbn_snark_verify; with g2 and tau_g2: sbn_snark_verify_kzg) -> True, or False when the proof is refused; `tr` moves on only
        when it is accepted.  Misuse (a wrong proof length among it) raises SbnError"""
        acc = C.c_int(0)
        inp, ni = (_ptr(input_) if input_ else None), C.c_size_t(len(input_) // 32)
        if g2 is not None:
            self._chk(lib().sbn_snark_verify_kzg(self.h, key.h, inp, ni, gens.h, g2.h, tau_g2.h, _ptr(proof), C.c_size_t(len(proof)), tr.h, C.byref(acc)), "sbn_snark_verify_kzg")
        else:
            self._chk(lib().sbn_snark_verify(self.h, key.h, inp, ni, gens.h, _ptr(proof), C.c_size_t(len(proof)), tr.h, C.byref(acc)), "sbn_snark_verify")
        return bool(acc.value)

    # ---- NIZK mode in one call each (snark.rs:162-287): no encode, the verifier holds the matrices
    def nizk_gens_new(self, num_cons, num_vars, num_inputs):
        """NIZKGens::new on the raw sizes (sbn_nizk_gens_new) -> SnarkGens with pc, g3, g4 alone"""
        h = C.c_void_p()
        self._chk(lib().sbn_nizk_gens_new(self.h, C.c_size_t(num_cons), C.c_size_t(num_vars), C.c_size_t(num_inputs), C.byref(h)), "sbn_nizk_gens_new")
        return SnarkGens(self, h)

    def nizk_instance_new(self, num_cons, num_vars, num_inputs, mats, digest=b"", flags=0):
        """Instance::new (sbn_nizk_instance_new) -> NizkInst.  The shape and the columns are raw; mats: A, B, C as for r1cs_upload; digest: the bytes of
        the reference's inst.digest, absorbed as they are"""
        keep, rows, cols, vals, nnz = _three_mats("nizk_instance_new", mats)      # noqa: F841 (keep: the arrays live until the call returns)
        h = C.c_void_p()
        self._chk(lib().sbn_nizk_instance_new(self.h, C.c_size_t(num_cons), C.c_size_t(num_vars), C.c_size_t(num_inputs), rows, cols, vals, nnz, C.c_uint32(flags),
                                              _ptr(digest) if digest else None, C.c_size_t(len(digest)), C.byref(h)), "sbn_nizk_instance_new")
        return NizkInst(self, h, num_cons, num_vars, num_inputs)

    def nizk_is_sat(self, inst, vars_, input_):
        """Instance::is_sat (sbn_nizk_is_sat) -> (sat, violated rows, the lowest of them)"""
        sat, nb, fb = C.c_int(-1), C.c_uint64(0), C.c_uint64(0)
        self._chk(lib().sbn_nizk_is_sat(self.h, inst.h, vars_.h, _ptr(input_) if input_ else None, C.c_size_t(len(input_) // 32), C.byref(sat), C.byref(nb), C.byref(fb)), "sbn_nizk_is_sat")
        return bool(sat.value), nb.value, fb.value

    def nizk_prove(self, inst, vars_, input_, gens, rnd, tr, check_sat=False):
        """NIZK::prove (sbn_nizk_prove) -> proof bytes: the R1CS proof | rx | ry.  vars_: a Table of at most num_vars_padded entries; rnd: inst.sizes()[0]
        scalars; `tr` (Transcript) moves on.  check_sat: an unsatisfied witness raises SbnUnsat before any proving launch"""
        n_rnd, n_proof = inst.sizes()
        if len(rnd) != 32 * n_rnd:
            raise ValueError(f"nizk_prove: rnd holds {len(rnd)} bytes, the shape needs {32 * n_rnd}")
        proof = (C.c_uint8 * n_proof)()
        rc = lib().sbn_nizk_prove(self.h, inst.h, vars_.h, _ptr(input_) if input_ else None, C.c_size_t(len(input_) // 32), gens.h,
                                  C.c_uint32(SBN_SNARK_CHECK_SAT if check_sat else 0), _ptr(rnd), tr.h, proof)
        if rc == SBN_EUNSAT:
            raise SbnUnsat(f"sbn_nizk_prove: rc={rc}: {lib().sbn_last_error(self.h).decode()}")
        self._chk(rc, "sbn_nizk_prove")
        return bytes(proof)

    def nizk_verify(self, inst, input_, gens, proof, tr):
        """NIZK::verify (sbn_nizk_verify) -> True, or False when the proof is refused (a derived (rx, ry) that differs from the claimed one among it); `tr`
        moves on only when it is accepted.  Misuse (a wrong proof length among it) raises SbnError"""
        acc = C.c_int(0)
        self._chk(lib().sbn_nizk_verify(self.h, inst.h, _ptr(input_) if input_ else None, C.c_size_t(len(input_) // 32), gens.h, _ptr(proof), C.c_size_t(len(proof)), tr.h,
                                        C.byref(acc)), "sbn_nizk_verify")
        return bool(acc.value)

    # ---- circom's .r1cs and .wtns files straight onto the device (r1cs_reader.rs, keyless_benchmark.rs:38-72)
    def circom_r1cs_load(self, data):
        """R1CS::from_reader + to_sparse_matrices_padded on the bytes of a .r1cs file (sbn_circom_r1cs_load) -> CircomR1cs; a refused file raises SbnError.
        data: bytes, or a numpy uint8 array (passed where it lies)"""
        h = C.c_void_p()
        self._chk(lib().sbn_circom_r1cs_load(self.h, _ptr(data) if len(data) else None, C.c_size_t(len(data)), C.byref(h)), "sbn_circom_r1cs_load")
        return CircomR1cs(self, h)

    def r1cs_from_circom(self, cr):
        """the R1cs sbn_r1cs_upload makes of the parsed circuit's triplets (sbn_r1cs_from_circom)"""
        h = C.c_void_p()
        self._chk(lib().sbn_r1cs_from_circom(self.h, cr.h, C.byref(h)), "sbn_r1cs_from_circom")
        i = cr.info()
        return R1cs(self, h, i["num_cons_padded"], i["num_vars_padded"])

    def nizk_instance_from_circom(self, cr, digest=b""):
        """Instance::new on the parsed circuit (sbn_nizk_instance_from_circom) -> NizkInst"""
        h = C.c_void_p()
        self._chk(lib().sbn_nizk_instance_from_circom(self.h, cr.h, _ptr(digest) if digest else None, C.c_size_t(len(digest)), C.byref(h)), "sbn_nizk_instance_from_circom")
        i = cr.info()
        return NizkInst(self, h, i["num_constraints"], i["num_vars"], i["num_pub_inputs"])

    def snark_encode_circom(self, cr, gens):
        """Instance::new + SNARK::encode on the parsed circuit (sbn_snark_encode_circom) -> SnarkKey"""
        h = C.c_void_p()
        self._chk(lib().sbn_snark_encode_circom(self.h, cr.h, gens.h, C.byref(h)), "sbn_snark_encode_circom")
        return SnarkKey(self, h)

    def circom_wtns_load(self, data, num_inputs):
        """parse_wtns on the bytes of a .wtns file (sbn_circom_wtns_load) -> (vars Table, input bytes, the file's value count)"""
        t, n = C.c_void_p(), C.c_size_t(0)
        inp = (C.c_uint8 * (32 * max(num_inputs, 1)))()
        self._chk(lib().sbn_circom_wtns_load(self.h, _ptr(data) if len(data) else None, C.c_size_t(len(data)), C.c_size_t(num_inputs), C.byref(t), inp, C.byref(n)), "sbn_circom_wtns_load")
        return Table(self, t), bytes(inp)[:32 * num_inputs], n.value

    def circom_r1cs_digest(self, cr):
        """the library's own circuit digest of a parsed circuit, leaves hashed on the device (sbn_circom_r1cs_digest) -> 32 bytes"""
        return cr.digest()

    # ---- profiling
    def prof_enable(self, on=True):
        self._chk(lib().sbn_prof_enable(self.h, int(on)), "prof_enable")

    def prof_last_job(self):
        """{c, W, slots, buckets} of the most recent MSM / row commit on this context"""
        o = (C.c_uint64 * 4)(); self._chk(lib().sbn_prof_last_job(self.h, o), "prof_last_job")
        return {"c": int(o[0]), "W": int(o[1]), "slots": int(o[2]), "buckets": int(o[3])}

    def prof_last_acc(self):
        """accumulate / reduction geometry of the most recent BUCKET job on this context (a lookup-table commit leaves it unchanged):
        {SEG, LPB, L, chunks, levels (k_reduce_combine launches), quad, extra_count, big_count}; synchronises the stream"""
        o = (C.c_uint64 * 8)(); self._chk(lib().sbn_prof_last_acc(self.h, o), "prof_last_acc")
        return dict(zip(("SEG", "LPB", "L", "chunks", "levels", "quad", "extra_count", "big_count"), (int(v) for v in o)))

    def prof_reset(self):
        self._chk(lib().sbn_prof_reset(self.h), "prof_reset")

    def prof_get(self):
        res = {}
        for i in range(lib().sbn_prof_count(self.h)):
            name = C.c_char_p(); ms = C.c_double(); cnt = C.c_uint64()
            lib().sbn_prof_get(self.h, i, C.byref(name), C.byref(ms), C.byref(cnt))
            res[name.value.decode()] = (ms.value, cnt.value)
        return res
