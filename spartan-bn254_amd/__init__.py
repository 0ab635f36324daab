"""spartan-bn254_amd — ctypes loader for libsbn254_hip.so (the C ABI in include/sbn254.h).

The product is the shared library; this module only lets Python tests and bench.py call it the way the
Rust shim would.  It contains no arithmetic and no fallback: if the HIP library or a
gfx950 device is missing, loading / context creation raises.
"""
from .binding import (  # noqa: F401
    Context, Group, Bases, Table, Dense, DerefsKey, SnarkGens, SnarkKey, NizkInst, CircomR1cs, SbnError, SbnUnsat, SBN_EUNSAT, SBN_SNARK_CHECK_SAT, SBN_SRS_CHECK, kzg_srs_g2_from_tau, ptau_scan, PtauInfo, lib, lib_path, build_library,
    SBN_SCALARS_MONT, SBN_POINTS_MONT, g1_compress, g1_sum, Transcript, fr_from_wide, unipoly_from_evals, unipoly_eval, factored_lens, r1cs_proof_sizes, sparse_eval_sizes, sparse_eval_kzg_sizes, EXPORTED_SYMBOLS,
    RandomTape,
)

__version__ = "0.15.0"   # 15th extension of the C ABI's surface: sbn_random_tape_*, the sbn_*_draw_rnd plans, sbn_circom_r1cs_digest
