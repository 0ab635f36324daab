/*
 * sbn254.h — C ABI of libsbn254_hip.so: the MI355X (gfx950) implementation of Spartan-BN254's prover
 * hot path.  These are the entry points a Rust `extern "C"` block binds (INTEGRATION.md shows the shim);
 * every function cites the reference interface it replaces (paths relative to the reference repo).
 *
 * Conventions
 *   - return 0 on success, a negative SBN_E* code otherwise; sbn_last_error() has the text.
 *     The reference's prover functions are infallible (assert!/panic on misuse, errors.rs:19-31 is
 *     verifier-only), so the shim turns a non-zero code into panic!.
 *   - scalars: 32 B little-endian.  Default = canonical integer < r (Scalar::to_bytes, scalar.rs:75-84);
 *     with SBN_SCALARS_MONT the 4 x u64 Montgomery limbs ark-ff keeps in memory (R = 2^256) are taken as-is.
 *   - points: 64 B = x || y, each 32 B little-endian canonical integer < p; all-zero = point at infinity.
 *     With SBN_POINTS_MONT the coordinates are ark-ff Montgomery limbs instead (G1Affine's in-memory x, y).
 *   - `*_dev` variants take DEVICE pointers (hipMalloc'ed by the caller or by sbn_dev_alloc); the others take
 *     host pointers and stage through HBM themselves.
 *   - a context owns one HIP stream and a workspace; calls on one context are serialised by a mutex
 *     (hyrax.rs:259-261 may enter B1 from many rayon workers at once); use one context per thread for overlap.
 *   - per-circuit data (generator sets, the SRS, the R1CS matrices and their dense representation) is uploaded once into a handle (sbn_bases, sbn_r1cs, sbn_dense) that
 *     later calls read; calls that produce vectors return new sbn_tables, which the sumcheck calls take as they are.
 *   - there is NO CPU fallback: without a gfx950 device sbn_ctx_create fails.
 */
#ifndef SBN254_H
#define SBN254_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define SBN_OK 0
#define SBN_EINVAL (-1)   /* bad argument (NULL, size mismatch, non-canonical input when checked) */
#define SBN_EHIP (-2)     /* HIP runtime error */
#define SBN_ENODEV (-3)   /* no usable gfx950 device */
#define SBN_ENOMEM (-4)

#define SBN_SCALARS_MONT 1u
#define SBN_POINTS_MONT 2u

typedef struct sbn_ctx sbn_ctx;
typedef struct sbn_bases sbn_bases;   /* device-resident generator table: MultiCommitGens.{G_affine,h_affine} (commitments.rs:17-27) */
typedef struct sbn_table sbn_table;   /* device-resident Fr table: DensePolynomial.Z (hyrax.rs:155-160) */
/* (sbn_r1cs, the device-resident R1CSShape, is declared with its calls below) */

/* ---- context ---- */
int sbn_ctx_create(int device, sbn_ctx** out);
void sbn_ctx_destroy(sbn_ctx* ctx);
const char* sbn_last_error(const sbn_ctx* ctx);
/* run on the caller's HIP stream (hipStream_t as void*); NULL restores the context's own stream */
int sbn_ctx_set_stream(sbn_ctx* ctx, void* hip_stream);
int sbn_ctx_sync(sbn_ctx* ctx);
const char* sbn_version(void);

/* ---- raw device memory for callers without their own allocator (the Rust shim) ---- */
int sbn_dev_alloc(sbn_ctx* ctx, size_t bytes, void** out_dev);
int sbn_dev_free(sbn_ctx* ctx, void* dev);
int sbn_dev_upload(sbn_ctx* ctx, void* dst_dev, const void* src_host, size_t bytes);
int sbn_dev_download(sbn_ctx* ctx, void* dst_host, const void* src_dev, size_t bytes);

/* ---- B1: single MSM — GroupElement::msm_affine(scalars, points) (group.rs:171-175) and
 *      vartime_multiscalar_mul (group.rs:143-158).  out_is_inf may be NULL.
 *      n == 0 returns the identity, as arkworks' msm of empty slices does. ---- */
int sbn_msm(sbn_ctx* ctx, const uint8_t* scalars, const uint8_t* points, size_t n, uint32_t flags,
            uint8_t out_xy[64], int* out_is_inf);

/* vartime_multiscalar_mul (group.rs:143-158) takes PROJECTIVE points and converts each with its own inversion on the CPU
 * (group.rs:153); here the n Jacobian triples X||Y||Z (96 B each; Z = 0 is the identity) are normalised on the device. */
int sbn_msm_jacobian(sbn_ctx* ctx, const uint8_t* scalars, const uint8_t* points_xyz, size_t n, uint32_t flags,
                     uint8_t out_xy[64], int* out_is_inf);

/* ---- generator tables — MultiCommitGens (commitments.rs:17-27).  G: n points, h: 1 point or NULL.
 *      Stored on the device in Montgomery form; duplicates are detected so that commit() can merge the
 *      scalars of equal bases (the reference's derivation makes ~66 % of them equal to G, group.rs:110-131). ---- */
int sbn_bases_upload(sbn_ctx* ctx, const uint8_t* G_xy, size_t n, const uint8_t* h_xy, uint32_t flags, sbn_bases** out);
void sbn_bases_free(sbn_ctx* ctx, sbn_bases* b);
size_t sbn_bases_len(const sbn_bases* b);          /* n (without h) */
/* Fixed-base precomputation for a generator set that will serve many commitments (the per-circuit gens_derefs / gens_ops of
 * SparseMatPolyCommitmentGens, sparse_mlpoly_full.rs:619-627): a table of every digit multiple d * 2^(c w) * G_j in HBM, so a row
 * commitment costs ceil(254/c) mixed additions per scalar and no bucket work.  The largest window c <= 16 whose table fits
 * max_bytes is built (the reference's 8193 gens_r1cs_eval generators: 2814 unique x 16 windows x 32768 x 64 B = 94 GB at c = 16);
 * commits on this handle use it from then on.  Results are unchanged (same group element).  *window_bits (optional) <- c. */
int sbn_bases_precompute(sbn_ctx* ctx, sbn_bases* b, size_t max_bytes, int* window_bits);
/* MultiCommitGens::new(n, label) (commitments.rs:31-62): SHAKE256 stream -> from_uniform_bytes (group.rs:110-131);
 * builds G[0..n) and h on the device and, if out_xy != NULL, also returns the n+1 canonical points. */
int sbn_gens_new(sbn_ctx* ctx, size_t n, const uint8_t* label, size_t label_len, uint8_t* out_xy, sbn_bases** out);

/* Synthetic benchmark bases with known discrete logs: P_i = (s0 + (first + i) * d) * G for
 * i in [0, n), all distinct, built on the device; the expected MSM result is then (sum k_i (s0 + (first+i) d)) * G. */
int sbn_bases_synthetic(sbn_ctx* ctx, size_t n, uint64_t first, const uint8_t s0[32], const uint8_t d[32], sbn_bases** out);
/* Synthetic benchmark scalars, written to a DEVICE buffer of n x 32 B: scalar t = the SplitMix64 outputs of
 * counters 4*(first+t)+1 .. +4 (state = seed + counter * 0x9E3779B97F4A7C15) as four little-endian u64 limbs, the top limb cut
 * to 62 bits, minus r when >= r: canonical, full-width values of Fr (the same stream bench.py's numpy generator produces). */
int sbn_scalars_synthetic(sbn_ctx* ctx, uint64_t seed, uint64_t first, size_t n, void* out_dev);
/* copy `count` points starting at `first` back to the host as canonical x||y (for tests of resident tables) */
int sbn_bases_download(sbn_ctx* ctx, const sbn_bases* b, size_t first, size_t count, uint8_t* out_xy);

/* MultiCommitGens::split_at(mid) (commitments.rs:78-98): (G[..mid], h) and (G[mid..], h) */
int sbn_bases_split_at(sbn_ctx* ctx, const sbn_bases* b, size_t mid, sbn_bases** left, sbn_bases** right);
/* MultiCommitGens::scale(s) (commitments.rs:64-76): G_i <- s * G_i, h unchanged */
int sbn_bases_scale(sbn_ctx* ctx, const sbn_bases* b, const uint8_t s[32], sbn_bases** out);

/* MSM of n scalars against the first n points of a resident table (no h): msm_affine with cached G_affine */
int sbn_msm_bases(sbn_ctx* ctx, const sbn_bases* b, const uint8_t* scalars, size_t n, uint32_t flags,
                  uint8_t out_xy[64], int* out_is_inf);
int sbn_msm_bases_dev(sbn_ctx* ctx, const sbn_bases* b, const void* scalars_dev, size_t n, uint32_t flags,
                      uint8_t out_xy[64], int* out_is_inf);

/* ---- B2: Pedersen / Hyrax commitments ----
 * <[Scalar] as Commitments>::commit(blind, gens_n) = MSM(scalars || blind, G || h) (commitments.rs:144-154):
 *   sbn_commit_rows with L = 1.
 * DensePolynomial::commit -> commit_inner (hyrax.rs:253-267, 283-308): C[i] = commit(Z[i*R..(i+1)*R], blinds[i]),
 *   Z row-major L x R, R == sbn_bases_len(b), blinds NULL = all zero (random_tape == None, hyrax.rs:301-305).
 * out_xy: L x 64 B canonical affine; out_inf: L flags or NULL.  flags: SBN_SCALARS_MONT only; any other bit is SBN_EINVAL
 *   (also through sbn_group_commit_rows / sbn_group_commit_rows_dev). */
int sbn_commit_rows(sbn_ctx* ctx, const sbn_bases* b, const uint8_t* Z, const uint8_t* blinds, size_t L, size_t R,
                    uint32_t flags, uint8_t* out_xy, uint8_t* out_inf);
int sbn_commit_rows_dev(sbn_ctx* ctx, const sbn_bases* b, const void* Z_dev, const void* blinds_dev, size_t L, size_t R,
                        uint32_t flags, uint8_t* out_xy, uint8_t* out_inf);
/* arkworks serialize_compressed of n affine points (group.rs:135-140; what transcript.rs:102-108 absorbs) */
int sbn_g1_compress(const uint8_t* xy, size_t n, uint8_t* out32);
/* sum of n canonical affine points on the host (no device needed): the fold of per-GPU partial MSM results after
 * the RCCL all-gather, i.e. the `+` of GroupElement (group.rs:199-262) applied n-1 times */
int sbn_g1_sum(const uint8_t* xy, size_t n, uint8_t out_xy[64], int* out_is_inf);
/* UniPoly::from_evals (unipoly.rs:28-59): the round polynomial from its values at 0, 1, 2[, 3] (n = 3 or 4 canonical scalars,
 * in the order [e0, claim - e0, e2, e3] of sumcheck.rs:137); coeffs low..high.  Host only.  UniPoly::evaluate (unipoly.rs:74-82). */
int sbn_unipoly_from_evals(const uint8_t* evals, size_t n, uint8_t* coeffs);
int sbn_unipoly_eval(const uint8_t* coeffs, size_t n, const uint8_t r[32], uint8_t out[32]);
/* EqPolynomial::compute_factored_lens (hyrax.rs:371-373) */
void sbn_factored_lens(size_t ell, size_t* left, size_t* right);

/* ---- B3: sumcheck rounds on device-resident tables ----
 * A table is a DensePolynomial's Z vector (len a power of two).  Each eval returns the per-round values the
 * host needs for UniPoly::from_evals (unipoly.rs:28-59) as canonical 32 B scalars. */
int sbn_table_upload(sbn_ctx* ctx, const uint8_t* Z, size_t len, uint32_t flags, sbn_table** out);
int sbn_table_from_dev(sbn_ctx* ctx, const void* Z_dev, size_t len, uint32_t flags, sbn_table** out);
void sbn_table_free(sbn_ctx* ctx, sbn_table* t);
size_t sbn_table_len(const sbn_table* t);                                   /* current len (halves per bind) */
int sbn_table_download(sbn_ctx* ctx, const sbn_table* t, uint8_t* out /* len x 32 canonical */);
int sbn_table_read0(sbn_ctx* ctx, const sbn_table* t, uint8_t out[32]);     /* poly[0] after the last round (sumcheck.rs:157) */
/* the same for `count` tables in one launch and one wait (out: count x 32 bytes): the products of several product circuits
 * (ProductCircuit::evaluate, product_tree.rs:59-64, called per circuit at sparse_mlpoly_full.rs:1326-1345) after all of them were enqueued */
int sbn_table_read0_many(sbn_ctx* ctx, const sbn_table* const* ts, size_t count, uint8_t* out);
/* DensePolynomial::bound_poly_var_top(r) (hyrax.rs:195-203) */
int sbn_bind_top(sbn_ctx* ctx, sbn_table* t, const uint8_t r[32]);
int sbn_bind_top_many(sbn_ctx* ctx, sbn_table* const* ts, size_t count, const uint8_t r[32]);
/* prove_cubic inner loop, comb = A*B*C (sumcheck.rs:111-135; product_tree.rs:178-181): out = e0,e2,e3 */
int sbn_sc_eval_cubic(sbn_ctx* ctx, const sbn_table* A, const sbn_table* B, const sbn_table* C, uint8_t out[96]);
/* prove_cubic_batched inner loops (sumcheck.rs:201-267): instance i uses (A[i], B[i], C[i]); pass the shared
 * poly_C_par for the "par" instances.  out = count x (e0,e2,e3) */
int sbn_sc_eval_cubic_batched(sbn_ctx* ctx, const sbn_table* const* A, const sbn_table* const* B,
                              const sbn_table* const* C, size_t count, uint8_t* out /* count x 96 */);
/* prove_cubic_with_additive_term inner loop, comb = tau*(Az*Bz - Cz) (sumcheck.rs:502-530; r1csproof.rs:288-292) */
int sbn_sc_eval_r1cs(sbn_ctx* ctx, const sbn_table* tau, const sbn_table* Az, const sbn_table* Bz, const sbn_table* Cz,
                     uint8_t out[96]);
/* prove_quad inner loop, comb = z*ABC (sumcheck.rs:691-699; r1csproof.rs:389-390): out = e0,e2 */
int sbn_sc_eval_quad(sbn_ctx* ctx, const sbn_table* Z, const sbn_table* ABC, uint8_t out[64]);
/* Fused round: bind every distinct table among the arguments to r (bound_poly_var_top, as sumcheck.rs:148-150 / 289-299 /
 * 551-554 / 715-716 do after each challenge) AND return the NEXT round's sums on the bound tables — the same values the
 * separate bind + eval calls give, in one pass over the data.  Needs len >= 4.  Argument order as the eval calls. */
int sbn_sc_bind_eval_cubic_batched(sbn_ctx* ctx, sbn_table* const* A, sbn_table* const* B, sbn_table* const* C, size_t count,
                                   const uint8_t r[32], uint8_t* out /* count x 96 */);
int sbn_sc_bind_eval_r1cs(sbn_ctx* ctx, sbn_table* tau, sbn_table* Az, sbn_table* Bz, sbn_table* Cz, const uint8_t r[32], uint8_t out[96]);
int sbn_sc_bind_eval_quad(sbn_ctx* ctx, sbn_table* Z, sbn_table* ABC, const uint8_t r[32], uint8_t out[64]);
/* ---- SumcheckInstanceProof::prove_cubic_batched (sumcheck.rs:165-330; comb_func = A*B*C, its only call sites product_tree.rs:275-278)
 *      as a device-resident state; the transcript stays with the caller:
 *        begin -> evals of round 0;  per round: (UniPoly::from_evals, absorb, squeeze r_j) -> round(r_j) -> evals of round j+1;  finish.
 * What crosses the boundary per round is what the transcript absorbs: the coeffs-weighted combination of the instances' sums
 * (sumcheck.rs:269-271), i.e. (e0, e2, e3) = sum_i coeffs[i] * (e0, e2, e3)_i as three canonical scalars — not the per-instance
 * triples.  The "par" instances share C_par (:201-235), the "seq" instances have their own C (:238-267); coeffs: n_par + n_seq
 * canonical scalars, "par" first.  n_par + n_seq <= 24.  The caller's tables are only read: the state binds into buffers of its own.
 * Same field elements as the per-instance calls + a host-side combination, bit for bit. */
typedef struct sbn_sumcheck sbn_sumcheck;
int sbn_sumcheck_begin(sbn_ctx* ctx, const sbn_table* const* A_par, const sbn_table* const* B_par, const sbn_table* C_par, size_t n_par,
                       const sbn_table* const* A_seq, const sbn_table* const* B_seq, const sbn_table* const* C_seq, size_t n_seq,
                       const uint8_t* coeffs, uint8_t out_evals[96], sbn_sumcheck** out);
/* The same with poly_C_par = EqPolynomial::new(rand).evals() built inside the call (product_tree.rs:267-275: how every layer of
 * ProductCircuitEvalProofBatched::prove makes its C): rand = ell canonical scalars, 2^ell = the tables' length; the eq table belongs to the
 * state (its final claim is listed where C_par's is).  One call per layer instead of sbn_eq_evals + sbn_sumcheck_begin + sbn_table_free. */
int sbn_sumcheck_begin_eq(sbn_ctx* ctx, const sbn_table* const* A_par, const sbn_table* const* B_par, size_t n_par, const uint8_t* rand, size_t ell,
                          const sbn_table* const* A_seq, const sbn_table* const* B_seq, const sbn_table* const* C_seq, size_t n_seq,
                          const uint8_t* coeffs, uint8_t out_evals[96], sbn_sumcheck** out);
/* bind every table to r_j (sumcheck.rs:289-299); out_evals = the combined sums of the next round (zeros after the last bind) */
int sbn_sumcheck_round(sbn_ctx* ctx, sbn_sumcheck* st, const uint8_t r[32], uint8_t out_evals[96]);
size_t sbn_sumcheck_len(const sbn_sumcheck* st);                       /* current table length (halves per round) */
/* after the last round (length 1): poly[0] of every table (sumcheck.rs:302-318), 32 B each, in the order
 * A_par[0..n_par), B_par[0..n_par), C_par, A_seq[..], B_seq[..], C_seq[..] */
int sbn_sumcheck_finish(sbn_ctx* ctx, sbn_sumcheck* st, uint8_t* finals);
void sbn_sumcheck_free(sbn_ctx* ctx, sbn_sumcheck* st);
/* ---- transcript: Merlin v1.0 over STROBE-128 / Keccak-f[1600] (merlin::Transcript as src/transcript.rs uses it) ----
 * Host only: no context, works without a device.  append_message / challenge_bytes are Merlin's; challenge_scalar is
 * ProofTranscript::challenge_scalar (transcript.rs:56-67): 64 challenge bytes, little-endian, mod r, as 32 canonical bytes.
 * The state record is 203 bytes: the 200 sponge bytes, then pos, pos_begin, cur_flags (from_state rejects pos >= 166,
 * pos_begin > 166 and undefined flag bits).  A failed call (SBN_EINVAL) leaves the transcript as it was. */
typedef struct sbn_transcript sbn_transcript;
int sbn_transcript_new(const uint8_t* label, size_t label_len, sbn_transcript** out);
int sbn_transcript_clone(const sbn_transcript* t, sbn_transcript** out);
void sbn_transcript_free(sbn_transcript* t);
int sbn_transcript_append_message(sbn_transcript* t, const uint8_t* label, size_t label_len, const uint8_t* msg, size_t msg_len);
int sbn_transcript_challenge_bytes(sbn_transcript* t, const uint8_t* label, size_t label_len, uint8_t* out, size_t out_len);
int sbn_transcript_challenge_scalar(sbn_transcript* t, const uint8_t* label, size_t label_len, uint8_t out[32]);
int sbn_transcript_state(const sbn_transcript* t, uint8_t out[203]);
int sbn_transcript_from_state(const uint8_t in[203], sbn_transcript** out);
/* Fr::from_le_bytes_mod_order on 64 bytes: what challenge_scalar does with its challenge bytes.  Host only. */
int sbn_fr_from_wide(const uint8_t in[64], uint8_t out[32]);
/* SumcheckInstanceProof::prove_cubic_batched (sumcheck.rs:165-330) in ONE call: `st` fresh from sbn_sumcheck_begin /
 * sbn_sumcheck_begin_eq, rounds = log2(sbn_sumcheck_len(st)).  Every round's kernels are queued at once; between them a one-wave
 * kernel does the host's part on the device — the combination, e1 = e - e0, UniPoly::from_evals, the transcript's seven operations
 * (unipoly.rs:117-122, challenge_scalar("challenge_nextround")), e = poly(r_j) — and leaves r_j in device memory for the launches
 * behind it.  One wait, one copy back.  out_polys: rounds x 4 x 32 (c0..c3 of every round polynomial, canonical); out_r: rounds x 32;
 * finals as sbn_sumcheck_finish.  `tr` moves on only if the whole call succeeded; a failure after the first launch leaves `st` dead
 * (later calls return SBN_EINVAL).  Same values as the loop over sbn_sumcheck_round with the same transcript on the host, bit for bit. */
int sbn_sumcheck_prove(sbn_ctx* ctx, sbn_sumcheck* st, sbn_transcript* tr, const uint8_t claim[32], uint8_t* out_polys, uint8_t* out_r, uint8_t* finals);
/* ProductCircuitEvalProofBatched::prove (product_tree.rs:251-392) in ONE call: every layer's coeff_vec and joint claim (:317-321), its
 * prove_cubic_batched with poly_C_par = eq(rand) (:271, :323-332), the claim appends (:352-365), r_layer and the folded claims (:368-376),
 * with the transcript, `rand`, coeff_vec and claims_to_verify on the device throughout.  Everything is queued at once; one wait, one copy back.
 *   layers[i * n_layers + j]: circuit i's layer j as sbn_product_circuit{,_many} produce it (left || right, 2^(n_layers - j) entries; j = 0 is the
 *   input, the last one has two entries); the call takes the halves as sbn_table_halves does.  dotp_*: n_dotp DotProductCircuits of
 *   2^(n_layers - 1) entries, joined at layer 0 only (:296-309); n_dotp = 0 allowed.  ProductCircuit::evaluate (:262-264) and
 *   DotProductCircuit::evaluate (:298) are computed inside.  n_circ >= 1, n_circ + n_dotp <= 24, n_layers >= 1.
 * The layer whose halves have one entry (no sumcheck round) is part of the proof: coeff_vec, the 2 n_circ appends and r_layer are drawn there too.
 *   out_polys:  sum_k k rounds (k = 0 .. n_layers - 1, top layer first) x 4 x 32: c0..c3 of every round polynomial
 *   out_claims: per layer, top first: claims_prod_left[n_circ], claims_prod_right[n_circ]; behind the last layer claims_dotp left[n_dotp], right[n_dotp], weight[n_dotp]
 *   out_rand:   n_layers x 32: the final `rand` (r_layer of the last layer first, :374-376)
 *   out_claims_final: n_circ x 32: claims_to_verify behind the last layer (= layer 0 of circuit i evaluated at out_rand)
 * All scalars out are canonical.  The caller's tables are only read.  `tr` moves on only if the whole call succeeded.  Same values, bit for bit, as
 * the layer loop over sbn_table_halves, sbn_transcript_challenge_scalar, sbn_sumcheck_begin_eq, sbn_sumcheck_prove / _round, sbn_sumcheck_finish and
 * sbn_transcript_append_message. */
int sbn_product_proof_prove(sbn_ctx* ctx, const sbn_table* const* layers, size_t n_circ, size_t n_layers,
                            const sbn_table* const* dotp_left, const sbn_table* const* dotp_right, const sbn_table* const* dotp_weight, size_t n_dotp,
                            sbn_transcript* tr, uint8_t* out_polys, uint8_t* out_claims, uint8_t* out_rand, uint8_t* out_claims_final);
/* EqPolynomial::evals (hyrax.rs:355-369) built on the device */
int sbn_eq_evals(sbn_ctx* ctx, const uint8_t* r, size_t ell, sbn_table** out);

/* ---- Hyrax opening pieces ----
 * compute_dotproduct (hyrax.rs:409-415) of two equally long tables */
int sbn_table_dot(sbn_ctx* ctx, const sbn_table* a, const sbn_table* b, uint8_t out[32]);
/* DensePolynomial::evaluate(r) (hyrax.rs:217-222) = <Z, eq(r)>; the eq table is built on the device (r: ell scalars, 2^ell == len) */
int sbn_table_evaluate(sbn_ctx* ctx, const sbn_table* Z, const uint8_t* r, size_t ell, uint8_t out[32]);
/* the same for `count` tables of equal length at ONE point: HashLayerProof::prove evaluates 6 derefs + 15 addr/val/ts polynomials at
 * rand_ops and 2 at rand_mem (sparse_mlpoly_full.rs:907-976), each call rebuilding the eq table in the reference; here it is built once.
 * out = count x 32 B */
int sbn_table_evaluate_many(sbn_ctx* ctx, const sbn_table* const* Z, size_t count, const uint8_t* r, size_t ell, uint8_t* out);
/* DensePolynomial::bound(L) (hyrax.rs:311-324), the L*Z of PolyEvalProof::prove (hyrax.rs:101): Z viewed as L_size x R_size,
 * out[i] = sum_j Lvec[j] * Z[j*R_size + i]  (a new table of R_size entries) */
int sbn_table_bound(sbn_ctx* ctx, const sbn_table* Z, const sbn_table* Lvec, sbn_table** out);

/* ---- BulletReductionProof::prove (nizk/bullet.rs:41-126) as a device-resident state; the transcript stays with the caller:
 *      begin, cross (the first round's L, R), then per challenge u: fold_cross(u) -> the next L, R (fold(u) for the last one), then finish.
 * The generators are never folded (bullet.rs:87-91 costs n 254-bit scalar multiplications per round): round j's L and R are
 * MSMs over the ORIGINAL generators with scalars a[..] * s_t, s_t the running product of the u / u_inv the fold would have
 * applied to G_t (the verifier's compute_s, bullet.rs:181-199); g_hat = MSM(s, G).  Same group elements, bit for bit. ----
 * begin: G = the n generators (+ h = H if the handle has one; it must outlive the state), Q_xy = canonical affine Q or NULL
 *   (term left out), a / b = the two vectors (copied, as bullet.rs:50-52 clones them).  If Gamma_xy != NULL it receives
 *   Gamma = MSM(a, G) + <a, b>*Q + blind*H (bullet.rs:58-60; blind NULL = 0). */
typedef struct sbn_bullet sbn_bullet;
int sbn_bullet_begin(sbn_ctx* ctx, const sbn_bases* G, const uint8_t* Q_xy, const sbn_table* a, const sbn_table* b, const uint8_t* blind,
                     uint8_t* Gamma_xy, int* Gamma_is_inf, sbn_bullet** out);
/* The same with Q = q_scale * Q_base: DotProductProofLog::prove (nizk/mod.rs:478-494) passes Q = gens_1.scale(r).G[0] with r fresh from the
 * transcript — a new point per proof over a FIXED base.  Given as (Q_base, q_scale) the derived generator set G || Q_base and its lookup
 * table are built once per generator set, not once per proof; Q_base's column carries c * q_scale.  Same Gamma, L, R, bit for bit. */
int sbn_bullet_begin_scaled(sbn_ctx* ctx, const sbn_bases* G, const uint8_t* Q_base_xy, const uint8_t q_scale[32], const sbn_table* a, const sbn_table* b,
                            const uint8_t* blind, uint8_t* Gamma_xy, int* Gamma_is_inf, sbn_bullet** out);
void sbn_bullet_free(sbn_ctx* ctx, sbn_bullet* st);
size_t sbn_bullet_len(const sbn_bullet* st);       /* current n (halves per fold) */
/* One round's cross terms (bullet.rs:72-78), h = n/2:
 *   c_L = <a[..h], b[h..]>,  c_R = <a[h..], b[..h]>,
 *   L = MSM(a[..h], G[h..]) + c_L*Q + blind_L*H,   R = MSM(a[h..], G[..h]) + c_R*Q + blind_R*H   (blinds: canonical or NULL = 0) */
int sbn_bullet_cross(sbn_ctx* ctx, sbn_bullet* st, const uint8_t* blind_L, const uint8_t* blind_R, uint8_t L_xy[64], int* L_is_inf,
                     uint8_t R_xy[64], int* R_is_inf, uint8_t c_L[32], uint8_t c_R[32]);
/* The folds after the challenge u (bullet.rs:86-106): G <- u_inv*G_L + u*G_R (kept as coefficients), a <- u*a_L + u_inv*a_R,
 * b <- u_inv*b_L + u*b_R; the length halves. */
int sbn_bullet_fold(sbn_ctx* ctx, sbn_bullet* st, const uint8_t u[32], const uint8_t u_inv[32]);
/* The loop body of bullet.rs:63-108 as ONE call per challenge: fold with u (as sbn_bullet_fold), then the cross terms of the NEXT round
 * (as sbn_bullet_cross) on the folded vectors — one launch ahead of the commit, one host wait.  Needs length >= 4 (after the fold at
 * least one more round follows); the last challenge goes to sbn_bullet_fold.  Same L, R, c_L, c_R as the two separate calls. */
int sbn_bullet_fold_cross(sbn_ctx* ctx, sbn_bullet* st, const uint8_t u[32], const uint8_t u_inv[32], const uint8_t* blind_L, const uint8_t* blind_R,
                          uint8_t L_xy[64], int* L_is_inf, uint8_t R_xy[64], int* R_is_inf, uint8_t c_L[32], uint8_t c_R[32]);
/* After the last fold (length 1): a_hat, b_hat, g_hat (bullet.rs:114-120) */
int sbn_bullet_finish(sbn_ctx* ctx, sbn_bullet* st, uint8_t a_hat[32], uint8_t b_hat[32], uint8_t g_hat_xy[64], int* g_hat_is_inf);

/* ---- the Hyrax opening in ONE call: PolyEvalProof::prove (hyrax.rs:65-116) with DotProductProofLog::prove (nizk/mod.rs:439-522) and
 *      BulletReductionProof::prove (nizk/bullet.rs:24-126) inside, the Merlin transcript included ----
 * (L_size, R_size) = 2^sbn_factored_lens(ell), n = R_size, lg n = log2(n).
 *   gens:   R_size + 1 generators with h, as sbn_gens_new(R_size + 1, label) gives them: gens_n = the first R_size, gens_1.G[0] = the last
 *           (DotProductProofGens::new, nizk/mod.rs:412-415).  The derived set and its lookup table are built on the first call and owned by the handle.
 *   Z:      2^ell entries, only read.   blinds: L_size x 32 canonical, or NULL = zeros (hyrax.rs:83-86).   r: ell x 32.   blind_Zr: or NULL = 0.
 *   rnd:    (3 + 2 lg n) x 32 canonical: d, r_delta, r_beta, then blinds_vec as (v1[i], v2[i]) pairs, the caller's RandomTape draws in the
 *           reference's order (nizk/mod.rs:458-468).
 *   out_proof: lg n x 32 compressed L, lg n x 32 compressed R, delta, beta (32 each, compressed), z1, z2 (32 each, canonical).
 *   out_Cx / out_Cy: the commitments C_LZ and C_Zr' (nizk/mod.rs:470-474) as canonical affine points.
 * ell >= 1 (ell == 0 is SBN_EINVAL), ell <= 40; every scalar in is checked canonical; Zr is not checked against <L*Z, R> (the reference does not).
 * Transcript, byte for byte the reference's: protocol-name x 2, Cx, Cy, every entry of a_vec = R as its own "a" message (transcript.rs:46-50),
 * challenge r, per round L, R, challenge u, then delta, beta, challenge c; points in the form sbn_g1_compress gives.
 * Every group element is a two-row commit over the one set G || Q_base with h: lg n + 2 commits, one host wait each; Gamma and g_hat are never
 * formed.  `tr` moves on only if the whole call succeeded.  Same bytes as the loop over sbn_table_bound, sbn_bullet_*, sbn_msm,
 * sbn_g1_compress and sbn_transcript_* with the same draws. */
int sbn_polyeval_prove(sbn_ctx* ctx, const sbn_bases* gens, const sbn_table* Z, const uint8_t* blinds, const uint8_t* r, size_t ell, const uint8_t Zr[32],
                       const uint8_t* blind_Zr, const uint8_t* rnd, sbn_transcript* tr, uint8_t* out_proof,
                       uint8_t out_Cx_xy[64], int* Cx_is_inf, uint8_t out_Cy_xy[64], int* Cy_is_inf);
/* The n-to-1 reduction the three HashLayerProof openings share (DerefsEvalProof::prove_single, sparse_mlpoly_full.rs:384-407; the comb_ops and
 * comb_mem openings, :986-1009, :1013-1035), then sbn_polyeval_prove on the merged table: append `evals` (count a power of two, padded by the
 * caller) under label_evals, challenge_vector(label_chal, log2 count), joint_claim = evals bound from the last challenge down
 * (bound_poly_var_bot, hyrax.rs:206-214), append it under label_claim, open Z (2^(log2 count + ell_r) entries) at challenges || r with no
 * blinds and blind_Zr = 0.  out_challenges: log2 count x 32 (may be NULL for count = 1); rnd, out_proof, out_Cx / out_Cy as above. */
int sbn_joint_opening_prove(sbn_ctx* ctx, const sbn_bases* gens, const sbn_table* Z, const uint8_t* evals, size_t count,
                            const uint8_t* label_evals, size_t label_evals_len, const uint8_t* label_chal, size_t label_chal_len,
                            const uint8_t* label_claim, size_t label_claim_len, const uint8_t* r, size_t ell_r, const uint8_t* rnd, sbn_transcript* tr,
                            uint8_t* out_challenges, uint8_t out_joint_claim[32], uint8_t* out_proof,
                            uint8_t out_Cx_xy[64], int* Cx_is_inf, uint8_t out_Cy_xy[64], int* Cy_is_inf);

/* ---- the Hyrax opening CHECK in one call: PolyEvalProof::verify / verify_plain (hyrax.rs:118-151) with DotProductProofLog::verify
 *      (nizk/mod.rs:525-567) and BulletReductionProof::verify (nizk/bullet.rs:130-173, compute_s :183-200) inside, the transcript included ---- */
/* arkworks deserialize_compressed of n points (group.rs:323-329) on the device, one point per lane; the inverse of sbn_g1_compress.
 * in32: n x 32 (x little-endian; bit 7 of byte 31: y is the larger root, bit 6: the identity).  out_xy: n x 64 canonical affine, the identity
 * all-zero.  out_ok[i] = 0: x >= p, or x^3 + 3 is not a square; out_xy[i] is then all-zero. */
int sbn_g1_decompress(sbn_ctx* ctx, const uint8_t* in32, size_t n, uint8_t* out_xy, uint8_t* out_ok);
/* the same into a resident point set (no h), for a commitment that arrives as bytes (comm_vars, r1csproof.rs:187; comm_derefs,
 * sparse_mlpoly_full.rs:301-304).  A point that does not decompress: SBN_EINVAL, *bad_index (may be NULL) = the first such i, no handle. */
int sbn_bases_from_compressed(sbn_ctx* ctx, const uint8_t* in32, size_t n, sbn_bases** out, size_t* bad_index);
/* (L_size, R_size) = 2^sbn_factored_lens(ell), n = R_size.
 *   gens:    R_size + 1 generators with h, the handle sbn_polyeval_prove takes.   comm: the L_size row commitments of the polynomial
 *            (PolyCommitment.C, hyrax.rs:283-308), no h: sbn_bases_upload or sbn_bases_from_compressed; identity rows are ordinary.
 *   r:       ell x 32.   Exactly one of C_Zr_xy (64 B canonical affine: verify, hyrax.rs:118-137) and Zr (32 B: verify_plain, :139-151) is non-NULL.
 *   proof:   64 lg n + 128 bytes, the out_proof of sbn_polyeval_prove.
 * The return code reports misuse only — SBN_EINVAL before any launch, `tr` unchanged: a NULL pointer, ell == 0 or > 40, sbn_bases_len(comm) !=
 * L_size, gens of another size or without h, both or neither of C_Zr_xy and Zr, a non-canonical r or Zr, a C_Zr_xy that is no point of the curve.
 * What an adversary controls gives SBN_OK with *accepted = 0: a proof point that does not decompress, z1 or z2 >= r, a challenge u = 0, the
 * failed check.  `tr` is advanced exactly as the reference's verifier advances it (protocol-name x 2, Cx, Cy, every entry of R = eq(r_right)
 * as its own "a" message, challenge r, per round L, R, challenge u, then delta, beta, challenge c), and only when *accepted == 1.
 * Two host waits: C_LZ = sum L_i C_i (and Zr * gens_1.G[0]) for the transcript, then the reference's final equation (nizk/mod.rs:560-565)
 * moved to one side — an MSM over the 2 lg n + 4 device points of the proof and ONE one-row commit of -z1 s over the prover's derived set —
 * whose sum must be the identity.  The same group equation, no random batching; no scalar multiplication on the CPU. */
int sbn_polyeval_verify(sbn_ctx* ctx, const sbn_bases* gens, const sbn_bases* comm, const uint8_t* r, size_t ell, const uint8_t* C_Zr_xy, const uint8_t* Zr,
                        const uint8_t* proof, sbn_transcript* tr, int* accepted);
/* The n-to-1 reduction in front of it, the mirror of sbn_joint_opening_prove: DerefsEvalProof::verify_single (sparse_mlpoly_full.rs:434-457) and its
 * two siblings in HashLayerProof::verify.  Append `evals`, challenge_vector, joint_claim = evals bound from the last challenge down, append it,
 * then verify_plain at challenges || r with Zr = joint_claim.  out_challenges: log2 count x 32, written whenever the call returns SBN_OK (may be
 * NULL).  Misuse as above, and a count that is no power of two or non-canonical evals. */
int sbn_joint_opening_verify(sbn_ctx* ctx, const sbn_bases* gens, const sbn_bases* comm, const uint8_t* evals, size_t count,
                             const uint8_t* label_evals, size_t label_evals_len, const uint8_t* label_chal, size_t label_chal_len,
                             const uint8_t* label_claim, size_t label_claim_len, const uint8_t* r, size_t ell_r,
                             const uint8_t* proof, sbn_transcript* tr, uint8_t* out_challenges, int* accepted);

/* ---- the two ZK sumchecks of R1CSProof::prove (r1csproof.rs:295, :394) in ONE call each: ZKSumcheckInstanceProof::
 *      prove_cubic_with_additive_term (sumcheck.rs:465-649) and ::prove_quad (sumcheck.rs:657-811), with UniPoly::from_evals, the four
 *      commitments of a round and DotProductProof::prove (nizk/mod.rs:306-366) inside, the Merlin transcript included ----
 * num_rounds = log2 of the tables' length; n = the coefficient count of a round polynomial: 4 (r1cs), 3 (quad).
 *   tables:  equal length, a power of two >= 2, distinct handles.  They are bound IN PLACE, as sbn_sc_bind_eval_* / sbn_bind_top do, and end with
 *            length 1; out_finals = their [0] in argument order (sumcheck.rs:646, :808), canonical.
 *   gens_1:  one generator with h.   gens_4 / gens_3: n generators with h.  The two h may differ (R1CSSumcheckGens::new clones gens_pc's gens_1
 *            and derives gens_3 / gens_4 from its label): no shared h is assumed.  The derived set gens_n.G || gens_n.h || gens_1.G[0] || gens_1.h
 *            and its lookup table are built on the first call with a (gens_1, gens_n) pair and owned by the gens_n handle.
 *   rnd:     num_rounds * (n + 4) x 32 canonical, the caller's RandomTape draws in the reference's order: blinds_poly[num_rounds],
 *            blinds_evals[num_rounds], then per round d_vec[n], r_delta, r_beta (nizk/mod.rs:326-328).
 *   out_proof: num_rounds x (6 + n) x 32, round-major: comm_poly, comm_eval, delta, beta (compressed as sbn_g1_compress gives them), then
 *            z[n], z_delta, z_beta (canonical).   out_r: num_rounds x 32.   out_blind = blinds_evals[num_rounds - 1].
 * Transcript, byte for byte the reference's, per round: comm_poly, challenge_scalar("challenge_nextround"), comm_claim_per_round, comm_eval,
 * challenge_vector("combine_two_claims_to_one", 2), protocol-name "dot product proof", Cx (= comm_poly, computed once), Cy, every entry of a as its
 * own "a" message, delta, beta, challenge_scalar("c").
 * Every group element is a row of a two-row commit over the derived set: three commits a round ({comm_poly, delta}, {comm_eval [, comm_claim]},
 * {Cy, beta}), the first queued behind the round kernel with no host wait in between; no scalar multiplication runs on the CPU.
 * SBN_EINVAL: a null pointer, unequal / non-power-of-two / < 2 lengths, a table passed twice, a generator handle of the wrong size or without h, any
 * scalar in (claim, blind_claim, rnd) not canonical — nothing has been launched then: tables and `tr` are unchanged.  `tr` moves on only if the
 * whole call succeeded; a failure after the first launch leaves the tables partly bound.  Same bytes as the round loop over sbn_sc_eval_*,
 * sbn_sc_bind_eval_*, sbn_bind_top, sbn_unipoly_from_evals, one-row sbn_commit_rows and sbn_transcript_* with the same draws. */
int sbn_zk_sumcheck_prove_r1cs(sbn_ctx* ctx, sbn_table* tau, sbn_table* Az, sbn_table* Bz, sbn_table* Cz,
                               const sbn_bases* gens_1, const sbn_bases* gens_4,
                               const uint8_t claim[32], const uint8_t blind_claim[32], const uint8_t* rnd, sbn_transcript* tr,
                               uint8_t* out_proof, uint8_t* out_r, uint8_t out_finals[128], uint8_t out_blind[32]);
int sbn_zk_sumcheck_prove_quad(sbn_ctx* ctx, sbn_table* Z, sbn_table* ABC,
                               const sbn_bases* gens_1, const sbn_bases* gens_3,
                               const uint8_t claim[32], const uint8_t blind_claim[32], const uint8_t* rnd, sbn_transcript* tr,
                               uint8_t* out_proof, uint8_t* out_r, uint8_t out_finals[64], uint8_t out_blind[32]);

/* ---- network construction pieces ----
 * sbn_hash_layer and sbn_product_layer only enqueue work (their outputs are consumed by later calls on the same context, which
 * are ordered behind them); every call that returns data to the host waits for it. ----
 * Layers::build_hash_layer (sparse_mlpoly_full.rs:745-796): out[j] = (ts[j] + ts_add) * r_hash^2 + val[j] * r_hash + addr[j] - r_multiset
 * addr_dev / ts_dev: DEVICE arrays of n uint32 (NULL addr = the cell index j, as for poly_init/audit_hashed; NULL ts = zeros);
 * ts_add = 1 gives the write set (read_ts + 1).  val: table of n entries (eval_table or a derefs poly). */
int sbn_hash_layer(sbn_ctx* ctx, const void* addr_dev, const sbn_table* val, const void* ts_dev, uint32_t ts_add,
                   const uint8_t r_hash[32], const uint8_t r_multiset[32], sbn_table** out);
/* Two hashed sets over the same (addr, val) in one pass: the read and write sets of one sparse polynomial (ts_a = ts_b = read_ts, adds 0 and 1) or
 * the init and audit sets of a memory (addr NULL, ts_a NULL, ts_b = audit_ts) — sparse_mlpoly_full.rs:762-790 builds each pair from the same inputs.
 * out_a / out_b = what two sbn_hash_layer calls with (ts_a, ts_a_add) / (ts_b, ts_b_add) return. */
int sbn_hash_layer_pair(sbn_ctx* ctx, const void* addr_dev, const sbn_table* val, const void* ts_a_dev, uint32_t ts_a_add, const void* ts_b_dev, uint32_t ts_b_add,
                        const uint8_t r_hash[32], const uint8_t r_multiset[32], sbn_table** out_a, sbn_table** out_b);
/* The same pair AND the first layer of both product circuits (ProductCircuit::compute_layer, product_tree.rs:21-37) in one pass: a hashed set is
 * otherwise written by this call and read back at once by the first sbn_product_layer.  out_a / out_b as sbn_hash_layer_pair gives them (the
 * sumcheck needs layer 0); prod_a[i] = out_a[i] * out_a[i + n/2], prod_b likewise: what sbn_product_layer(out_a) / (out_b) return, n/2 entries.
 * n = sbn_table_len(val) must be a power of two >= 2, else SBN_EINVAL.  Enqueued only. */
int sbn_hash_layer_pair_product(sbn_ctx* ctx, const void* addr_dev, const sbn_table* val, const void* ts_a_dev, uint32_t ts_a_add, const void* ts_b_dev, uint32_t ts_b_add,
                                const uint8_t r_hash[32], const uint8_t r_multiset[32], sbn_table** out_a, sbn_table** out_b, sbn_table** prod_a, sbn_table** prod_b);
/* ProductCircuit::compute_layer (product_tree.rs:21-37): the next layer's full vector out[i] = in[i] * in[i + len/2] */
int sbn_product_layer(sbn_ctx* ctx, const sbn_table* in, sbn_table** out);
/* ProductCircuit::new (product_tree.rs:39-57): every layer above `in` in one call — layers[0] = compute_layer(in) (len/2 entries),
 * layers[k] = compute_layer(layers[k-1]), down to the single-entry layer whose value is the circuit's product (evaluate(), :59-66).
 * cap = size of the caller's array (log2(len) layers are produced), *count <- number written.  Enqueued only, like sbn_product_layer. */
int sbn_product_circuit(sbn_ctx* ctx, const sbn_table* in, sbn_table** layers, size_t cap, size_t* count);
/* n product circuits over tables of ONE length, built together: layers[i * cap + k] = layer k of circuit i, *count <- layers per circuit.
 * The hashed sets of a sparse-polynomial evaluation proof all get their circuit at the same point (sparse_mlpoly_full.rs:813-823: row / col x
 * read / write over the operations, init / audit over the memories); one launch per layer serves all of them — below ~2^15 entries a layer's
 * launch costs more than its arithmetic.  Same values as n sbn_product_circuit calls. */
int sbn_product_circuit_many(sbn_ctx* ctx, const sbn_table* const* ins, size_t n, sbn_table** layers, size_t cap, size_t* count);
/* DensePolynomial::split(len/2) (hyrax.rs:186-192) as views: left = first half, right = second half of `t` (the A and B tables of
 * a product-circuit layer).  Views share t's memory and must be freed before t. */
int sbn_table_halves(sbn_ctx* ctx, const sbn_table* t, sbn_table** left, sbn_table** right);

/* entries [first, first + len) of t as a view (len a power of two; freed before t): the polynomials DensePolynomial::merge laid end to end
 * (hyrax.rs:237-247) are slices of the merged table — e.g. Derefs' row_ops_val / col_ops_val inside `comb` (sparse_mlpoly_full.rs:286-297),
 * which Layers::new hashes again (sparse_mlpoly_full.rs:745-796) */
int sbn_table_slice(sbn_ctx* ctx, const sbn_table* t, size_t first, size_t len, sbn_table** out);

/* ---- derefs on the device ----
 * MultiSparseMatPolynomialAsDense::deref -> AddrTimestamps::deref_mem (sparse_mlpoly_full.rs:245-257, 275-279) followed by
 * Derefs::new -> DensePolynomial::merge (sparse_mlpoly_full.rs:293-297, hyrax.rs:237-247):
 *   out = concat_k [ mem[k][addr[k][i]] for i < n ], zero-padded to the next power of two.
 * mem[k]: the table instance k reads (the eq(rx) table for the row_ops_val polys, eq(ry) for col_ops_val: build them with
 * sbn_eq_evals).  addr[k]: DEVICE arrays of n uint32 cell indices (fixed per circuit: upload once with sbn_dev_upload).
 * The result is a table (the `comb` polynomial), ready for sbn_commit_table — the 1 GiB scalar matrix of the keyless
 * derefs commitment never crosses PCIe. */
int sbn_gather_merge(sbn_ctx* ctx, const sbn_table* const* mem, const void* const* addr_dev, size_t count, size_t n, sbn_table** out);
/* One device's share of the same polynomial when its L x R view (R a power of two, hyrax.rs:371-373) is committed by interleaved rows over
 * several devices: only the rows row0, row0 + rstep, ... (nrows of them) are gathered, as one table of nrows x R entries for
 * sbn_commit_table(…, L = nrows, R).  row0 = 0, rstep = 1, nrows = L gives sbn_gather_merge's table. */
int sbn_gather_merge_rows(sbn_ctx* ctx, const sbn_table* const* mem, const void* const* addr_dev, size_t count, size_t n, size_t R,
                          size_t row0, size_t rstep, size_t nrows, sbn_table** out);
/* DensePolynomial::commit (hyrax.rs:283-308) of a device-resident table viewed as L x R (L*R == len, R == gens n); blinds as
 * in sbn_commit_rows (host pointer or NULL) */
int sbn_commit_table(sbn_ctx* ctx, const sbn_bases* b, const sbn_table* t, const uint8_t* blinds, size_t L, size_t R,
                     uint8_t* out_xy, uint8_t* out_inf);

/* ---- device groups: ONE host process, several GPUs behind one call ----
 * The reference parallelises inside one process (rayon over the rows of the Hyrax matrix, hyrax.rs:259-261; arkworks over the windows of
 * an MSM), so its drop-in has one process too: a group owns one context per listed device (a device may be listed more than once) and
 * runs every call with one (persistent) host thread per device.  Nothing here needs a launcher or a collective library.
 *   rows of ONE matrix: row i on device i mod N, no exchange (rows are independent);
 *   ONE MSM: contiguous base-point ranges, the N 64-byte partial sums folded on the host with sbn_g1_sum (group.rs:199-262). */
typedef struct sbn_group sbn_group;
typedef struct sbn_group_bases sbn_group_bases;
int sbn_group_create(const int* devices, size_t n, sbn_group** out);
void sbn_group_destroy(sbn_group* g);
size_t sbn_group_size(const sbn_group* g);
sbn_ctx* sbn_group_ctx(sbn_group* g, size_t i);                 /* the i-th device's context (for the single-device calls above) */
const char* sbn_group_last_error(const sbn_group* g);
/* MultiCommitGens (commitments.rs:17-27) replicated on every device of the group */
int sbn_group_bases_upload(sbn_group* g, const uint8_t* G_xy, size_t n, const uint8_t* h_xy, uint32_t flags, sbn_group_bases** out);
int sbn_group_gens_new(sbn_group* g, size_t n, const uint8_t* label, size_t label_len, uint8_t* out_xy, sbn_group_bases** out);
int sbn_group_bases_precompute(sbn_group* g, sbn_group_bases* gb, size_t max_bytes_per_device, int* window_bits);
void sbn_group_bases_free(sbn_group* g, sbn_group_bases* gb);
/* DensePolynomial::commit -> commit_inner (hyrax.rs:253-267) of ONE L x R matrix (host pointer) over the group; arguments as sbn_commit_rows */
int sbn_group_commit_rows(sbn_group* g, const sbn_group_bases* gb, const uint8_t* Z, const uint8_t* blinds, size_t L, size_t R,
                          uint32_t flags, uint8_t* out_xy, uint8_t* out_inf);
/* The same with the matrix already ON the devices: Z_dev[d] = device pointer on device d to ITS rows (d, d + N, d + 2N, ... in this order,
 * contiguous, R x 32 B each); blinds_dev[d] likewise (32 B per row) or blinds_dev == NULL.  Only the L x 64 B of results cross PCIe. */
int sbn_group_commit_rows_dev(sbn_group* g, const sbn_group_bases* gb, const void* const* Z_dev, const void* const* blinds_dev, size_t L, size_t R,
                              uint32_t flags, uint8_t* out_xy, uint8_t* out_inf);
/* Derefs::commit (sparse_mlpoly_full.rs:301-304) over the group from device-resident inputs: deref_mem + merge (sparse_mlpoly_full.rs:245-257,
 * 293-297) and commit_inner (hyrax.rs:253-267) in one call.  mem[d * count + k] / addr_dev[d * count + k]: table k (the eq(rx) / eq(ry) tables,
 * built per device with sbn_eq_evals on sbn_group_ctx(g, d)) and its n uint32 cell addresses ON device d.  Device d gathers and commits only
 * the rows d, d + N, ... of the L x R view of the merged polynomial (L * R = next power of two of count * n); no blinds. */
int sbn_group_gather_commit(sbn_group* g, const sbn_group_bases* gb, const sbn_table* const* mem, const void* const* addr_dev, size_t count, size_t n,
                            size_t L, size_t R, uint8_t* out_xy, uint8_t* out_inf);
/* GroupElement::msm_affine (group.rs:171-175) of ONE MSM over the group: device d takes the pairs [d n / N, (d+1) n / N) */
int sbn_group_msm(sbn_group* g, const uint8_t* scalars, const uint8_t* points, size_t n, uint32_t flags, uint8_t out_xy[64], int* out_is_inf);
/* the same with resident points: cut once into the per-device ranges (no h), then only scalars travel */
int sbn_group_bases_upload_ranges(sbn_group* g, const uint8_t* G_xy, size_t n, uint32_t flags, sbn_group_bases** out);
int sbn_group_bases_synthetic_ranges(sbn_group* g, size_t n, const uint8_t s0[32], const uint8_t d[32], sbn_group_bases** out);   /* sbn_bases_synthetic, range by range */
void sbn_group_range(const sbn_group_bases* gb, size_t device, size_t* lo, size_t* hi);
int sbn_group_msm_bases(sbn_group* g, const sbn_group_bases* gb, const uint8_t* scalars, size_t n, uint32_t flags, uint8_t out_xy[64], int* out_is_inf);
/* scalars_dev[d]: device pointer ON device d to the (hi - lo) x 32 B of its range */
int sbn_group_msm_bases_dev(sbn_group* g, const sbn_group_bases* gb, const void* const* scalars_dev, uint32_t flags, uint8_t out_xy[64], int* out_is_inf);

/* ---- KZG mode (--features kzg): commitments and openings over a resident SRS (kzg.rs) ----
 * The SRS is an sbn_bases handle (no h; sbn_bases_free / _len / _download work on it).  A polynomial is the first n entries of a
 * table, coefficients low to high; n <= the table's length, entries from n on are never read.  z, gamma, tau: canonical (< r).
 * The transcript stays with the caller; the pairing checks of these openings are sbn_kzg_verify / sbn_kzg_verify_batched below. */
/* KZGSrs.powers_g1 (kzg.rs:25-31): n canonical affine points (SBN_POINTS_MONT: ark-ff limbs); no duplicate detection */
int sbn_kzg_srs_upload(sbn_ctx* ctx, const uint8_t* powers_xy, size_t n, uint32_t flags, sbn_bases** out);
/* [tau^i]G1 for i < n (kzg.rs:37-56 with tau supplied), built on the device; tau non-zero, n >= 1 */
int sbn_kzg_srs_from_tau(sbn_ctx* ctx, const uint8_t tau[32], size_t n, sbn_bases** out);
/* KZGPolyCommitment::commit (kzg.rs:386-395): MSM of the first min(n, srs len) coefficients; n = 0 gives the identity */
int sbn_kzg_commit(sbn_ctx* ctx, const sbn_bases* srs, const sbn_table* t, size_t n, uint8_t out_xy[64], int* out_is_inf);
/* evaluate_poly + compute_quotient (kzg.rs:220-260): eval = p(z), *q = (p - p(z)) / (X - z) as a new table of the n - 1 quotient
 * coefficients zero-padded to a power of two (*q = NULL when n <= 1; n = 0 gives eval 0) */
int sbn_poly_div_linear(sbn_ctx* ctx, const sbn_table* t, size_t n, const uint8_t z[32], uint8_t eval[32], sbn_table** q);
/* KZGProof::prove (kzg.rs:174-192): eval = p(z), proof = MSM of the quotient over srs[0..n-1) (identity for n <= 1);
 * n - 1 > srs len is SBN_EINVAL (the reference panics on the slice) */
int sbn_kzg_open(sbn_ctx* ctx, const sbn_bases* srs, const sbn_table* t, size_t n, const uint8_t z[32],
                 uint8_t eval[32], uint8_t proof_xy[64], int* proof_is_inf);
/* KZGBatchedEvalProof::prove -> KZGBatchProof::batch_prove (kzg.rs:478-500, 268-312): evals[k] = p_k(z) (count x 32 B); the proof opens
 * sum_k gamma^k p_k over max(ns) coefficients at z.  gamma comes from the caller's transcript (any canonical value, zero included);
 * count = 0 gives the identity and no evals */
int sbn_kzg_open_batched(sbn_ctx* ctx, const sbn_bases* srs, const sbn_table* const* ts, const size_t* ns, size_t count,
                         const uint8_t z[32], const uint8_t gamma[32], uint8_t* evals, uint8_t proof_xy[64], int* proof_is_inf);

/* ---- the R1CS matrices on the device: R1CSShape (r1cs.rs:22-82) uploaded once per circuit ----
 * A, B, C as (row, col, val) triplets, mats[0..3) = A, B, C; num_cons and num_vars powers of two.  Columns index
 * z = (vars, 1, inputs, 0 ...) of 2 * num_vars entries (r1csproof.rs:268-277).  Entries in any order, duplicates allowed (they add).
 * row >= num_cons is SBN_EINVAL; col >= 2 * num_vars is dropped (all three reference loops skip it); a val >= r is SBN_EINVAL;
 * SBN_SCALARS_MONT: vals are ark-ff limbs.  A matrix with nnz = 0 is valid (zero tables, zero evaluations); its arrays may be NULL.
 * Outputs are ordinary tables that feed sbn_sc_eval_r1cs / sbn_sc_eval_quad and their bind variants directly. */
typedef struct sbn_r1cs sbn_r1cs;
int sbn_r1cs_upload(sbn_ctx* ctx, size_t num_cons, size_t num_vars, const uint32_t* const* rows, const uint32_t* const* cols,
                    const uint8_t* const* vals, const size_t* nnz, uint32_t flags, sbn_r1cs** out);
void sbn_r1cs_free(sbn_ctx* ctx, sbn_r1cs* m);
/* R1CSShape::multiply_vec (r1cs.rs:132-146): z has 2 * num_vars entries; Az, Bz, Cz: three new tables of num_cons entries */
int sbn_r1cs_multiply(sbn_ctx* ctx, const sbn_r1cs* m, const sbn_table* z, sbn_table** Az, sbn_table** Bz, sbn_table** Cz);
/* evals_ABC of r1csproof.rs:376-387: r_A*evals_A + r_B*evals_B + r_C*evals_C with evals_M = compute_eval_table_sparse(eq(rx))
 * (r1cs.rs:148-163); rx: ell_x = log2(num_cons) canonical scalars (the eq table is built inside the call); a new table of 2 * num_vars entries */
int sbn_r1cs_eval_table(sbn_ctx* ctx, const sbn_r1cs* m, const uint8_t* rx, size_t ell_x, const uint8_t rA[32], const uint8_t rB[32],
                        const uint8_t rC[32], sbn_table** out);
/* R1CSShape::evaluate (r1cs.rs:126-129; snark.rs:465 "Instance evaluations"): out = A(rx,ry) || B(rx,ry) || C(rx,ry), canonical;
 * ell_x = log2(num_cons), ell_y = log2(2 * num_vars) */
int sbn_r1cs_evaluate(sbn_ctx* ctx, const sbn_r1cs* m, const uint8_t* rx, size_t ell_x, const uint8_t* ry, size_t ell_y, uint8_t out[96]);

/* ---- R1CSProof::prove (r1csproof.rs:241-459) in ONE call: the witness commitment, both ZK sumchecks, the three Σ-protocols between them
 * (KnowledgeProof, ProductProof, EqualityProof::prove, nizk/mod.rs:34-59, :167-227, :96-124), the Hyrax opening and every transcript line ----
 * Notation: nx = log2(num_cons), ell = log2(num_vars), ny = ell + 1, (L, R) = 2^sbn_factored_lens(ell), lg = log2(R).
 *   inst     its num_cons and num_vars (both >= 2) define the shape.
 *   vars     a table of num_vars entries; only read, never bound.
 *   input    num_inputs x 32 B canonical scalars (NULL with num_inputs == 0); num_inputs < num_vars (r1csproof.rs:253).
 *   gens_pc  R + 1 generators with h, the handle sbn_polyeval_prove takes (sbn_gens_new(R + 1, label)): gens_n = the first R with h,
 *            gens_1 = (G[R], h).  Both are derived inside the call on first use, owned by gens_pc and freed with it.  There is no gens_1
 *            parameter: R1CSGens::new (r1csproof.rs:177-182) makes gens_sc.gens_1 a clone of gens_pc.gens.gens_1.
 *   gens_3, gens_4   3 and 4 generators with h (R1CSSumcheckGens::new), as the ZK sumcheck calls take them.
 *   rnd      the RandomTape draws, canonical, in the reference's order:
 *              poly_blinds [L] | phase 1 [8 nx, as sbn_zk_sumcheck_prove_r1cs] | Az_blind, Bz_blind, Cz_blind, prod_Az_Bz_blind | t1, t2 |
 *              b1 .. b5 | r of the first equality proof | phase 2 [7 ny, as sbn_zk_sumcheck_prove_quad] | blind_eval |
 *              the opening [3 + 2 lg, as sbn_polyeval_prove] | r of the second equality proof
 *            L + 8 nx + 7 ny + 2 lg + 17 scalars.
 *   out_proof  the fields of R1CSProof in declaration order (r1csproof.rs:187-202), points as sbn_g1_compress gives them, scalars canonical:
 *              comm_vars [L x 32] | sc_proof_phase1 [nx x 10 x 32, layout of sbn_zk_sumcheck_prove_r1cs] |
 *              comm_Az_claim, comm_Bz_claim, comm_Cz_claim, comm_prod_Az_Bz_claims [4 x 32] |
 *              pok_claims_phase2 [11 x 32: knowledge proof alpha, z1, z2; product proof alpha, beta, delta, z[5]] |
 *              proof_eq_sc_phase1 [alpha, z] | sc_proof_phase2 [ny x 9 x 32, layout of sbn_zk_sumcheck_prove_quad] | comm_vars_at_ry [32] |
 *              proof_eval_vars_at_ry [64 lg + 128, out_proof of sbn_polyeval_prove] | proof_eq_sc_phase2 [alpha, z]
 *              32 (L + 10 nx + 9 ny + 20) + 64 lg + 128 bytes.
 *   out_rx   nx x 32 B;  out_ry  ny x 32 B.
 * `tr` is advanced exactly as the reference advances its transcript, and only when the call returns SBN_OK.  A refusal (a wrong length, a
 * shape below 2, num_inputs >= num_vars, a generator set of the wrong size or without h, a scalar >= r) is SBN_EINVAL before any launch. */
/* host only: the sizes of rnd (in scalars) and out_proof (in bytes) of a shape; SBN_EINVAL for a shape the call refuses */
int sbn_r1cs_proof_sizes(size_t num_cons, size_t num_vars, size_t* rnd_scalars, size_t* proof_bytes);
int sbn_r1cs_proof_prove(sbn_ctx* ctx, const sbn_r1cs* inst, const sbn_table* vars, const uint8_t* input, size_t num_inputs,
                         const sbn_bases* gens_pc, const sbn_bases* gens_3, const sbn_bases* gens_4, const uint8_t* rnd, sbn_transcript* tr,
                         uint8_t* out_proof, uint8_t* out_rx, uint8_t* out_ry);

/* ---- the CHECK of that proof in one call: R1CSProof::verify (r1csproof.rs:463-619) and, on its own, ZKSumcheckInstanceProof::verify
 *      (sumcheck.rs:366-457) with DotProductProof::verify (nizk/mod.rs:368-400) inside, the Merlin transcript included ----
 * No fresh point is multiplied: every point of a check is a point of the proof or a generator and every coefficient a scalar the host derives
 * from the transcript (c * Cy_i = (c w0) P_{i-1} + (c w1) comm_eval_i), so every check is a sum of entries of one table T[p][k] = 2^k P_p,
 * selected by scalar bits.  Per call: ONE decompress launch over all the proof's points, ONE table launch over them and the generators, one
 * sum launch and one host wait for each point whose bytes the transcript needs, and ONE last launch for every equation, each moved to one
 * side, answered as packed "the sum is the identity" bits.  The same group equations, no random batching; no scalar multiplication and no
 * point addition on the CPU.
 * Both calls follow the contract of sbn_polyeval_verify.  The return code reports misuse only — SBN_EINVAL before any launch, `tr` unchanged.
 * What an adversary controls gives SBN_OK with *accepted = 0: a point that does not decompress, a scalar of the proof >= r, any failed
 * check.  `tr` is advanced exactly as the reference's verifier advances it, and only when *accepted == 1; the out_ arrays are written only then.
 *
 * sbn_zk_sumcheck_verify:  gens_1: one generator with h; gens_n: degree_bound + 1 generators with h; comm_claim_xy: canonical affine (all-zero:
 *   the identity); proof: num_rounds x (6 + n) x 32 with n = degree_bound + 1, the out_proof of sbn_zk_sumcheck_prove_r1cs (3) / _quad (2).
 *   out_r: num_rounds x 32; out_comm_eval_xy: comm_evals[num_rounds - 1] (sumcheck.rs:456), canonical affine.  num_rounds + 1 sum launches.
 *   Misuse: a NULL pointer, num_rounds == 0 or > 64, degree_bound outside {2, 3}, a generator handle of the wrong size or without h, a
 *   comm_claim_xy that is no canonical point of the curve. */
int sbn_zk_sumcheck_verify(sbn_ctx* ctx, const sbn_bases* gens_1, const sbn_bases* gens_n, const uint8_t comm_claim_xy[64],
                           size_t num_rounds, size_t degree_bound, const uint8_t* proof, sbn_transcript* tr,
                           uint8_t* out_r, uint8_t out_comm_eval_xy[64], int* accepted);
/* sbn_r1cs_proof_verify:  shape, input, gens_pc, gens_3, gens_4 as sbn_r1cs_proof_prove takes them; proof: its out_proof (sbn_r1cs_proof_sizes).
 *   evals = A(rx, ry) || B(rx, ry) || C(rx, ry), canonical: the caller's, as in the reference (r1csproof.rs:469) — sbn_r1cs_evaluate after a
 *   first pass, or the proof's inst_evals; it enters the last equality check only (:603-605).
 *   In the reference's order: both sumcheck checks, KnowledgeProof / ProductProof / EqualityProof::verify (nizk/mod.rs:61-81, :243-283, :126-149),
 *   the opening of comm_vars at ry[1..] (the body of sbn_polyeval_verify on a handle made of the proof's bytes, as sbn_bases_from_compressed
 *   makes one: its own two waits), poly_input_eval (:580-594).  nx + ny + 3 sum launches with a wait each (Cy of every round, phase 2's
 *   comm_claim, the two `expected` points) and one for the 2 (nx + ny) + 6 equations.
 *   Misuse: a NULL pointer (input may be NULL with num_inputs == 0), a shape below 2 or no power of two, num_inputs >= num_vars, a generator
 *   handle of the wrong size or without h, a non-canonical input or evals. */
int sbn_r1cs_proof_verify(sbn_ctx* ctx, size_t num_cons, size_t num_vars, const uint8_t* input, size_t num_inputs, const uint8_t evals[96],
                          const sbn_bases* gens_pc, const sbn_bases* gens_3, const sbn_bases* gens_4, const uint8_t* proof,
                          sbn_transcript* tr, uint8_t* out_rx, uint8_t* out_ry, int* accepted);

/* ---- many short sums of fresh points in ONE launch: what a verifier's equations over a handful of proof points are in the reference,
 *      GroupElement::vartime_multiscalar_mul (group.rs:143-158) over 2 lg n + 4 points in DotProductProofLog::verify (nizk/mod.rs:560-565) and
 *      over 2 .. 8 in DotProductProof / EqualityProof::verify (nizk/mod.rs:389-394, :141-146) ----
 * Sum i = sum_j scalars[j] * points[j] over the next counts[i] entries of the two arrays (counts[i] <= 64, nsums <= 256; a count of 0: the
 * identity).  points_xy: canonical affine x || y as sbn_msm takes them, all-zero = the identity.  scalars: canonical.  out_xy: nsums x 64 canonical
 * affine, all-zero for the identity; out_is_inf: nsums flags, may be NULL.
 * No table of multiples and no bucket pipeline: the scalars are cut into 64 windows of 4 bits, one block per (sum, window) adds digit * P over
 * the sum's terms (each lane one bit of one digit: at most three doublings), whatever nsums in ONE launch; one upload in front of it, one
 * hand-over behind it, and the host folds each sum's 64 window sums (252 doublings), as it folds the bucket pipeline's.  Repeated points, P and
 * -P and identity inputs take the degenerate branches of the ordinary addition.
 * Host work, on the calling thread and outside the context's mutex (other threads' calls on the context run meanwhile): per term the curve check and
 * two Montgomery conversions, per sum the fold and one inversion, about 70 us a sum of 64 terms: 18 of the 20 ms of a call
 * at the cap.  A caller with hundreds of sums spreads them over threads, a few dozen sums a call.
 * SBN_EINVAL before any launch: a NULL pointer with nsums > 0, counts[i] > 64, nsums > 256, a scalar >= r, a point that is not on the curve or
 * not canonical.  nsums == 0 is SBN_OK and touches nothing. */
int sbn_g1_small_sums(sbn_ctx* ctx, const uint8_t* points_xy, const uint8_t* scalars, const uint32_t* counts, size_t nsums,
                      uint8_t* out_xy, uint8_t* out_is_inf);

/* ---- the sparse polynomial evaluation proof's CHECK in one call, the Hyrax build: SparseMatPolyEvalProof::verify (sparse_mlpoly_full.rs:1815-1845; what
 *      R1CSEvalProof::verify wraps, r1cs.rs:465-490) with PolyEvalNetworkProof::verify (:1581-1650), ProductLayerProof::verify (:1436-1520), both
 *      ProductCircuitEvalProofBatched::verify (product_tree.rs:394-537), HashLayerProof::verify (:1048-1265), the three joint openings and the
 *      Merlin transcript inside.  With sbn_r1cs_proof_verify it is the whole of SNARK::verify.  The KZG build's derefs opening is a pairing check:
 *      sbn_sparse_eval_verify_kzg below is the KZG build's whole check. ----
 *   shape:   num_vars_x, num_vars_y, num_ops (N), batch as sbn_sparse_eval_prove's dense handle has them; num_cells = 2^max(num_vars_x, num_vars_y).
 *   proof:   exactly the out_proof of sbn_sparse_eval_prove (sbn_sparse_eval_sizes gives its length).
 *   comm_ops / comm_mem: the row commitments of comb_ops / comb_mem (the computation commitment, :176-193) as point sets without h, 2^(ell/2) points
 *            each with ell = log2 N + log2 next_pow2(5 batch) and log2 num_cells + 1: sbn_bases_upload or sbn_bases_from_compressed; resident across proofs.
 *   gens_*:  the handles the prover's call takes.   rx, ry, evals: num_vars_x, num_vars_y, batch x 32, canonical.
 * Work: ONE k_g1_decompress launch over every point of the proof before any hashing (comm_derefs lands in table layout and is read where it lies: no
 * handle is built); the field checks and the transcript on the host; per opening (derefs, ops, mem) the n-to-1 reduction on the host, eq(r), C_LZ as
 * an MSM over the commitment's device points and Zr * G as a one-term k_window_sums launch, one hand-over and one wait, then the opening's transcript
 * lines.  The three final equations (nizk/mod.rs:560-565, each moved to one side) feed no transcript: their row commits are queued behind the next
 * opening's hand-over, their sums over the 2 lg n + 4 proof points go through ONE k_window_sums launch, and one last hand-over brings everything.
 * Four host waits a call; each equation is tested for the identity on its own, no random batching.
 * The return code reports misuse only — SBN_EINVAL before any launch, `tr` unchanged: a NULL pointer, batch outside 1 .. 4, N below 2 or no power of
 * two, num_cells != 2^max(num_vars_x, num_vars_y), a commitment or generator handle of the wrong size (or generators without h), a non-canonical rx,
 * ry or evals.  What the prover controls gives SBN_OK with *accepted = 0: a scalar of the proof >= r, a point that does not decompress, a failed
 * sumcheck round, layer check, subset or hash check, eval_dotp_left + eval_dotp_right != evals[i], a challenge u = 0, a failed equation.  `tr`
 * moves on only behind *accepted == 1 and then ends where the prover's transcript ended; behind a refusal nothing stays queued. */
int sbn_sparse_eval_verify(sbn_ctx* ctx, size_t num_vars_x, size_t num_vars_y, size_t num_ops, size_t num_cells, size_t batch,
                           const sbn_bases* comm_ops, const sbn_bases* comm_mem, const uint8_t* rx, const uint8_t* ry, const uint8_t* evals,
                           const sbn_bases* gens_ops, const sbn_bases* gens_mem, const sbn_bases* gens_derefs,
                           const uint8_t* proof, sbn_transcript* tr, int* accepted);

/* ---- MultiSparseMatPolynomialAsDense on the device: what SNARK::encode -> R1CSShape::commit (r1cs.rs:375-400) builds once per circuit ----
 * SparseMatPolynomial::multi_sparse_to_dense_rep -> AddrTimestamps::new (sparse_mlpoly_full.rs:89-101, 120-174, 211-243), from the same
 * (row, col, val) triplets sbn_r1cs_upload takes, in the caller's entry order.  `batch` matrices (1 .. 8; the reference uses 3), nnz[k] entries each.
 *   N     = max_k next_power_of_two(nnz[k]), with next_power_of_two(0) = 1;   cells = 2^max(num_vars_x, num_vars_y) (:145-149).
 *   per matrix k (sparse_to_dense_vecs, :89-101): ops_row[k][i], ops_col[k][i], val[k][i] = entry i for i < nnz[k], zeros from nnz[k] to N.
 *     Nothing is merged, dropped or reordered: duplicates, zero values and the padding are ops like any other (the padding reads cell 0).
 *   per side (rows, then columns, independently; :211-243), ONE audit_ts running across the batch:
 *     read_ts[k][i] = the number of ops (k', i') before (k, i) in (k, i) lexicographic order with the same address,
 *     audit_ts[a]   = the number of ops on a over the whole batch.
 *   comb_ops = merge(row addr[0..batch) || row read_ts[..] || col addr[..] || col read_ts[..] || val[..]) (:154-162): polynomial j of group g
 *     (g = 0 .. 4 in this order) is the slice [(g * batch + j) * N, + N); the 5 * batch * N entries are zero-padded to the next power of two
 *     (hyrax.rs:237-251); integers enter as Scalar::from_u64.
 *   comb_mem = row audit_ts || col audit_ts (:163-164): 2 * cells entries, the column side from entry `cells`.
 * Errors: an address >= cells (the reference asserts it, :226), a value >= r, batch outside 1 .. 8, a NULL array with nnz > 0, and
 * batch * N > 2^31 (timestamps are 32-bit) are SBN_EINVAL; tables that do not fit are SBN_ENOMEM.  A matrix with nnz = 0 is valid.
 * SBN_SCALARS_MONT: vals are ark-ff limbs.  The handle is independent of sbn_r1cs: encode calls both with the same arrays.
 * Lifetime: every pointer and table below belongs to the handle and lives until sbn_dense_free.  The two tables are read-only: never pass
 * them to a bind call or to sbn_table_free; views taken with sbn_table_slice / sbn_table_halves are freed before the handle. */
typedef struct sbn_dense sbn_dense;
int sbn_dense_build(sbn_ctx* ctx, size_t num_vars_x, size_t num_vars_y, const uint32_t* const* rows, const uint32_t* const* cols,
                    const uint8_t* const* vals, const size_t* nnz, size_t batch, uint32_t flags, sbn_dense** out);
void sbn_dense_free(sbn_ctx* ctx, sbn_dense* d);
size_t sbn_dense_num_ops(const sbn_dense* d);      /* N */
size_t sbn_dense_num_cells(const sbn_dense* d);
size_t sbn_dense_batch(const sbn_dense* d);
/* DEVICE arrays of uint32: what sbn_gather_merge / sbn_hash_layer[_pair] take.  side 0 = row, 1 = col; NULL for a bad side or k */
const void* sbn_dense_addr_dev(const sbn_dense* d, int side, size_t k);      /* N entries (ops_addr_usize) */
const void* sbn_dense_read_ts_dev(const sbn_dense* d, int side, size_t k);   /* N entries */
const void* sbn_dense_audit_ts_dev(const sbn_dense* d, int side);            /* cells entries */
/* the two merged polynomials as tables (for sbn_commit_table, sbn_table_slice, sbn_table_evaluate_many, sbn_table_bound, sbn_table_download) */
const sbn_table* sbn_dense_comb_ops(const sbn_dense* d);
const sbn_table* sbn_dense_comb_mem(const sbn_dense* d);

/* ---- SparseMatPolyEvalProof::prove (sparse_mlpoly_full.rs:1700-1755, the Hyrax build) in ONE call: what R1CSEvalProof::prove (r1cs.rs:435-462) wraps —
 *      equalize, the two eq tables, derefs and their commitment, challenge_r_hash, PolyEvalNetwork::new, ProductLayerProof::prove (:1306-1428) and
 *      HashLayerProof::prove (:922-1046) with DerefsEvalProof::prove (:412-432) and the three joint openings, every transcript line included ----
 * Notation: b = sbn_dense_batch(dense) (1 .. 4), N = sbn_dense_num_ops (>= 2), cells = sbn_dense_num_cells (>= 2), m = log2 cells = max(nx, ny),
 * n = log2 N; per opened polynomial k in {ops, mem, derefs}: ell_ops = n + log2 npo2(5 b), ell_mem = m + 1, ell_derefs = n + log2 npo2(2 b)
 * (:619-627), (L_k, R_k) = 2^sbn_factored_lens(ell_k), lg_k = log2 R_k; npo2 = next power of two.
 *   dense    only read: its tables, addresses and timestamps are left as they are.
 *   rx, ry   nx / ny canonical scalars; the shorter point is padded with zeros at the front (equalize, :1681-1697).
 *   evals    b canonical scalars: the claimed evaluations, one per matrix.
 *   gens_k   R_k + 1 generators with h, the handle sbn_polyeval_prove takes.  The derefs commitment runs over the first R_derefs of gens_derefs
 *            with no blinds; that subset is derived on first use, owned by gens_derefs and freed with it.
 *   rnd      the RandomTape draws of the three openings in the reference's order: derefs [3 + 2 lg_derefs] | ops [3 + 2 lg_ops] | mem [3 + 2 lg_mem],
 *            each as sbn_polyeval_prove takes them.     rnd_scalars = 9 + 2 (lg_derefs + lg_ops + lg_mem).
 *   out_proof  the fields of SparseMatPolyEvalProof in declaration order, nested structs likewise; points as sbn_g1_compress gives them, scalars canonical.
 *              PCEPB(c, l, d) = a ProductCircuitEvalProofBatched of c circuits, l layers, d dot-product circuits: sbn_product_proof_prove's out_polys
 *              (128 l (l - 1) / 2 bytes) followed by its out_claims (32 (2 c l + 3 d) bytes).  OPEN(lg) = sbn_polyeval_prove's out_proof (64 lg + 128 bytes).
 *                comm_derefs                  [L_derefs x 32]
 *                proof_prod_layer.eval_row    [init, read[b], write[b], audit]
 *                proof_prod_layer.eval_col    [init, read[b], write[b], audit]
 *                proof_prod_layer.eval_val    [eval_dotp_left[b], eval_dotp_right[b]]
 *                proof_prod_layer.proof_mem   PCEPB(4, m, 0): row init, row audit, col init, col audit   (declared before proof_ops, proved after it)
 *                proof_prod_layer.proof_ops   PCEPB(4 b, n, 2 b): row read[b], row write[b], col read[b], col write[b]; dot-product halves left_0, right_0, left_1, ...
 *                proof_hash_layer.eval_row    [addr[b], read_ts[b], audit_ts]
 *                proof_hash_layer.eval_col    [addr[b], read_ts[b], audit_ts]
 *                proof_hash_layer.eval_val    [b]
 *                proof_hash_layer.eval_derefs [row[b], col[b]]
 *                proof_hash_layer.proof_ops   OPEN(lg_ops)
 *                proof_hash_layer.proof_mem   OPEN(lg_mem)
 *                proof_hash_layer.proof_derefs OPEN(lg_derefs)
 *              proof_bytes = 32 L_derefs + 32 (13 b + 6) + 64 (m (m - 1) + n (n - 1)) + 256 (m + b n) + 192 b + 64 (lg_ops + lg_mem + lg_derefs) + 384.
 * `tr` is advanced exactly as the reference advances its transcript, and only when the call returns SBN_OK; out_proof is written only then.
 * SBN_EINVAL before any launch (text cites the reference's assert): a null pointer, batch > 4 (6 b instances must fit one product proof), N < 2, max(nx, ny) !=
 * log2 cells, a generator handle of the wrong size or without h, a scalar of rx, ry, evals or rnd >= r.  After launches: eval_dotp_left + eval_dotp_right !=
 * evals[i] is SBN_EINVAL (the reference panics, :1366); a failed subset check init * writes == reads * audit (:1324, :1339; impossible on a handle
 * sbn_dense_build made) is SBN_EHIP.  Same bytes as the loop over the calls above with the same draws (tests/sparse_eval_loop.py). */
/* host only: the sizes of rnd (in scalars) and out_proof (in bytes); SBN_EINVAL for a shape the call refuses (batch outside 1 .. 4, N < 2 or not a power of two) */
int sbn_sparse_eval_sizes(size_t num_vars_x, size_t num_vars_y, size_t num_ops /* N */, size_t batch, size_t* rnd_scalars, size_t* proof_bytes);
int sbn_sparse_eval_prove(sbn_ctx* ctx, const sbn_dense* dense, const uint8_t* rx, size_t nx, const uint8_t* ry, size_t ny, const uint8_t* evals /* batch x 32 */,
                          const sbn_bases* gens_ops, const sbn_bases* gens_mem, const sbn_bases* gens_derefs, const uint8_t* rnd, sbn_transcript* tr, uint8_t* out_proof);

/* ---- sbn_derefs_key: the KZG build's derefs commitment (Derefs::commit_kzg, sparse_mlpoly_full.rs:307-312) as a sum over memory cells ----
 * derefs[i] = eq[addr[i]], so  sum_i derefs[i] [tau^i]G = sum_a eq(rx)[a] S[0][a] + sum_a eq(ry)[a] S[1][a]  with
 *   S[side][a] = sum_{k < b} sum_{i < N, addr[side][k][i] = a} srs[(side b + k) N + i]
 * (coefficient i of polynomial k of that side in Derefs::new's merge order, :293-297).  S depends on the circuit and the SRS only: it is built once,
 * at encode time, and a proof's commitment becomes an MSM over the cells read at least once (at most 2 cells points) instead of npo2(2 b) N.
 * The group element is the same, bit for bit.
 *   build     enqueued on the context's stream, synchronised before it returns: the per-cell lists come from the handle's audit_ts (count) and read_ts
 *             (rank), the sums from the MSM's bucket accumulate (segments of SEG entries; sbn_prof_last_acc reports SEG, LPB = 1 and the two counters
 *             as for a bucket job).  Cells never read are dropped: they have no affine form.
 *             SBN_EINVAL before any launch: srs has an h, srs has fewer than n' = 2 b N points, 2 b N >= 2^31.
 *   lifetime  the key borrows nothing after the build, but records dense's shape, the SRS length and both handles' addresses so that
 *             sbn_sparse_eval_prove_kzg can refuse a foreign key: free it BEFORE the dense handle and the SRS.
 *   len       cells read at least once, row side + column side (>= 2: N >= 2 reads cell 0 on both sides).
 *   download  cells [first, first + count): out_cell[j] = side << 31 | a (row side first, a ascending), out_xy[64 j ..] = S[side][a], canonical affine x || y.
 *   commit    from the two eq tables (sbn_eq_evals of the equalized points, cells entries each): the point sbn_kzg_commit gives on the gathered,
 *             merged table.  SBN_EINVAL for a table shorter than cells. */
typedef struct sbn_derefs_key sbn_derefs_key;
int sbn_derefs_key_build(sbn_ctx* ctx, const sbn_dense* dense, const sbn_bases* srs, sbn_derefs_key** out);
void sbn_derefs_key_free(sbn_ctx* ctx, sbn_derefs_key* key);
size_t sbn_derefs_key_len(const sbn_derefs_key* key);
int sbn_derefs_key_download(sbn_ctx* ctx, const sbn_derefs_key* key, size_t first, size_t count, uint32_t* out_cell, uint8_t* out_xy);
int sbn_derefs_key_commit(sbn_ctx* ctx, const sbn_derefs_key* key, const sbn_table* mem_rx, const sbn_table* mem_ry, uint8_t out_xy[64], int* out_is_inf);

/* ---- SparseMatPolyEvalProof::prove, the KZG build (--features kzg, sparse_mlpoly_full.rs:1757-1813) in ONE call ----
 * Everything of sbn_sparse_eval_prove above holds (notation, dense, rx, ry, evals, gens_ops, gens_mem, the transcript and out_proof rules) except:
 *   srs      the KZG SRS (sbn_kzg_srs_upload / _from_tau: no h) in place of gens_derefs.  n_d = npo2(2 b) N is the derefs polynomial's length,
 *            n' = 2 b N its non-zero prefix; the SRS must hold n_d - 1 points (the reference slices the quotient's bases, kzg.rs:186).
 *   key      sbn_derefs_key_build(dense, srs), or NULL.  The bytes are the same with and without it.
 *   the commitment  (:1781-1785, :349-356, kzg.rs:386-404) ONE point.  With a key: sbn_derefs_key_commit's body.  Without: the MSM of the first
 *            min(n', srs->n) entries of the gathered table (KZGPolyCommitment::commit's truncation, restricted to the non-zero prefix).  Transcript:
 *            derefs_commitment / begin_derefs_commitment, comm_poly_row_col_ops_val <- the 32 compressed bytes, derefs_commitment / end_derefs_commitment.
 *   DerefsEvalProof::prove  (:503-550) protocol name "Derefs evaluation proof (KZG)", evals_ops_val per scalar, log2 npo2(2 b) challenges
 *            challenge_combine_n_to_one, joint_claim_eval, the challenge kzg_eval_point, then KZGProof::prove on the derefs table: the division over
 *            n' coefficients and the MSM of the n' - 1 quotient coefficients (q_i = 0 from n' - 1 on).  Nothing is appended afterwards, no draw is used.
 *   rnd      ops [3 + 2 lg_ops] | mem [3 + 2 lg_mem].     rnd_scalars = 6 + 2 (lg_ops + lg_mem).
 *   out_proof  the Hyrax layout with  comm_derefs [32]  and  proof_hash_layer.proof_derefs [proof 32 | eval 32]  (the identity as sbn_g1_compress writes it).
 *              proof_bytes = 32 (13 b + 6) + 64 (m (m - 1) + n (n - 1)) + 256 (m + b n) + 192 b + 64 (lg_ops + lg_mem) + 352.
 * SBN_EINVAL before any launch: the Hyrax call's refusals (without gens_derefs), an SRS with h, srs->n < n_d - 1, a key whose recorded shape, SRS length or
 * handles are not this call's.  sbn_sparse_eval_verify_kzg checks this proof in one call. */
int sbn_sparse_eval_kzg_sizes(size_t num_vars_x, size_t num_vars_y, size_t num_ops /* N */, size_t batch, size_t* rnd_scalars, size_t* proof_bytes);
int sbn_sparse_eval_prove_kzg(sbn_ctx* ctx, const sbn_dense* dense, const uint8_t* rx, size_t nx, const uint8_t* ry, size_t ny, const uint8_t* evals /* batch x 32 */,
                              const sbn_bases* gens_ops, const sbn_bases* gens_mem, const sbn_bases* srs, const sbn_derefs_key* key /* or NULL */,
                              const uint8_t* rnd, sbn_transcript* tr, uint8_t* out_proof);

/* ---- pairings and KZG verification: Bn254::pairing at the reference's verifier call sites (kzg.rs:196-217, :315-352) ----
 * Tower: Fq2 = Fq[u]/(u^2 + 1), xi = 9 + u, Fq6 = Fq2[v]/(v^3 - xi), Fq12 = Fq6[w]/(w^2 - v) (arkworks').  A GT value is 384 bytes: the twelve Fq
 * coefficients c0.c0.c0, c0.c0.c1, c0.c1.c0, ..., c1.c2.c1, each 32 bytes little-endian canonical.  The pairing is the optimal ate pairing with the
 * EXACT final exponent (q^12 - 1)/r, so GT bytes are comparable with any implementation that takes that exponent (tests/pairing_model.py).
 * A G2 point is 128 bytes  x.c0 | x.c1 | y.c0 | y.c1  of the twist E': y^2 = x^3 + 3/xi, each part canonical (< q) little-endian; with SBN_POINTS_MONT
 * the parts are ark-ff's Montgomery limbs (G2Affine's in-memory x, y).  A G1 point is 64 bytes x | y as everywhere; 64 zero bytes: the identity. */
typedef struct sbn_g2_lines sbn_g2_lines;
/* G2Prepared::from (what Bn254::pairing builds from srs.g2 / srs.tau_g2 on every call, kzg.rs:212-214), ONCE per point: parsed, checked, the 88 lines of
 * its Miller loop computed on the host (most of the time is the literal subgroup test [r]Q == O; DESIGN 4.20 has the figure) and uploaded (11 KiB).  The handle belongs to `ctx`.
 * SBN_EINVAL: a NULL pointer, unknown flags, a coordinate >= q, the identity (128 zero bytes), a point off E', a point of E' outside the r-torsion
 * (#E'(Fq2) = r (2q - r): most points of E' are). */
int sbn_g2_prepare(sbn_ctx* ctx, const uint8_t q_xy[128], uint32_t flags, sbn_g2_lines** out);
/* releases the handle to the context that made it (`ctx` is not consulted: a handle knows its context); before that context is destroyed */
void sbn_g2_lines_free(sbn_ctx* ctx, sbn_g2_lines* l);
/* Bn254::multi_pairing (kzg.rs:212-216 compares two of them): nchecks independent products  prod_t e(P_t, Q_t)  in ONE launch of k_pairing_products,
 * one wave a check.  counts[i] in 0 .. 4: the terms of check i, laid out one check after the other in p_xy (64 B each) and q; 0 terms is the empty
 * product (is_one = 1), a term whose P is the identity contributes 1.  The same handle may stand in any number of terms.
 * out_is_one: nchecks bytes, 1 where the product is the unit of GT;  out_gt: nchecks x 384 bytes, or NULL.  One upload, one launch, one wait.
 * SBN_EINVAL before any launch, outputs untouched: a NULL pointer, nchecks > 65536, counts[i] > 4, a NULL handle or one of another context, a P that is not a canonical
 * point of the curve.  nchecks == 0 is SBN_OK and touches nothing. */
int sbn_pairing_products(sbn_ctx* ctx, const uint8_t* p_xy, const sbn_g2_lines* const* q, const uint32_t* counts, size_t nchecks,
                         uint8_t* out_is_one, uint8_t* out_gt);
/* KZGProof::verify (kzg.rs:196-217) / KZGPolyEvalProof::verify (:428-437):  e(C - y G, g2) == e(pi, tau_g2 - z g2)  tested as
 *     e(C - y G + z pi, g2) * e(-pi, tau_g2) == 1
 * which is the same statement by bilinearity alone (no relation between g2 and tau_g2 is assumed) and multiplies no G2 point.  G = (1, 2).
 * Work: the three-term G1 sum through sbn_g1_small_sums' launch and fold, then one two-term k_pairing_products launch: two host waits.
 * pi = O reduces the check to C == y G.  The return code reports misuse only — SBN_EINVAL before any launch, *accepted untouched: a NULL pointer,
 * a handle of another context, z or eval >= r, a commitment that is not a canonical point of the curve.  A proof point that is not on the curve
 * is the prover's doing: SBN_OK with *accepted = 0, as for a failed product. */
int sbn_kzg_verify(sbn_ctx* ctx, const sbn_g2_lines* g2, const sbn_g2_lines* tau_g2, const uint8_t comm_xy[64], const uint8_t z[32],
                   const uint8_t eval[32], const uint8_t proof_xy[64], int* accepted);
/* KZGBatchProof::batch_verify (kzg.rs:315-352): the check above on  sum_k gamma^k C_k  and  sum_k gamma^k evals[k]; gamma from the caller's
 * transcript as in sbn_kzg_open_batched (any canonical value, zero included).  The combination is part of the same G1 sum (count + 2 terms):
 * count <= 62.  count = 0 tests pi against the identity commitment.  SBN_EINVAL as above, and for count > 62 or an eval >= r. */
int sbn_kzg_verify_batched(sbn_ctx* ctx, const sbn_g2_lines* g2, const sbn_g2_lines* tau_g2, const uint8_t* comms_xy, size_t count,
                           const uint8_t z[32], const uint8_t gamma[32], const uint8_t* evals, const uint8_t proof_xy[64], int* accepted);

/* SparseMatPolyEvalProof::verify, the KZG build (--features kzg; sparse_mlpoly_full.rs:1815-1845 with DerefsEvalProof::verify, :552-595) in ONE call:
 * sbn_sparse_eval_verify above with (g2, tau_g2) in place of gens_derefs and the proof layout of sbn_sparse_eval_prove_kzg (sbn_sparse_eval_kzg_sizes):
 * comm_derefs [32], proof_hash_layer.proof_derefs [proof 32 | eval 32].  With sbn_r1cs_proof_verify the KZG build's SNARK::verify is two foreign calls.
 * The commitment is absorbed as :349-356 does; derefs_reduce (:561-584) runs on the host: as in the reference the joint claim is absorbed and NOT
 * compared, and the opening is checked at kzg_eval_point against the proof's own eval.  The field half, the transcript and the two joint openings of
 * comb_ops and comb_mem are the Hyrax call's (one decompress launch over their points, one wait an opening, one for the two final equations: three
 * host waits); behind them comm_derefs and pi are decompressed (sbn_g1_decompress: one wait) and the opening is checked as sbn_kzg_verify checks it (two
 * waits): SIX host waits a call.  The pairing check is not yet queued under the host's hashing of the openings; it costs its 2 ms behind them.
 * Rules as for sbn_sparse_eval_verify: SBN_EINVAL before any launch with `tr` and *accepted untouched for a NULL pointer, a G2 handle of another
 * context, a bad shape, handle size or non-canonical rx, ry, evals.  SBN_OK with *accepted = 0 for what the prover controls, among it an eval >= r inside
 * the proof, comm_derefs or pi that does not decompress, a failed pairing product.  `tr` moves on only behind *accepted == 1 and then ends where
 * sbn_sparse_eval_prove_kzg's transcript ended. */
int sbn_sparse_eval_verify_kzg(sbn_ctx* ctx, size_t num_vars_x, size_t num_vars_y, size_t num_ops, size_t num_cells, size_t batch,
                               const sbn_bases* comm_ops, const sbn_bases* comm_mem, const uint8_t* rx, const uint8_t* ry, const uint8_t* evals,
                               const sbn_bases* gens_ops, const sbn_bases* gens_mem, const sbn_g2_lines* g2, const sbn_g2_lines* tau_g2,
                               const uint8_t* proof, sbn_transcript* tr, int* accepted);

/* ---- Instance::is_sat (snark.rs:137-158 -> R1CSShape::is_sat, r1cs.rs:105-123) on the device: does z = vars | 1 | input satisfy Az o Bz = Cz? ----
 *   vars   a table of at most num_vars entries (a power of two, as every table); a shorter one is zero-padded on the device (Assignment::pad).
 *   input  num_inputs canonical scalars, num_inputs < num_vars (z has 2 num_vars entries).
 * Work: k_r1cs_build_z, the launches of sbn_r1cs_multiply into tables of the call's own (released before it returns), then ONE k_r1cs_sat_check pass:
 * a lane a row, Az[i] Bz[i] - Cz[i] tested on its canonical value, one atomicAdd and one atomicMin a block.  One host wait.
 *   *sat = 1: every row holds.  Otherwise *num_bad = the violated rows and *first_bad = the lowest of them (meaningful only with *sat == 0).
 * SBN_EINVAL before any launch, outputs untouched: a NULL pointer, vars longer than num_vars, num_inputs >= num_vars, an input >= r. */
int sbn_r1cs_is_sat(sbn_ctx* ctx, const sbn_r1cs* inst, const sbn_table* vars, const uint8_t* input, size_t num_inputs,
                    int* sat, uint64_t* num_bad, uint64_t* first_bad);

/* ---- the reference's public surface in one call each: SNARKGens::new, Instance::new + SNARK::encode, Instance::is_sat, SNARK::prove, SNARK::verify
 *      (snark.rs:59-158, :290-529), both builds.  NIZK mode (snark.rs:162-287) follows below as sbn_nizk_*: its transcript absorbs R1CSShape::get_digest
 *      (zlib over bincode, r1cs.rs:97-101), which arrives as bytes — the caller's inst.digest — and is never computed here. ----
 * Shapes are RAW: num_cons, num_vars, num_inputs as the circuit has them, columns as the circuit numbers them (vars | 1 | inputs).  Instance::new's
 * rules are applied inside (snark.rs:74-110): num_vars_padded = npo2(max(num_vars, num_inputs + 1)), num_cons_padded = npo2(max(num_cons, 2)), a column
 * >= num_vars moves to col + num_vars_padded - num_vars; nx = log2 num_cons_padded, ny = log2(2 num_vars_padded).  Entry order is kept.
 *
 * sbn_snark_gens: SNARKGens (snark.rs:305-328).  Six sets through sbn_gens_new: under the label "gens_r1cs_sat" gens_pc (R + 1 generators with h,
 *   (L, R) = 2^sbn_factored_lens(log2 num_vars_padded)), gens_3 and gens_4 (r1csproof.rs:155-182: gens_1 is gens_pc's); under "gens_r1cs_eval"
 *   gens_ops, gens_mem, gens_derefs (R_k + 1 each, sbn_sparse_eval_prove's notation with b = 3, N = npo2(num_nz_entries), sparse_mlpoly_full.rs:612-630).
 *   num_nz_entries is the largest of the three nnz, as the reference requires (r1cs.rs:273-274): a bundle made for another N is refused by encode.
 *   sbn_snark_gens_get(gens, which): which = 0 gens_pc, 1 gens_3, 2 gens_4, 3 gens_ops, 4 gens_mem, 5 gens_derefs; owned by the bundle (e.g. for
 *   sbn_bases_precompute); NULL for another `which`.  The KZG build ignores gens_derefs.
 *
 * sbn_snark_key: what SNARK::encode returns, resident.  The prover's half: the matrices (sbn_r1cs) and their dense representation (sbn_dense); the
 *   verifier's half: the shape and the two PolyCommitments of R1CSCommitment as point sets.
 *   sbn_snark_encode      rows / cols / vals / nnz: three matrices as sbn_r1cs_upload takes them, raw.  In order: the conversion on the host, sbn_r1cs_upload,
 *                         sbn_dense_build(nx, ny), DensePolynomial::commit of comb_ops and comb_mem with no blinds (hyrax.rs:283-308), sbn_g1_compress.
 *                         SBN_EINVAL: a row >= num_cons, a col >= num_vars + 1 + num_inputs, a value >= r (snark.rs:95-101), num_vars_padded < 2, no matrix
 *                         with more than one entry (N < 2: product_tree.rs:89), a bundle made for another shape or N, flags other than SBN_SCALARS_MONT.
 *   sbn_snark_key_comm    R1CSCommitment as bytes: six little-endian u64  num_cons_padded | num_vars_padded | num_inputs | batch (3) | num_ops N |
 *                         num_mem_cells,  then comm_comb_ops [L_ops x 32] and comm_comb_mem [L_mem x 32] as sbn_g1_compress gives them, L_k = 2^left of
 *                         sbn_factored_lens(ell_k).  *len <- the length, always; out == NULL asks for the length alone; cap < *len is SBN_EINVAL.
 *   sbn_snark_key_from_comm  the verifier's half from those bytes (sbn_bases_from_compressed twice).  The bytes are the caller's own data: SBN_EINVAL for a
 *                         wrong length, a size that is no power of two, N < 2, num_mem_cells != 2^max(nx, ny), num_inputs >= num_vars_padded, batch != 3,
 *                         a point that does not decompress.  Proving or checking a witness on such a key is SBN_EINVAL.
 *   sbn_snark_key_dense   the prover's dense handle, owned by the key (NULL on a verifier key): what sbn_derefs_key_build takes for the KZG build.
 *   sbn_snark_sizes       kzg = 0 / 1: rnd_scalars and proof_bytes of the build.
 *        rnd   = sbn_r1cs_proof_prove's rnd | sbn_sparse_eval_prove[_kzg]'s rnd: ONE RandomTape (b"snark_proof", snark.rs:438), draws in call order.
 *        proof = r1cs_sat_proof (sbn_r1cs_proof_prove's out_proof) | inst_evals A, B, C(rx, ry) [96] | r1cs_eval_proof (sbn_sparse_eval_prove[_kzg]'s
 *                out_proof): the declaration order of snark.rs:405-409.
 *
 * sbn_snark_is_sat: sbn_r1cs_is_sat on the key's matrices; num_inputs must be the instance's (snark.rs:145).
 * sbn_snark_prove: SNARK::prove (snark.rs:428-484).  Transcript: protocol-name "Spartan SNARK proof"; R1CSCommitment::append_to_transcript (r1cs.rs:355-362,
 *   sparse_mlpoly_full.rs:710-717): append_u64 (Merlin's: eight little-endian bytes) of num_cons, num_vars, num_inputs, batch_size, num_ops,
 *   num_mem_cells, then the two PolyCommitments under comm_comb_ops / comm_comb_mem (hyrax.rs:44-51); then R1CSProof::prove on the padded vars
 *   (sbn_r1cs_proof_prove's body), A, B, C(rx, ry) (sbn_r1cs_evaluate's), R1CSEvalProof::prove (sbn_sparse_eval_prove's), all under one hold of the mutex.
 *   vars: at most num_vars_padded entries; a table at raw and at padded length give the same bytes.  num_inputs must be the instance's.
 *   flags: SBN_SNARK_CHECK_SAT runs the witness check first; an unsatisfied witness is SBN_EUNSAT before any proving launch (the text names the count and
 *   the first row).  `tr` moves on and out_proof is written only behind SBN_OK.  SBN_EINVAL before any launch: a NULL pointer, a verifier key, unknown
 *   flags, a wrong num_inputs, vars too long, a bundle of another shape, a scalar of input or rnd >= r; the KZG build's SRS and derefs-key rules are
 *   sbn_sparse_eval_prove_kzg's (derefs_key: sbn_derefs_key_build(sbn_snark_key_dense(key), srs), or NULL).
 * sbn_snark_verify: SNARK::verify (snark.rs:487-528) on either kind of key: proof_len against sbn_snark_sizes, the prefix, R1CSProof::verify with the
 *   proof's own inst_evals (sbn_r1cs_proof_verify's body), R1CSEvalProof::verify at the (rx, ry) it returned (sbn_sparse_eval_verify[_kzg]'s); a refused
 *   first half skips the second.  SBN_EINVAL before any launch, `tr` unchanged: a NULL pointer, a wrong proof_len or num_inputs, an input >= r, a
 *   bundle of another shape, a G2 handle of another context.  What the prover controls is SBN_OK with *accepted = 0, an inst_evals scalar >= r among
 *   it.  `tr` moves on only behind *accepted == 1 and then ends where sbn_snark_prove's transcript ended. */
#define SBN_EUNSAT (-5)            /* sbn_snark_prove with SBN_SNARK_CHECK_SAT: the witness does not satisfy the instance */
#define SBN_SNARK_CHECK_SAT 1u
typedef struct sbn_snark_gens sbn_snark_gens;
typedef struct sbn_snark_key sbn_snark_key;
int sbn_snark_gens_new(sbn_ctx* ctx, size_t num_cons, size_t num_vars, size_t num_inputs, size_t num_nz_entries, sbn_snark_gens** out);
const sbn_bases* sbn_snark_gens_get(const sbn_snark_gens* gens, int which);
void sbn_snark_gens_free(sbn_ctx* ctx, sbn_snark_gens* gens);
int sbn_snark_encode(sbn_ctx* ctx, size_t num_cons, size_t num_vars, size_t num_inputs, const uint32_t* const* rows, const uint32_t* const* cols,
                     const uint8_t* const* vals, const size_t* nnz, uint32_t flags, const sbn_snark_gens* gens, sbn_snark_key** out);
int sbn_snark_key_from_comm(sbn_ctx* ctx, const uint8_t* comm, size_t len, sbn_snark_key** out);
int sbn_snark_key_comm(const sbn_snark_key* key, uint8_t* out, size_t cap, size_t* len);
const sbn_dense* sbn_snark_key_dense(const sbn_snark_key* key);
void sbn_snark_key_free(sbn_ctx* ctx, sbn_snark_key* key);
int sbn_snark_sizes(const sbn_snark_key* key, int kzg, size_t* rnd_scalars, size_t* proof_bytes);
int sbn_snark_is_sat(sbn_ctx* ctx, const sbn_snark_key* key, const sbn_table* vars, const uint8_t* input, size_t num_inputs,
                     int* sat, uint64_t* num_bad, uint64_t* first_bad);
int sbn_snark_prove(sbn_ctx* ctx, const sbn_snark_key* key, const sbn_table* vars, const uint8_t* input, size_t num_inputs, const sbn_snark_gens* gens,
                    uint32_t flags, const uint8_t* rnd, sbn_transcript* tr, uint8_t* out_proof);
int sbn_snark_verify(sbn_ctx* ctx, const sbn_snark_key* key, const uint8_t* input, size_t num_inputs, const sbn_snark_gens* gens,
                     const uint8_t* proof, size_t proof_len, sbn_transcript* tr, int* accepted);
int sbn_snark_prove_kzg(sbn_ctx* ctx, const sbn_snark_key* key, const sbn_table* vars, const uint8_t* input, size_t num_inputs, const sbn_snark_gens* gens,
                        const sbn_bases* srs, const sbn_derefs_key* derefs_key /* or NULL */, uint32_t flags, const uint8_t* rnd, sbn_transcript* tr,
                        uint8_t* out_proof);
int sbn_snark_verify_kzg(sbn_ctx* ctx, const sbn_snark_key* key, const uint8_t* input, size_t num_inputs, const sbn_snark_gens* gens,
                         const sbn_g2_lines* g2, const sbn_g2_lines* tau_g2, const uint8_t* proof, size_t proof_len, sbn_transcript* tr, int* accepted);

/* ---- NIZK mode in one call each: NIZKGens::new, Instance::new, Instance::is_sat, NIZK::prove, NIZK::verify (snark.rs:162-287).  No preprocessing: no
 *      dense representation, no commitment, and the verifier holds the matrices.  A prove is the R1CS proof alone.  Shapes are RAW, as for sbn_snark_*. ----
 * The digest: NIZK::prove and ::verify append inst.digest under "R1CSShapeDigest" (snark.rs:213, :253) and do nothing else with it.  It is an opaque byte
 *   string that Instance::new computed once (snark.rs:125-127); the caller passes those bytes to sbn_nizk_instance_new, which keeps a copy.  Any length
 *   up to 2^32 - 1 is taken, NULL with length 0 too; the library does not compute, check or interpret them.  Prover and verifier must hold the same bytes.
 *
 * sbn_nizk_gens_new: NIZKGens::new (snark.rs:169-180) = R1CSGens::new(b"gens_r1cs_sat", num_cons, num_vars_padded): the first three sets of
 *   sbn_snark_gens_new (gens_pc, gens_3, gens_4) under the same label, as a sbn_snark_gens whose three eval sets are absent: sbn_snark_gens_get(g, 3..5)
 *   is NULL, sbn_snark_encode / _prove / _verify refuse it (SBN_EINVAL), sbn_snark_gens_free frees it.  A whole SNARK bundle of the right shape is taken
 *   by the NIZK calls and gives the same bytes.
 * sbn_nizk_instance_new: Instance::new (snark.rs:66-128) on a raw circuit, as sbn_snark_encode takes one: the conversion on the host with its three errors
 *   in the reference's order (a row >= num_cons, a col >= num_vars + 1 + num_inputs, a value >= r: SBN_EINVAL, the text names the entry), then
 *   sbn_r1cs_upload.  No sbn_dense_build, no commitment.  num_vars_padded < 2 is SBN_EINVAL as in encode; an instance whose matrices hold one entry or
 *   none is valid (encode's N < 2 rule comes from the product circuits, which NIZK does not have).  flags: SBN_SCALARS_MONT only.
 *   sbn_nizk_instance_r1cs   the matrices, owned by the handle: what sbn_r1cs_evaluate takes.  NULL for NULL.
 *   sbn_nizk_sizes           rnd_scalars = sbn_r1cs_proof_sizes' count at the padded shape; proof_bytes = its proof length + 32 (nx + ny).
 *        proof = r1cs_sat_proof (sbn_r1cs_proof_prove's out_proof) | rx [nx x 32] | ry [ny x 32], canonical: the declaration order of snark.rs:191-194.
 * sbn_nizk_is_sat: sbn_r1cs_is_sat on the handle's matrices; num_inputs must be the instance's (snark.rs:145).
 * sbn_nizk_prove: NIZK::prove (snark.rs:202-240) under one hold of the mutex: protocol-name "Spartan NIZK proof", "R1CSShapeDigest" <- the digest,
 *   Assignment::pad on the device, R1CSProof::prove (sbn_r1cs_proof_prove's body); out_proof = its proof | the rx, ry it returned.  rnd: R1CSProof::prove's
 *   draws (RandomTape b"proof", snark.rs:210), drawn by the caller.  vars: at most num_vars_padded entries; a table at raw and at padded length give the
 *   same bytes.  flags: SBN_SNARK_CHECK_SAT as in sbn_snark_prove: an unsatisfied witness is SBN_EUNSAT before any proving launch.  `tr` moves on and
 *   out_proof is written only behind SBN_OK.  SBN_EINVAL before any launch: a NULL pointer, unknown flags, a wrong num_inputs, vars longer than
 *   num_vars_padded, a bundle of another shape, a scalar of input or rnd >= r.
 * sbn_nizk_verify: NIZK::verify (snark.rs:243-286): the two prefix lines; A, B, C at the CLAIMED (rx, ry) over the handle's own matrices (sbn_r1cs_evaluate's
 *   body); R1CSProof::verify with those three values (sbn_r1cs_proof_verify's body); then the (rx, ry) it derived against the claimed ones.  That last
 *   comparison is assert_eq! in the reference (snark.rs:280-281), a panic; a proof is the prover's data, so here a mismatch is a refusal: SBN_OK with
 *   *accepted = 0.  So are a claimed scalar >= r and a refused R1CS proof.  SBN_EINVAL reports misuse only, before any launch and with `tr` and
 *   *accepted unchanged: a NULL pointer, a wrong proof_len or num_inputs, an input >= r, a bundle of another shape.  `tr` moves on only behind
 *   *accepted == 1 and then ends where sbn_nizk_prove's transcript ended. */
typedef struct sbn_nizk_inst sbn_nizk_inst;
int sbn_nizk_gens_new(sbn_ctx* ctx, size_t num_cons, size_t num_vars, size_t num_inputs, sbn_snark_gens** out);
int sbn_nizk_instance_new(sbn_ctx* ctx, size_t num_cons, size_t num_vars, size_t num_inputs, const uint32_t* const* rows, const uint32_t* const* cols,
                          const uint8_t* const* vals, const size_t* nnz, uint32_t flags, const uint8_t* digest, size_t digest_len, sbn_nizk_inst** out);
void sbn_nizk_instance_free(sbn_ctx* ctx, sbn_nizk_inst* inst);
const sbn_r1cs* sbn_nizk_instance_r1cs(const sbn_nizk_inst* inst);
int sbn_nizk_sizes(const sbn_nizk_inst* inst, size_t* rnd_scalars, size_t* proof_bytes);
int sbn_nizk_is_sat(sbn_ctx* ctx, const sbn_nizk_inst* inst, const sbn_table* vars, const uint8_t* input, size_t num_inputs,
                    int* sat, uint64_t* num_bad, uint64_t* first_bad);
int sbn_nizk_prove(sbn_ctx* ctx, const sbn_nizk_inst* inst, const sbn_table* vars, const uint8_t* input, size_t num_inputs, const sbn_snark_gens* gens,
                   uint32_t flags, const uint8_t* rnd, sbn_transcript* tr, uint8_t* out_proof);
int sbn_nizk_verify(sbn_ctx* ctx, const sbn_nizk_inst* inst, const uint8_t* input, size_t num_inputs, const sbn_snark_gens* gens,
                    const uint8_t* proof, size_t proof_len, sbn_transcript* tr, int* accepted);

/* ---- circom's .r1cs and .wtns files straight onto the device (reference src/r1cs_reader.rs, examples/keyless_benchmark.rs:38-72) ----
 * The caller maps or reads the two files; bytes go in, resident handles come out, and the prove and verify calls above take those handles as they are.
 * The host scans the sections and walks the 3 * nConstraints entry counts (the format's one sequential dependency); the payload goes up in one copy and
 * everything per entry — the record, the value against r, the column remap, the two compressed copies, the dense representation — is device work.
 *
 * sbn_circom_r1cs_load: R1CS::from_reader (r1cs_reader.rs:55-191) and to_sparse_matrices_padded (:213-242) at the padded shape Instance::new gives
 *   (num_vars = nWires - 1 - num_pub_inputs, num_inputs = num_pub_inputs = nPubOut + nPubIn, num_cons = nConstraints; snark.rs:74-90).  The handle holds,
 *   per matrix and in file order, (row = constraint, remapped column, canonical value): wire 0 -> num_vars_padded, wires 1..=num_pub_inputs ->
 *   num_vars_padded + wire, the others -> wire - num_pub_inputs - 1.  An entry whose value is >= r is dropped, as the reader drops it (:156-158), and
 *   counted in `dropped`.  Refused with SBN_EINVAL and a reason in sbn_last_error: a wrong magic, a version other than 1, field_size other than 32, a
 *   missing section 1 or 2, any read past `len`, nWires < 1 + num_pub_inputs, more than 2^31 entries, a shape past 2^29; and three things the reference
 *   would misread without a word: a prime that is not BN254's r, a constraints walk that passes the end of section 2 (the reference reads on into the
 *   next section), a wire >= nWires (the reference aliases it onto another column; the text names the entry).  One host wait; a second one only where a
 *   value was dropped.  The file's bytes are free again when the call returns.
 * sbn_circom_r1cs_info: the stored counts, no device work.  nnz[m] are R1CSStats' nnz_a, _b, _c (kept entries); their maximum is the num_nz_entries
 *   sbn_snark_gens_new takes.
 * sbn_circom_r1cs_download: matrix m (0, 1, 2) as to_sparse_matrices_padded(num_vars_padded) returns it: nnz[m] rows, columns and 32-byte values.
 * sbn_r1cs_from_circom: the handle sbn_r1cs_upload(num_cons_padded, num_vars_padded, ...) makes of those triplets, without the host's sorts.
 * sbn_nizk_instance_from_circom: sbn_nizk_instance_new on the parsed circuit; the digest stays the caller's bytes.
 * sbn_snark_encode_circom: sbn_snark_encode on the parsed circuit, with the same refusals (num_vars_padded < 2, N < 2, a bundle of another shape or N).
 * The handles made from a sbn_circom_r1cs keep nothing of it: it may be freed right after.
 * sbn_circom_wtns_load: parse_wtns (keyless_benchmark.rs:38-72): input <- witness[1 .. 1 + num_inputs] (canonical bytes), *vars <- witness[1 + num_inputs ..]
 *   as a table of next_power_of_two(max(its length, num_inputs + 1)) entries, zeros behind the last value; *num_witness <- the file's value count.  Refused
 *   (SBN_EINVAL, no table) where the example truncates or concatenates without a word: a second section 2, a section past the end of the file, a size
 *   that is no multiple of 32, fewer than 1 + num_inputs values, and a value >= r (the example takes its low 64 bits; the text names the index). */
typedef struct sbn_circom_r1cs sbn_circom_r1cs;
typedef struct {
  uint64_t num_constraints, num_variables, num_pub_inputs, num_prv_inputs, num_labels;
  uint64_t nnz[3];       /* kept entries: R1CSStats' nnz_a, _b, _c */
  uint64_t dropped[3];   /* values >= r the reader skipped */
  uint64_t num_vars, num_cons_padded, num_vars_padded;
} sbn_circom_info;
int sbn_circom_r1cs_load(sbn_ctx* ctx, const uint8_t* file, size_t len, sbn_circom_r1cs** out);
int sbn_circom_r1cs_info(const sbn_circom_r1cs* f, sbn_circom_info* out);
int sbn_circom_r1cs_download(sbn_ctx* ctx, const sbn_circom_r1cs* f, int m, uint32_t* rows, uint32_t* cols, uint8_t* vals);
void sbn_circom_r1cs_free(sbn_ctx* ctx, sbn_circom_r1cs* f);
int sbn_r1cs_from_circom(sbn_ctx* ctx, const sbn_circom_r1cs* f, sbn_r1cs** out);
int sbn_nizk_instance_from_circom(sbn_ctx* ctx, const sbn_circom_r1cs* f, const uint8_t* digest, size_t digest_len, sbn_nizk_inst** out);
int sbn_snark_encode_circom(sbn_ctx* ctx, const sbn_circom_r1cs* f, const sbn_snark_gens* gens, sbn_snark_key** out);
int sbn_circom_wtns_load(sbn_ctx* ctx, const uint8_t* file, size_t len, size_t num_inputs, sbn_table** vars, uint8_t* input, size_t* num_witness);

/* ---- a circuit digest computed on the device: the bytes sbn_nizk_instance_from_circom takes, for a caller who has no Rust side to ask ----
 * THIS IS THE LIBRARY'S OWN DIGEST.  It is not the reference's R1CSShape::get_digest (zlib over bincode, r1cs.rs:97-101), which is not reproduced here:
 * a NIZK proof made under one digest does not verify under the other.  Prover and verifier must both take this one, or both the reference's.
 * It is defined over what sbn_circom_r1cs_download returns — kept entries in file order, remapped columns, canonical values — and not over the
 * file's bytes, so the order of the file's sections and its dropped (>= r) entries do not change it:
 *     leaf(m, j) = SHAKE256("sbn254/r1cs-digest/leaf/v1" | u8 m | u64le j | u32le k | k x (u32le row | u32le col | val[32]))[0..32]
 *                  entries 128 j .. 128 j + k - 1 of matrix m,  k = min(128, nnz[m] - 128 j);  no leaf for nnz[m] = 0
 *     root       = SHAKE256("sbn254/r1cs-digest/root/v1" | u64le num_constraints | num_variables | num_pub_inputs | num_cons_padded | num_vars_padded
 *                           | for m = 0, 1, 2: u64le nnz[m] | the leaves of m in order)[0..32]
 * with the five shape fields as sbn_circom_r1cs_info gives them.  A row, a column, a value, a shape field, the matrix an entry sits in and the order
 * of two entries all change it.
 * Work: ONE launch of k_circom_digest_leaves, a lane a leaf (Keccak-f[1600] on 25 lanes in registers, the leaf's 5 KiB read as dwords where the handle
 * holds them), the leaves (32 B per 128 entries) brought back behind ONE host wait, and one SHAKE256 over them on the host (DESIGN 4.25 has the times).
 * SBN_EINVAL: a NULL pointer.  A circuit without entries has a digest (the root over the shape and three zero counts) and launches nothing. */
int sbn_circom_r1cs_digest(sbn_ctx* ctx, const sbn_circom_r1cs* f, uint8_t out[32]);

/* ---- the prover's randomness: RandomTape (random.rs) and the draw plans that fill `rnd` for every one-call prover above.  Host only: no context,
 *      no device.  A tape is a Merlin transcript of its own; a tape started from the same `init` gives the draws the reference's tape gives, so a Rust
 *      caller and a C caller with one seed make one proof.  A Rust caller may equally keep its own tape and pass its draws as before. ----
 * sbn_random_tape_new: RandomTape::new (random.rs:15-23): Transcript::new(name), append_scalar(b"init_randomness", init).  The reference's names are
 *   b"snark_proof" (snark.rs:438) and b"proof" (snark.rs:210).  init: 32 canonical bytes (>= r: SBN_EINVAL), or NULL: 64 bytes from getrandom(2) reduced
 *   mod r as a challenge is (sbn_fr_from_wide), which stands in for Scalar::random(&mut OsRng); a failure of getrandom is SBN_EOS with errno's text.
 *   A fixed init makes a proof reproducible and its blinds predictable: it is for tests and for a caller that derives it from its own entropy.
 * sbn_random_tape_scalars: random_scalar / random_vector (:25-31): n x challenge_scalar(label) (transcript.rs:56-71), n x 32 canonical bytes.  n = 0 and
 *   an empty label (NULL with length 0) are legal.
 * sbn_random_tape_free: wipes the state before it is released.  No call prints, logs or keeps init or a draw; error texts never hold one.
 * sbn_random_tape_last_error: why the last call on this tape was refused; with NULL, why this thread's last sbn_random_tape_new was.
 *
 * Draw plans.  Each fills `out` exactly as the matching prove call documents its rnd, with the reference's labels in the reference's order, and
 * advances the tape by those draws.  out_scalars is the caller's count and must equal the plan's, which is the one the matching *_sizes call gives;
 * a refusal (SBN_EINVAL: a NULL pointer, a shape the *_sizes call refuses, another count) draws nothing and leaves the tape as it was.
 *   sbn_zk_sumcheck_draw_rnd   num_rounds (n + 4), n = 4 (r1cs) or 3 (quad): blinds_poly[num_rounds], blinds_evals[num_rounds] (sumcheck.rs:483-484,
 *                              :673-674), then per round d_vec[n], r_delta, r_beta (nizk/mod.rs:326-328)
 *   sbn_polyeval_draw_rnd      3 + 2 lg, lg = the right half of sbn_factored_lens(ell): d, r_delta, r_beta, blinds_vec (nizk/mod.rs:458-464).  Two things
 *                              are the reference's and are kept: r_beta is drawn under the label b"r_delta" (:460), and blinds_vec_1[lg] is drawn whole,
 *                              then blinds_vec_2[lg], while rnd stores them as (v1[i], v2[i]) pairs
 *   sbn_r1cs_proof_draw_rnd    sbn_r1cs_proof_sizes' count: poly_blinds[L] (r1csproof.rs:225), phase 1, Az_blind, Bz_blind, Cz_blind, prod_Az_Bz_blind
 *                              (:318-321), t1, t2 (nizk/mod.rs:44-45), b1 .. b5 (:181-185), r (:108), phase 2, blind_eval (r1csproof.rs:410), the opening, r
 *   sbn_sparse_eval_draw_rnd   sbn_sparse_eval_sizes' / _kzg_sizes' count (kzg = 0 / 1): the openings of derefs (Hyrax build only), ops, mem
 *   sbn_snark_draw_rnd         sbn_snark_sizes' count: the R1CS proof's draws, then the sparse proof's, from ONE tape (name b"snark_proof")
 *   sbn_nizk_draw_rnd          sbn_nizk_sizes' count: the R1CS proof's draws (name b"proof") */
#define SBN_EOS (-6)               /* the operating system refused a request (getrandom) */
typedef struct sbn_random_tape sbn_random_tape;
int sbn_random_tape_new(const uint8_t* name, size_t name_len, const uint8_t* init /* 32 bytes, or NULL */, sbn_random_tape** out);
int sbn_random_tape_scalars(sbn_random_tape* tape, const uint8_t* label, size_t label_len, size_t n, uint8_t* out);
void sbn_random_tape_free(sbn_random_tape* tape);
const char* sbn_random_tape_last_error(const sbn_random_tape* tape);
int sbn_zk_sumcheck_draw_rnd(size_t num_rounds, size_t n, sbn_random_tape* tape, uint8_t* out, size_t out_scalars);
int sbn_polyeval_draw_rnd(size_t ell, sbn_random_tape* tape, uint8_t* out, size_t out_scalars);
int sbn_r1cs_proof_draw_rnd(size_t num_cons, size_t num_vars, sbn_random_tape* tape, uint8_t* out, size_t out_scalars);
int sbn_sparse_eval_draw_rnd(size_t num_vars_x, size_t num_vars_y, size_t num_ops /* N */, size_t batch, int kzg, sbn_random_tape* tape, uint8_t* out,
                             size_t out_scalars);
int sbn_snark_draw_rnd(const sbn_snark_key* key, int kzg, sbn_random_tape* tape, uint8_t* out, size_t out_scalars);
int sbn_nizk_draw_rnd(const sbn_nizk_inst* inst, sbn_random_tape* tape, uint8_t* out, size_t out_scalars);

/* ---- the KZG SRS as a file buffer: KZGSrs::load_from_file / save_to_file / load_or_generate (kzg.rs:66-115), and a consistency check ----
 * The file is what #[derive(CanonicalSerialize)] writes for KZGSrs { powers_g1, tau_g2, g2 } in compressed mode (ark-serialize 0.5):
 *     n (u64 little-endian) | n x 32 B powers, each as sbn_g1_compress writes it | tau_g2 64 B | g2 64 B | anything (ignored)
 * A compressed G2 point is x.c0 then x.c1 (32 B each, little-endian canonical), bit 7 of byte 63 = "y is the larger of y and -y" (Fq2 ordered by c1
 * first, c0 on a tie), bit 6 = identity.
 *
 * sbn_kzg_srs_load: bytes in, resident handles out.  *out_srs is the handle sbn_kzg_srs_upload makes (no h, no duplicate map); *out_g2 and *out_tau_g2
 *   are what sbn_g2_prepare makes of the file's g2 and tau_g2 (both NULL for a prover that never verifies); out_g2_xy (or NULL) receives g2 | tau_g2 as
 *   128-byte canonical points.  The powers go up in chunks of SBN_SRS_CHUNK points (read when the context is created) through pinned staging, the copy
 *   of one chunk beside the square roots of the one before; nothing but the Montgomery affine point is written per point.
 *   Refused with SBN_EINVAL and the reason in sbn_last_error; no handle is left and the stream is drained.  The reference's own refusals: a file shorter
 *   than its length field says, a power with x >= q, with x^3 + 3 not a square or with both flag bits set, a G2 coordinate >= q, both flag bits, a G2 x
 *   with no y on the twist, a G2 point outside the r-torsion.  Beyond the reference: n = 0, an identity among the powers, an identity g2 or tau_g2 (no
 *   SRS has them and every consumer divides by them, in effect).  For a power, *bad_index is the smallest refused index of the whole file and the text
 *   names it; otherwise *bad_index is SIZE_MAX.
 *   SBN_SRS_CHECK in flags runs sbn_kzg_srs_check on what was loaded, with a rho drawn from the OS; an inconsistent file is refused like a bad point.
 *   Without it the file is loaded as the reference loads it: arkworks checks no relation between the points either.
 * sbn_kzg_srs_check: *consistent <- 1 exactly when P_0 = (1, 2) — the G sbn_kzg_verify hard-wires — and e(P_{i+1}, g2) = e(P_i, tau_g2) for all
 *   i < n - 1, the relations batched by the powers of rho: T = sum_i rho^i P_i (one MSM over the handle), A = T - P_0, B = rho T - rho^n P_{n-1},
 *   e(A, g2) e(-B, tau_g2) == 1 (one pairing product).  A false accept has probability at most n / r over rho (Schwartz-Zippel), so the caller draws rho
 *   AFTER the file is fixed.  rho = 0 or rho >= r: SBN_EINVAL.  For n = 1 the check is the P_0 test alone.
 * sbn_kzg_srs_save: the bytes of save_to_file.  out = NULL is the size query: *out_len <- 8 + 32 n + 128.  cap below that: SBN_EINVAL, nothing written.
 *   g2_xy, tau_g2_xy: 128-byte points as sbn_g2_prepare takes them (SBN_POINTS_MONT: ark-ff limbs), refused with SBN_EINVAL where it refuses them.
 *   An all-zero point of the handle is written as the identity (31 zero bytes, 0x40).
 * sbn_kzg_srs_g2_from_tau: host only.  g2 = arkworks' generator of G2, tau_g2 = [tau] g2, as canonical bytes: with sbn_kzg_srs_from_tau and the save,
 *   the "generate" half of load_or_generate for a caller who supplies tau.  tau = 0 or tau >= r: SBN_EINVAL. */
#define SBN_SRS_CHECK 1u
int sbn_kzg_srs_load(sbn_ctx* ctx, const uint8_t* bytes, size_t len, uint32_t flags, sbn_bases** out_srs, sbn_g2_lines** out_g2, sbn_g2_lines** out_tau_g2,
                     uint8_t out_g2_xy[256], size_t* bad_index);
int sbn_kzg_srs_check(sbn_ctx* ctx, const sbn_bases* srs, const sbn_g2_lines* g2, const sbn_g2_lines* tau_g2, const uint8_t rho[32], int* consistent);
int sbn_kzg_srs_save(sbn_ctx* ctx, const sbn_bases* srs, const uint8_t g2_xy[128], const uint8_t tau_g2_xy[128], uint32_t flags, uint8_t* out, size_t cap,
                     size_t* out_len);
int sbn_kzg_srs_g2_from_tau(const uint8_t tau[32], uint8_t out_g2_xy[128], uint8_t out_tau_g2_xy[128]);

/* ---- a powers-of-tau ceremony file (.ptau, what circom users hold) as the KZG SRS: an SRS whose tau nobody knows ----
 * The format, all integers little-endian (written from a description; NOT compared with a file snarkjs wrote):
 *     "ptau" | u32 version = 1 | u32 nSections | nSections x ( u32 id | u64 size | size bytes )
 *     section 1 (44 B)   u32 n8 = 32 | n8 bytes q = BN254's base prime | u32 power (1 .. 28) | u32 ceremonyPower
 *     section 2 (tauG1)  2^(power+1) - 1 points of 64 B: x | y;  point i = [tau^i] G1
 *     section 3 (tauG2)  2^power points of 128 B: x.c0 | x.c1 | y.c0 | y.c1;  point i = [tau^i] G2; only points 0 and 1 are read
 *   A coordinate is 32 bytes of v 2^256 mod q: the limbs SBN_POINTS_MONT means.  A point of all zero bytes is the identity.  Sections come in any order;
 *   ids other than 1, 2, 3 are skipped (a real file has 4 .. 7, a prepared one 12 .. 15); a second section 1, 2 or 3 is refused; the sizes of sections
 *   1, 2 and 3 must be exactly the values above.
 * sbn_ptau_scan: host only, no context.  Walks the section table, every offset and size checked against len without overflow, and reads section 1; no
 *   point is touched.  off_g1 / off_g2 are the byte offsets of the first point of sections 2 / 3 in `bytes`.  SBN_EINVAL: a NULL pointer, or a file the
 *   load below would refuse before it reads a point.
 * sbn_kzg_srs_load_ptau: the first n powers (n = 0: all n_g1 of them; n > n_g1: SBN_EINVAL) and tauG2[0], tauG2[1] -> the three handles and out_g2_xy of
 *   sbn_kzg_srs_load, with its outputs and refusal conventions: the reason in sbn_last_error, *bad_index the smallest refused index of the first n powers or
 *   SIZE_MAX, no handle left, the stream drained.  For one tau and n the handle is byte for byte the one sbn_kzg_srs_from_tau and sbn_kzg_srs_load make.
 *   Read: the header, the section table, section 1, the first 64 n bytes of section 2 and the first 256 bytes of section 3 — a caller who has mapped a
 *   32 GiB file pays for that prefix only (the whole of `len` must still cover every section the table names).
 *   Every point is validated on the device (k_ptau_points, the chunks and staging of sbn_kzg_srs_load): both residues < q, not the all-zero point,
 *   y^2 = x^3 + 3; each coordinate changes Montgomery form with one field product; no square root.  The two G2 points are taken out of Montgomery form on
 *   the host and go through every refusal of sbn_g2_prepare (>= q, the identity, off the twist, outside the r-torsion).
 *   SBN_SRS_CHECK in flags runs sbn_kzg_srs_check on what was loaded, exactly as in sbn_kzg_srs_load.  The ceremony's contribution chain is not verified. */
typedef struct { uint32_t power, ceremony_power; uint64_t n_g1, n_g2, off_g1, off_g2; } sbn_ptau_info;
int sbn_ptau_scan(const uint8_t* bytes, size_t len, sbn_ptau_info* out);
int sbn_kzg_srs_load_ptau(sbn_ctx* ctx, const uint8_t* bytes, size_t len, size_t n, uint32_t flags, sbn_bases** out_srs, sbn_g2_lines** out_g2,
                          sbn_g2_lines** out_tau_g2, uint8_t out_g2_xy[256], size_t* bad_index);

/* ---- per-kernel timing (HIP events on the context's stream), for bench.py's roofline line ---- */
int sbn_prof_enable(sbn_ctx* ctx, int on);
int sbn_prof_reset(sbn_ctx* ctx);
/* number of distinct kernel names seen; i-th name, summed ms and launch count */
int sbn_prof_count(sbn_ctx* ctx);
int sbn_prof_get(sbn_ctx* ctx, int i, const char** name, double* total_ms, uint64_t* launches);
/* shape of the context's most recent bucket job (an MSM or a row commit): out = {window bits c, windows W, (digit, point)
 * slots = mixed additions when no digit is zero, buckets}; bench.py prices the accumulate kernel against the ALU roofline with it */
int sbn_prof_last_job(sbn_ctx* ctx, uint64_t out[4]);
/* accumulate / reduction geometry of the context's most recent BUCKET job: out = {segment length SEG, lanes per bucket LPB (k_acc_first<LPB>),
 * buckets per lane L of k_reduce_l1, chunks per problem, k_reduce_combine launches, 1 if they were the quad kernel, and the device counters
 * extra_count (segments past the first, over all buckets) and big_count (buckets with more than SEG entries)}.  The call synchronises the
 * context's stream to read the two counters; the MSM path itself stores six integers and reads nothing back.  A job that took the lookup
 * table (sbn_bases_precompute) runs no bucket kernels and leaves these values as the last bucket job set them (all zero before the first).
 * SBN_EINVAL on a null context or a null out. */
int sbn_prof_last_acc(sbn_ctx* ctx, uint64_t out[8]);

/* host microseconds of the context's most recent opening: {a_vec = R computed on the host beside the first commit, the wait for that
 * commit behind it, Cx + Cy + the n a_vec messages absorbed into the transcript} */
int sbn_prof_last_polyeval(sbn_ctx* ctx, double out_us[3]);

#ifdef __cplusplus
}
#endif
#endif
