// abi_nizk.inc — C ABI: the reference's NIZK mode (snark.rs:162-287) in one call each — NIZKGens::new, Instance::new, Instance::is_sat, NIZK::prove and
// NIZK::verify.  No preprocessing: there is no dense representation and no commitment, and the verifier holds the matrices.  Nothing here launches a
// kernel of its own: every call runs the bodies of the calls that already hold its parts, under ONE hold of the context's mutex and on ONE working copy
// of the caller's transcript:
//   gens      the first three sets of sbn_snark_gens_new (R1CSGens::new under "gens_r1cs_sat"), as a sbn_snark_gens whose eval sets are null
//   instance  snark_host.hpp's shape rules and column shift (abi_snark.inc: snark_convert), sbn_r1cs_upload, a copy of the caller's digest bytes
//   is_sat    r1cs_is_sat_locked (abi_r1cs.inc)
//   prove     the two prefix lines (snark_host.hpp: nizk_prefix), Assignment::pad on the device, r1cs_proof_locked; the proof is its bytes | rx | ry
//   verify    the two prefix lines, r1cs_evaluate_locked at the CLAIMED (rx, ry) over the handle's own matrices, r1cs_verify_locked with those three
//             values, then the (rx, ry) it derived against the claimed ones: the reference's assert_eq! (snark.rs:280-281) is a refusal here
// The digest (R1CSShape::get_digest, zlib over bincode, r1cs.rs:97-101) is never computed: NIZK::prove and ::verify only append inst.digest
// (snark.rs:213, :253), and the caller has those bytes.  Included by sbn254.hip behind abi_snark.inc.

struct sbn_nizk_inst {
  sbn_host::snark::Shape sh;
  sbn_r1cs* inst = nullptr;
  std::vector<uint8_t> digest;                                                    // the caller's inst.digest, opaque
};

// the R1CS proof's shape and the sizes of the whole, for a handle; false: outside what the proof takes
struct NizkShapes { R1csProofShape r; sbn_host::snark::NizkSizes z; };
static bool nizk_shapes(const sbn_nizk_inst* k, NizkShapes* s) {
  if (!r1cs_proof_shape(k->sh.nc, k->sh.nv, &s->r)) return false;
  s->z = sbn_host::snark::nizk_sizes(k->sh);
  // snark_host.hpp counts the layout on its own (it is built without this file): the proof's own numbers decide
  return s->z.rnd_scalars == s->r.rnd_scalars && s->z.r1cs_proof == s->r.proof_bytes && k->sh.nx == s->r.nx && k->sh.ny == s->r.ny;
}

// the three sets R1CSProof::prove / ::verify take, against the handle's shape: an NIZK bundle or a whole SNARK bundle, before any launch
static int nizk_gens_check(sbn_ctx* c, const char* pfx, const sbn_snark_gens* g, const R1csProofShape& r) {
  const struct { int which; size_t n; const char* name; } want[3] = {{SNARK_PC, r.R + 1, "gens_pc"}, {SNARK_G3, 3, "gens_3"}, {SNARK_G4, 4, "gens_4"}};
  for (const auto& w : want) {
    const sbn_bases* b = g->g[w.which];
    if (!b || b->n != w.n || !b->has_h)
      return fail(c, SBN_EINVAL, "%s: %s has %zu points, the instance's shape (2^%zu x 2^%zu) needs %zu with h: make the bundle with the circuit's sizes  [snark.rs:169-180]",
                  pfx, w.name, b ? b->n : (size_t)0, r.nx, r.ell, w.n);
  }
  return SBN_OK;
}

// Instance::is_sat's own checks (snark.rs:142-147) in front of the witness check's
static int nizk_witness_check(sbn_ctx* c, const char* pfx, const sbn_nizk_inst* k, const sbn_table* vars, const uint8_t* input, size_t num_inputs) {
  if (num_inputs != k->sh.num_inputs) return fail(c, SBN_EINVAL, "%s: %zu inputs, the instance has %zu  [snark.rs:145 InvalidNumberOfInputs]", pfx, num_inputs, k->sh.num_inputs);
  return r1cs_is_sat_check(c, k->inst, vars, input, num_inputs);
}

extern "C" {

int sbn_nizk_gens_new(sbn_ctx* c, size_t num_cons, size_t num_vars, size_t num_inputs, sbn_snark_gens** out) {
  if (!c || !out) return SBN_EINVAL;
  *out = nullptr;
  sbn_host::snark::Shape sh;
  if (!sbn_host::snark::shape_make(num_cons, num_vars, num_inputs, &sh)) return fail(c, SBN_EINVAL, "nizk gens: shape %zu x %zu, %zu inputs is too large", num_cons, num_vars, num_inputs);
  return snark_gens_make(c, "nizk gens", sh, 1, 3, out);
}

int sbn_nizk_instance_new(sbn_ctx* c, size_t num_cons, size_t num_vars, size_t num_inputs, const uint32_t* const* rows, const uint32_t* const* cols, const uint8_t* const* vals,
                          const size_t* nnz, uint32_t flags, const uint8_t* digest, size_t digest_len, sbn_nizk_inst** out) {
  if (!c || !rows || !cols || !vals || !nnz || (!digest && digest_len) || !out) return SBN_EINVAL;
  *out = nullptr;
  namespace sn = sbn_host::snark;
  if (flags & ~SBN_SCALARS_MONT) return fail(c, SBN_EINVAL, "nizk instance: unknown flags %#x", flags);
  if (digest_len > UINT32_MAX) return fail(c, SBN_EINVAL, "nizk instance: a digest of %zu bytes: a transcript message has a 32-bit length", digest_len);
  sn::Shape sh;
  if (!sn::shape_make(num_cons, num_vars, num_inputs, &sh)) return fail(c, SBN_EINVAL, "nizk instance: shape %zu x %zu, %zu inputs is too large", num_cons, num_vars, num_inputs);
  if (sh.nv < 2) return fail(c, SBN_EINVAL, "nizk instance: num_vars = %zu pads to %zu: the opening of the witness needs at least one variable  [hyrax.rs:77]", num_vars, sh.nv);
  std::vector<uint32_t> nc_[3];
  const uint32_t* ncols[3];
  int rc = snark_convert(c, "nizk instance", sh, rows, cols, vals, nnz, nc_, ncols);
  if (rc) return rc;
  sbn_nizk_inst* k = new sbn_nizk_inst();
  k->sh = sh;
  if (digest_len) k->digest.assign(digest, digest + digest_len);
  NizkShapes s;
  if (!nizk_shapes(k, &s)) { delete k; return fail(c, SBN_EINVAL, "nizk instance: shape %zu x %zu is outside what the proof takes", sh.nc, sh.nv); }
  if ((rc = sbn_r1cs_upload(c, sh.nc, sh.nv, rows, ncols, vals, nnz, flags, &k->inst))) { delete k; return rc; }
  *out = k;
  return SBN_OK;
}

void sbn_nizk_instance_free(sbn_ctx* c, sbn_nizk_inst* k) {
  if (!k) return;
  if (k->inst) sbn_r1cs_free(c, k->inst);
  delete k;
}

const sbn_r1cs* sbn_nizk_instance_r1cs(const sbn_nizk_inst* k) { return k ? k->inst : nullptr; }

int sbn_nizk_sizes(const sbn_nizk_inst* k, size_t* rnd_scalars, size_t* proof_bytes) {
  NizkShapes s;
  if (!k || !nizk_shapes(k, &s)) return SBN_EINVAL;
  if (rnd_scalars) *rnd_scalars = s.z.rnd_scalars;
  if (proof_bytes) *proof_bytes = s.z.proof_bytes;
  return SBN_OK;
}

int sbn_nizk_is_sat(sbn_ctx* c, const sbn_nizk_inst* k, const sbn_table* vars, const uint8_t* input, size_t num_inputs, int* sat, uint64_t* num_bad, uint64_t* first_bad) {
  if (!c || !k || !vars || (!input && num_inputs) || !sat || !num_bad || !first_bad) return SBN_EINVAL;
  int rc;
  if ((rc = nizk_witness_check(c, "nizk is_sat", k, vars, input, num_inputs))) return rc;
  std::lock_guard<std::mutex> g(c->mu); hipSetDevice(c->device);
  int s = 0; uint64_t nb = 0, fb = 0;
  if ((rc = r1cs_is_sat_locked(c, k->inst, vars, input, num_inputs, &s, &nb, &fb))) return rc;
  *sat = s; *num_bad = nb; *first_bad = fb;
  return SBN_OK;
}

int sbn_nizk_prove(sbn_ctx* c, const sbn_nizk_inst* k, const sbn_table* vars, const uint8_t* input, size_t num_inputs, const sbn_snark_gens* gens, uint32_t flags,
                   const uint8_t* rnd, sbn_transcript* tr, uint8_t* out_proof) {
  if (!c || !k || !vars || (!input && num_inputs) || !gens || !rnd || !tr || !out_proof) return SBN_EINVAL;
  const char* pfx = "nizk prove";
  int rc;
  if (flags & ~SBN_SNARK_CHECK_SAT) return fail(c, SBN_EINVAL, "%s: unknown flags %#x", pfx, flags);
  if ((rc = nizk_witness_check(c, pfx, k, vars, input, num_inputs))) return rc;
  NizkShapes s;
  if (!nizk_shapes(k, &s)) return fail(c, SBN_EINVAL, "%s: the instance's shape is outside what the proof takes", pfx);
  if ((rc = nizk_gens_check(c, pfx, gens, s.r))) return rc;
  for (size_t i = 0; i < s.z.rnd_scalars; i++) if (!fr_canonical(rnd + 32 * i)) return fail(c, SBN_EINVAL, "%s: rnd[%zu] is not canonical  [scalar.rs:87-95]", pfx, i);
  std::lock_guard<std::mutex> g(c->mu); hipSetDevice(c->device);
  if (flags & SBN_SNARK_CHECK_SAT) {                                              // before any proving launch
    int sat = 0; uint64_t nb = 0, fb = 0;
    if ((rc = r1cs_is_sat_locked(c, k->inst, vars, input, num_inputs, &sat, &nb, &fb))) return rc;
    if (!sat) return fail(c, SBN_EUNSAT, "%s: the witness violates %llu constraints, the first is row %llu", pfx, (unsigned long long)nb, (unsigned long long)fb);
  }
  std::vector<uint8_t> proof(s.z.proof_bytes);                                    // the caller's buffer is written only by a call that succeeded
  rc = prove_on_copy(c, tr, [&](sbn_host::MerlinTranscript& t) -> int {
    int rc2;
    TableScope T(c);
    sbn_host::Script ts{t};
    sbn_host::snark::nizk_prefix(ts, k->digest.data(), k->digest.size());         // snark.rs:212-213
    const sbn_table* pv = nullptr;
    if ((rc2 = r1cs_pad_vars(c, T, vars, k->inst->nv, &pv))) return rc2;          // :216-223
    uint8_t* rx = proof.data() + s.z.r1cs_proof;                                  // r: (rx, ry) behind r1cs_sat_proof (:191-194)
    if ((rc2 = r1cs_proof_locked(c, k->inst, pv, input, num_inputs, gens->g[SNARK_PC], gens->g[SNARK_G3], gens->g[SNARK_G4], s.r, rnd, t, proof.data(), rx, rx + 32 * s.r.nx))) return rc2;
    return T.done();
  });
  if (rc) return rc;
  memcpy(out_proof, proof.data(), proof.size());
  return SBN_OK;
}

int sbn_nizk_verify(sbn_ctx* c, const sbn_nizk_inst* k, const uint8_t* input, size_t num_inputs, const sbn_snark_gens* gens, const uint8_t* proof, size_t proof_len,
                    sbn_transcript* tr, int* accepted) {
  if (!c || !k || (!input && num_inputs) || !gens || !proof || !tr || !accepted) return SBN_EINVAL;
  const char* pfx = "nizk verify";
  int rc;
  NizkShapes s;
  if (!nizk_shapes(k, &s)) return fail(c, SBN_EINVAL, "%s: the instance's shape is outside what the check takes", pfx);
  if (proof_len != s.z.proof_bytes) return fail(c, SBN_EINVAL, "%s: the proof has %zu bytes, the instance's shape gives %zu", pfx, proof_len, s.z.proof_bytes);
  if (num_inputs != k->sh.num_inputs) return fail(c, SBN_EINVAL, "%s: %zu inputs, the instance has %zu  [snark.rs:262 assert_eq]", pfx, num_inputs, k->sh.num_inputs);
  for (size_t i = 0; i < num_inputs; i++) if (!fr_canonical(input + 32 * i)) return fail(c, SBN_EINVAL, "%s: input[%zu] is not canonical  [scalar.rs:87-95]", pfx, i);
  if ((rc = nizk_gens_check(c, pfx, gens, s.r))) return rc;
  const size_t nx = s.r.nx, ny = s.r.ny;
  const uint8_t* claimed_rx = proof + s.z.r1cs_proof;
  const uint8_t* claimed_ry = claimed_rx + 32 * nx;
  std::lock_guard<std::mutex> g(c->mu); hipSetDevice(c->device);
  return verify_on_copy(c, tr, accepted, [&](sbn_host::MerlinTranscript& t) -> int {
    for (size_t i = 0; i < nx + ny; i++) if (!fr_canonical(claimed_rx + 32 * i)) return SBN_OK;      // r is the prover's: Scalar::from_bytes fails (scalar.rs:87-95)
    sbn_host::Script ts{t};
    sbn_host::snark::nizk_prefix(ts, k->digest.data(), k->digest.size());         // snark.rs:252-253
    uint8_t evals[96];
    std::vector<uint8_t> rx(32 * nx), ry(32 * ny);
    int rc2, ok = 0;
    if ((rc2 = r1cs_evaluate_locked(c, k->inst, claimed_rx, nx, claimed_ry, ny, evals))) return rc2;      // :257-258: at the point the proof claims
    if ((rc2 = r1cs_verify_locked(c, s.r, input, num_inputs, evals, gens->g[SNARK_PC], gens->g[SNARK_G3], gens->g[SNARK_G4], proof, t, rx.data(), ry.data(), &ok))) return rc2;
    if (!ok) return SBN_OK;                                                       // :271-277
    // :280-281: the point the transcript gives against the claimed one.  The reference panics; a proof is the prover's data, so this is a refusal
    if (memcmp(rx.data(), claimed_rx, 32 * nx) || memcmp(ry.data(), claimed_ry, 32 * ny)) return SBN_OK;
    *accepted = 1;
    return SBN_OK;
  });
}

}  // extern "C"
