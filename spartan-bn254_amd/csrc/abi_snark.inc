// abi_snark.inc — C ABI: the reference's public surface (snark.rs:59-158, :290-529) in one call each — SNARKGens::new, Instance::new + SNARK::encode,
// Instance::is_sat, SNARK::prove and SNARK::verify, for the Hyrax and the KZG build.  Nothing here launches a kernel of its own: every call runs the
// bodies of the calls that already hold its parts, under ONE hold of the context's mutex and on ONE working copy of the caller's transcript:
//   encode   snark_host.hpp's shape rules and column shift, sbn_r1cs_upload, sbn_dense_build(nx, ny), the two commits of sbn_commit_table with no blinds
//            (sparse_eval_commit over the first R generators), sbn_g1_compress, the commitment bytes, the two commitments as resident point sets
//   is_sat   r1cs_is_sat_locked (abi_r1cs.inc)
//   prove    the prefix (snark_host.hpp), Assignment::pad on the device, r1cs_proof_locked, r1cs_evaluate_locked at the (rx, ry) it returned,
//            sparse_eval_locked — rnd is ONE tape, the sat half's draws, then the eval half's
//   verify   the prefix, r1cs_verify_locked with the proof's own inst_evals, sparse_verify_locked at the (rx, ry) it returned (skipped behind a refusal);
//            the KZG build's pairing check follows behind the mutex' release, as in sbn_sparse_eval_verify_kzg
// A key from sbn_snark_key_from_comm holds the verifier's half only: the shape and the two commitments.  snark_gens_make and snark_convert serve NIZK mode
// too (abi_nizk.inc).  Included by sbn254.hip.

struct sbn_snark_gens {
  sbn_bases* g[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};      // pc, g3, g4, ops, mem, derefs
  size_t nc = 0, nv = 0, N = 0;                                                  // the padded shape and npo2(num_nz_entries) they were made for
};
struct sbn_snark_key {
  sbn_host::snark::Comm cm;
  std::vector<uint8_t> comm;                                                      // R1CSCommitment's bytes
  sbn_r1cs* inst = nullptr; sbn_dense* dense = nullptr;                           // the prover's half: null on a key made of commitment bytes
  sbn_bases *comm_ops = nullptr, *comm_mem = nullptr;                             // the two PolyCommitments as resident point sets
};
enum { SNARK_PC = 0, SNARK_G3, SNARK_G4, SNARK_OPS, SNARK_MEM, SNARK_DEREFS };

static void snark_key_release(sbn_ctx* c, sbn_snark_key* k) {
  if (!k) return;
  if (k->dense) sbn_dense_free(c, k->dense);
  if (k->inst) sbn_r1cs_free(c, k->inst);
  if (k->comm_ops) sbn_bases_free(c, k->comm_ops);
  if (k->comm_mem) sbn_bases_free(c, k->comm_mem);
  delete k;
}

// the shapes of the two halves and the sizes of the whole, for a key; false: outside what the two halves take
struct SnarkShapes { R1csProofShape r; SparseEvalShape e; sbn_host::snark::Sizes z; };
static bool snark_shapes(const sbn_snark_key* k, bool kzg, SnarkShapes* s) {
  if (!r1cs_proof_shape((size_t)k->cm.nc, (size_t)k->cm.nv, &s->r) || !sparse_eval_shape(k->cm.nx, k->cm.ny, (size_t)k->cm.N, (size_t)k->cm.batch, &s->e)) return false;
  s->z = sbn_host::snark::sizes(k->cm, kzg);
  // snark_host.hpp counts the two layouts on its own (it is built without this file): the halves' own numbers decide
  return s->z.r1cs_rnd == s->r.rnd_scalars && s->z.r1cs_proof == s->r.proof_bytes && s->z.eval_rnd == (kzg ? s->e.rnd_scalars_kzg : s->e.rnd_scalars) &&
         s->z.eval_proof == (kzg ? s->e.proof_bytes_kzg : s->e.proof_bytes) && s->e.cells == (size_t)k->cm.cells;
}

// the generator handles against the key's shape: what sbn_r1cs_proof_prove / _verify and sbn_sparse_eval_prove / _verify check, before any launch
static int snark_gens_check(sbn_ctx* c, const char* pfx, const sbn_snark_gens* g, const SnarkShapes& s, bool kzg) {
  const struct { int which; size_t n; const char* name; } want[6] = {{SNARK_PC, s.r.R + 1, "gens_pc"}, {SNARK_G3, 3, "gens_3"}, {SNARK_G4, 4, "gens_4"},
    {SNARK_OPS, ((size_t)1 << s.e.lg_o) + 1, "gens_ops"}, {SNARK_MEM, ((size_t)1 << s.e.lg_m) + 1, "gens_mem"}, {SNARK_DEREFS, ((size_t)1 << s.e.lg_d) + 1, "gens_derefs"}};
  for (const auto& w : want) {
    if (kzg && w.which == SNARK_DEREFS) continue;
    const sbn_bases* b = g->g[w.which];
    if (!b || b->n != w.n || !b->has_h)
      return fail(c, SBN_EINVAL, "%s: %s has %zu points, the key's shape (2^%zu x 2^%zu, N = %zu) needs %zu with h: make the bundle with the circuit's sizes and its largest nnz  [snark.rs:305-328]",
                  pfx, w.name, b ? b->n : (size_t)0, s.r.nx, s.r.ell, s.e.N, w.n);
  }
  return SBN_OK;
}

// the first `nsets` of SNARKGens::new's six sets: 6 is the whole bundle, 3 is R1CSGens::new alone, which is all NIZKGens::new makes (snark.rs:169-180);
// the eval sets of such a bundle stay null and N is not looked at
static int snark_gens_make(sbn_ctx* c, const char* pfx, const sbn_host::snark::Shape& sh, size_t N, int nsets, sbn_snark_gens** out) {
  namespace sn = sbn_host::snark;
  const size_t ell = sn::log2u(sh.nv), e_o = sn::ell_ops(N), e_m = std::max(sh.nx, sh.ny) + 1, e_d = sn::log2u(N) + sn::log2u(sn::npo2(2 * (size_t)sn::BATCH));
  if ((nsets == 6 ? std::max(std::max(ell, e_o), std::max(e_m, e_d)) : ell) > 2 * (size_t)PE_SIDE_MAX) return fail(c, SBN_EINVAL, "%s: the shape is outside what the openings take", pfx);
  auto R = [](size_t e) { return (size_t)1 << (e - e / 2); };                   // 2^right of compute_factored_lens
  static const char SAT[] = "gens_r1cs_sat", EVAL[] = "gens_r1cs_eval";          // snark.rs:321-322
  const struct { size_t n; const char* label; } want[6] = {{R(ell) + 1, SAT}, {3, SAT}, {4, SAT},      // R1CSGens::new, r1csproof.rs:177-182 (gens_1 is gens_pc's)
                                                           {R(e_o) + 1, EVAL}, {R(e_m) + 1, EVAL}, {R(e_d) + 1, EVAL}};      // sparse_mlpoly_full.rs:612-630
  sbn_snark_gens* g = new sbn_snark_gens();
  g->nc = sh.nc; g->nv = sh.nv; g->N = nsets == 6 ? N : 0;
  for (int k = 0; k < nsets; k++) {
    const int rc = sbn_gens_new(c, want[k].n, (const uint8_t*)want[k].label, strlen(want[k].label), nullptr, &g->g[k]);
    if (rc) { for (int j = 0; j < k; j++) sbn_bases_free(c, g->g[j]); delete g; return rc; }
  }
  *out = g;
  return SBN_OK;
}

// Instance::new's convert (snark.rs:92-110) on the three raw matrices: ncols[m] <- the columns of the padded instance, held by store[m]
static int snark_convert(sbn_ctx* c, const char* pfx, const sbn_host::snark::Shape& sh, const uint32_t* const* rows, const uint32_t* const* cols, const uint8_t* const* vals,
                         const size_t* nnz, std::vector<uint32_t> store[3], const uint32_t* ncols[3]) {
  namespace sn = sbn_host::snark;
  const size_t live = sh.num_vars + 1 + sh.num_inputs;
  for (int m = 0; m < 3; m++) {
    if (nnz[m] && (!rows[m] || !cols[m] || !vals[m])) return fail(c, SBN_EINVAL, "%s: matrix %d has %zu entries and a NULL array", pfx, m, nnz[m]);
    store[m].resize(std::max<size_t>(nnz[m], 1));
    size_t bad = 0;
    const int e = sn::convert_cols(sh, rows[m], cols[m], vals[m], nnz[m], store[m].data(), &bad);
    if (e == sn::CONV_ROW) return fail(c, SBN_EINVAL, "%s: matrix %d entry %zu: row %u >= num_cons %zu  [snark.rs:95 InvalidIndex]", pfx, m, bad, rows[m][bad], sh.num_cons);
    if (e == sn::CONV_COL) return fail(c, SBN_EINVAL, "%s: matrix %d entry %zu: col %u >= num_vars + 1 + num_inputs = %zu  [snark.rs:98 InvalidIndex]", pfx, m, bad, cols[m][bad], live);
    if (e == sn::CONV_VAL) return fail(c, SBN_EINVAL, "%s: matrix %d entry %zu: value >= r  [snark.rs:101 InvalidScalar]", pfx, m, bad);
    ncols[m] = store[m].data();
  }
  return SBN_OK;
}
static int snark_encode_finish(sbn_ctx* c, sbn_snark_key* k, const sbn_host::snark::Shape& sh, const sbn_snark_gens* gens, sbn_snark_key** out);

extern "C" {

int sbn_snark_gens_new(sbn_ctx* c, size_t num_cons, size_t num_vars, size_t num_inputs, size_t num_nz_entries, sbn_snark_gens** out) {
  if (!c || !out) return SBN_EINVAL;
  *out = nullptr;
  namespace sn = sbn_host::snark;
  sn::Shape sh;
  if (!sn::shape_make(num_cons, num_vars, num_inputs, &sh) || num_nz_entries > ((size_t)1 << 31))
    return fail(c, SBN_EINVAL, "snark gens: shape %zu x %zu, %zu inputs, %zu non-zeros is too large", num_cons, num_vars, num_inputs, num_nz_entries);
  return snark_gens_make(c, "snark gens", sh, sn::npo2(num_nz_entries), 6, out);
}
const sbn_bases* sbn_snark_gens_get(const sbn_snark_gens* g, int which) { return (g && which >= 0 && which < 6) ? g->g[which] : nullptr; }
void sbn_snark_gens_free(sbn_ctx* c, sbn_snark_gens* g) {
  if (!g) return;
  for (sbn_bases* b : g->g) if (b) sbn_bases_free(c, b);
  delete g;
}

void sbn_snark_key_free(sbn_ctx* c, sbn_snark_key* k) { snark_key_release(c, k); }

int sbn_snark_encode(sbn_ctx* c, size_t num_cons, size_t num_vars, size_t num_inputs, const uint32_t* const* rows, const uint32_t* const* cols, const uint8_t* const* vals,
                     const size_t* nnz, uint32_t flags, const sbn_snark_gens* gens, sbn_snark_key** out) {
  if (!c || !rows || !cols || !vals || !nnz || !gens || !out) return SBN_EINVAL;
  *out = nullptr;
  namespace sn = sbn_host::snark;
  if (flags & ~SBN_SCALARS_MONT) return fail(c, SBN_EINVAL, "snark encode: unknown flags %#x", flags);
  sn::Shape sh;
  if (!sn::shape_make(num_cons, num_vars, num_inputs, &sh)) return fail(c, SBN_EINVAL, "snark encode: shape %zu x %zu, %zu inputs is too large", num_cons, num_vars, num_inputs);
  if (sh.nv < 2) return fail(c, SBN_EINVAL, "snark encode: num_vars = %zu pads to %zu: the opening of the witness needs at least one variable  [hyrax.rs:77]", num_vars, sh.nv);
  std::vector<uint32_t> nc_[3];
  const uint32_t* ncols[3];
  int rc = snark_convert(c, "snark encode", sh, rows, cols, vals, nnz, nc_, ncols);
  if (rc) return rc;
  if (gens->nc != sh.nc || gens->nv != sh.nv) return fail(c, SBN_EINVAL, "snark encode: the generator bundle was made for %zu x %zu, the instance pads to %zu x %zu", gens->nc, gens->nv, sh.nc, sh.nv);
  sbn_snark_key* k = new sbn_snark_key();
  rc = sbn_r1cs_upload(c, sh.nc, sh.nv, rows, ncols, vals, nnz, flags, &k->inst);
  if (rc == SBN_OK) rc = sbn_dense_build(c, sh.nx, sh.ny, rows, ncols, vals, nnz, (size_t)sn::BATCH, flags, &k->dense);
  if (rc) { snark_key_release(c, k); return rc; }
  return snark_encode_finish(c, k, sh, gens, out);
}

}  // extern "C"

// SNARK::encode behind the two resident halves (k->inst, k->dense): the N >= 2 rule, the two commitments, the commitment's bytes.  Takes the key over:
// *out <- k, or k is released.  Shared by sbn_snark_encode and sbn_snark_encode_circom (abi_circom.inc)
static int snark_encode_finish(sbn_ctx* c, sbn_snark_key* k, const sbn_host::snark::Shape& sh, const sbn_snark_gens* gens, sbn_snark_key** out) {
  namespace sn = sbn_host::snark;
  int rc = SBN_OK;
  const size_t N = k->dense->N;
  if (N < 2) { snark_key_release(c, k); return fail(c, SBN_EINVAL, "snark encode: no matrix has more than one entry (N = %zu): the dot-product circuits cannot be split  [product_tree.rs:89 assert_eq]", N); }
  k->cm = sn::comm_of(sh, N);
  SnarkShapes s;
  if (!snark_shapes(k, false, &s)) { snark_key_release(c, k); return fail(c, SBN_EINVAL, "snark encode: shape (%zu x %zu, N = %zu) is outside what the two proofs take", sh.nc, sh.nv, N); }
  const sbn_bases* g[2] = {gens->g[SNARK_OPS], gens->g[SNARK_MEM]};
  const size_t ells[2] = {s.e.ell_o, s.e.ell_mm};
  const sbn_table* tabs[2] = {&k->dense->ops, &k->dense->mem};
  std::vector<uint8_t> comp[2];
  for (int q = 0; q < 2 && rc == SBN_OK; q++) {
    const size_t L = (size_t)1 << (ells[q] / 2), R = (size_t)1 << (ells[q] - ells[q] / 2);
    if (!g[q] || g[q]->n != R + 1 || !g[q]->has_h) {
      rc = fail(c, SBN_EINVAL, "snark encode: %s has %zu points, N = %zu needs %zu with h: make the bundle with num_nz_entries = the largest nnz  [r1cs.rs:273-274]", q ? "gens_mem" : "gens_ops", g[q] ? g[q]->n : (size_t)0, N, R + 1);
      break;
    }
    std::vector<uint8_t> xy(64 * L);
    {
      std::lock_guard<std::mutex> lk(c->mu); hipSetDevice(c->device);
      const sbn_bases *gn = nullptr, *g1 = nullptr;
      if ((rc = r1cs_proof_gens(c, g[q], R, &gn, &g1)) == SBN_OK) rc = sparse_eval_commit(c, gn, tabs[q], L, R, xy.data());      // DensePolynomial::commit, no blinds (hyrax.rs:283-308)
      if (rc) hipStreamSynchronize(c->stream);
    }
    if (rc) break;
    comp[q].resize(32 * L);
    sbn_g1_compress(xy.data(), L, comp[q].data());
    rc = sbn_bases_upload(c, xy.data(), L, nullptr, 0, q ? &k->comm_mem : &k->comm_ops);
  }
  if (rc) { snark_key_release(c, k); return rc; }
  k->comm = sn::comm_build(k->cm, comp[0].data(), comp[1].data());
  *out = k;
  return SBN_OK;
}

extern "C" {

int sbn_snark_key_from_comm(sbn_ctx* c, const uint8_t* comm, size_t len, sbn_snark_key** out) {
  if (!c || !comm || !out) return SBN_EINVAL;
  *out = nullptr;
  namespace sn = sbn_host::snark;
  static const char* const WHY[] = {"", "shorter than its six u64", "num_cons is no power of two from 2 on", "num_vars is no power of two", "num_inputs >= num_vars", "batch_size != 3",
                                    "num_ops is no power of two from 2 on", "num_mem_cells != 2^max(log2 num_cons, log2(2 num_vars))", "its length does not fit its shape"};
  sbn_snark_key* k = new sbn_snark_key();
  const int e = sn::comm_parse(comm, len, &k->cm);
  if (e != sn::COMM_OK) { delete k; return fail(c, SBN_EINVAL, "snark key: the commitment's bytes are refused: %s", WHY[e]); }
  SnarkShapes s;
  if (k->cm.nv < 2 || !snark_shapes(k, false, &s)) { delete k; return fail(c, SBN_EINVAL, "snark key: the commitment's shape is outside what the two proofs take"); }
  k->comm = sn::comm_build(k->cm, sn::comm_ops(k->cm, comm), sn::comm_mem(k->cm, comm));      // normalised, as the reference's deserialisation leaves the points
  int rc = sbn_bases_from_compressed(c, sn::comm_ops(k->cm, k->comm.data()), k->cm.L_ops, &k->comm_ops, nullptr);
  if (rc == SBN_OK) rc = sbn_bases_from_compressed(c, sn::comm_mem(k->cm, k->comm.data()), k->cm.L_mem, &k->comm_mem, nullptr);
  if (rc) { snark_key_release(c, k); return rc; }                                 // a point that does not decompress: SBN_EINVAL, the commitment is the caller's own data
  *out = k;
  return SBN_OK;
}

int sbn_snark_key_comm(const sbn_snark_key* k, uint8_t* out, size_t cap, size_t* len) {
  if (!k || !len) return SBN_EINVAL;
  *len = k->comm.size();
  if (!out) return SBN_OK;                                                        // the length alone
  if (cap < k->comm.size()) return SBN_EINVAL;
  memcpy(out, k->comm.data(), k->comm.size());
  return SBN_OK;
}

int sbn_snark_sizes(const sbn_snark_key* k, int kzg, size_t* rnd_scalars, size_t* proof_bytes) {
  SnarkShapes s;
  if (!k || !snark_shapes(k, kzg != 0, &s)) return SBN_EINVAL;
  if (rnd_scalars) *rnd_scalars = s.z.rnd_scalars;
  if (proof_bytes) *proof_bytes = s.z.proof_bytes;
  return SBN_OK;
}

}  // extern "C"

// Instance::is_sat's own checks (snark.rs:142-147) in front of the witness check's
static int snark_witness_check(sbn_ctx* c, const char* pfx, const sbn_snark_key* k, const sbn_table* vars, const uint8_t* input, size_t num_inputs) {
  if (!k->inst || !k->dense) return fail(c, SBN_EINVAL, "%s: the key was made of commitment bytes: it holds the verifier's half only", pfx);
  if (num_inputs != (size_t)k->cm.ni) return fail(c, SBN_EINVAL, "%s: %zu inputs, the instance has %zu  [snark.rs:145 InvalidNumberOfInputs]", pfx, num_inputs, (size_t)k->cm.ni);
  return r1cs_is_sat_check(c, k->inst, vars, input, num_inputs);
}

static int snark_prove_entry(sbn_ctx* c, const char* pfx, const sbn_snark_key* k, const sbn_table* vars, const uint8_t* input, size_t num_inputs, const sbn_snark_gens* gens,
                             const sbn_bases* srs, const sbn_derefs_key* dkey, uint32_t flags, const uint8_t* rnd, sbn_transcript* tr, uint8_t* out_proof) {
  const bool kzg = srs != nullptr;
  int rc;
  if (flags & ~SBN_SNARK_CHECK_SAT) return fail(c, SBN_EINVAL, "%s: unknown flags %#x", pfx, flags);
  if ((rc = snark_witness_check(c, pfx, k, vars, input, num_inputs))) return rc;
  SnarkShapes s;
  if (!snark_shapes(k, kzg, &s)) return fail(c, SBN_EINVAL, "%s: the key's shape is outside what the two proofs take", pfx);
  if ((rc = snark_gens_check(c, pfx, gens, s, kzg))) return rc;
  for (size_t i = 0; i < s.z.r1cs_rnd; i++) if (!fr_canonical(rnd + 32 * i)) return fail(c, SBN_EINVAL, "%s: rnd[%zu] is not canonical  [scalar.rs:87-95]", pfx, i);
  const uint8_t* rnd_eval = rnd + 32 * s.z.r1cs_rnd;
  const size_t nx = k->cm.nx, ny = k->cm.ny;
  std::lock_guard<std::mutex> g(c->mu); hipSetDevice(c->device);
  {
    // the eval half's own checks (its rnd among them), with points and evals that are canonical whatever they will be
    const std::vector<uint8_t> zeros(32 * std::max<size_t>(std::max(nx, ny), 3), 0);
    SparseEvalShape e2;
    if ((rc = sparse_eval_check(c, pfx, k->dense, zeros.data(), nx, zeros.data(), ny, zeros.data(), gens->g[SNARK_OPS], gens->g[SNARK_MEM], kzg ? nullptr : gens->g[SNARK_DEREFS], srs, dkey, rnd_eval, &e2))) return rc;
  }
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
    sbn_host::snark::prefix(ts, k->cm, k->comm.data());                           // snark.rs:440-442
    const sbn_table* pv = nullptr;
    if ((rc2 = r1cs_pad_vars(c, T, vars, k->inst->nv, &pv))) return rc2;          // :445-452
    std::vector<uint8_t> rx(32 * nx), ry(32 * ny);
    uint8_t* evals = proof.data() + s.z.r1cs_proof;
    if ((rc2 = r1cs_proof_locked(c, k->inst, pv, input, num_inputs, gens->g[SNARK_PC], gens->g[SNARK_G3], gens->g[SNARK_G4], s.r, rnd, t, proof.data(), rx.data(), ry.data()))) return rc2;
    if ((rc2 = r1cs_evaluate_locked(c, k->inst, rx.data(), nx, ry.data(), ny, evals))) return rc2;      // :465
    if ((rc2 = sparse_eval_locked(c, k->dense, rx.data(), nx, ry.data(), ny, evals, gens->g[SNARK_OPS], gens->g[SNARK_MEM], kzg ? nullptr : gens->g[SNARK_DEREFS], srs, dkey, s.e,
                                  rnd_eval, t, evals + 96))) return rc2;          // :468-476
    return T.done();
  });
  if (rc) return rc;
  memcpy(out_proof, proof.data(), proof.size());
  return SBN_OK;
}

static int snark_verify_entry(sbn_ctx* c, const char* pfx, const sbn_snark_key* k, const uint8_t* input, size_t num_inputs, const sbn_snark_gens* gens,
                              const sbn_g2_lines* g2, const sbn_g2_lines* tau_g2, const uint8_t* proof, size_t proof_len, sbn_transcript* tr, int* accepted) {
  namespace spv = sbn_host::spv;
  const bool kzg = g2 != nullptr;
  int rc;
  SnarkShapes s;
  spv::Layout L;
  if (!snark_shapes(k, kzg, &s) || !spv::layout_make(k->cm.nx, k->cm.ny, (size_t)k->cm.N, (size_t)k->cm.batch, &L, kzg) || L.off[spv::NFIELDS] != s.z.eval_proof)
    return fail(c, SBN_EINVAL, "%s: the key's shape is outside what the two checks take", pfx);
  if (kzg && (g2->ctx != c || tau_g2->ctx != c)) return fail(c, SBN_EINVAL, "%s: a G2 handle of another context", pfx);
  if (proof_len != s.z.proof_bytes) return fail(c, SBN_EINVAL, "%s: the proof has %zu bytes, the key's shape gives %zu", pfx, proof_len, s.z.proof_bytes);
  if (num_inputs != (size_t)k->cm.ni) return fail(c, SBN_EINVAL, "%s: %zu inputs, the commitment has %zu  [snark.rs:501 assert_eq]", pfx, num_inputs, (size_t)k->cm.ni);
  for (size_t i = 0; i < num_inputs; i++) if (!fr_canonical(input + 32 * i)) return fail(c, SBN_EINVAL, "%s: input[%zu] is not canonical  [scalar.rs:87-95]", pfx, i);
  if ((rc = snark_gens_check(c, pfx, gens, s, kzg))) return rc;
  if (!k->comm_ops || !k->comm_mem || k->comm_ops->n != k->cm.L_ops || k->comm_mem->n != k->cm.L_mem) return fail(c, SBN_EINVAL, "%s: the key holds no commitment", pfx);
  const uint8_t* evals = proof + s.z.r1cs_proof;
  const uint8_t* eval_proof = evals + 96;
  const size_t nx = k->cm.nx, ny = k->cm.ny;
  sbn_host::MerlinTranscript t = tr->t;
  SvKzg kz;
  int acc = 0;
  {
    std::lock_guard<std::mutex> g(c->mu); hipSetDevice(c->device);
    rc = [&]() -> int {
      for (int i = 0; i < 3; i++) if (!fr_canonical(evals + 32 * i)) return SBN_OK;      // inst_evals are the prover's: Scalar::from_bytes fails (scalar.rs:87-95)
      sbn_host::Script ts{t};
      sbn_host::snark::prefix(ts, k->cm, k->comm.data());                         // snark.rs:496-498
      std::vector<uint8_t> rx(32 * nx), ry(32 * ny);
      int rc2, ok = 0;
      if ((rc2 = r1cs_verify_locked(c, s.r, input, num_inputs, evals, gens->g[SNARK_PC], gens->g[SNARK_G3], gens->g[SNARK_G4], proof, t, rx.data(), ry.data(), &ok))) return rc2;
      if (!ok) return SBN_OK;                                                     // :504-511: a failed first half skips the second
      return sparse_verify_locked(c, s.e, L, k->comm_ops, k->comm_mem, rx.data(), nx, ry.data(), ny, evals, gens->g[SNARK_OPS], gens->g[SNARK_MEM], kzg ? nullptr : gens->g[SNARK_DEREFS],
                                  eval_proof, t, &acc, kzg ? &kz : nullptr);
    }();
    if (rc != SBN_OK) { hipStreamSynchronize(c->stream); return rc; }
  }
  if (acc && kzg) {                                                               // DerefsEvalProof::verify's pairing check, as sbn_sparse_eval_verify_kzg runs it
    uint8_t comp[64], xy[128], ok[2] = {0, 0};
    memcpy(comp, kz.comm, 32); memcpy(comp + 32, kz.pi, 32);
    if ((rc = sbn_g1_decompress(c, comp, 2, xy, ok))) return rc;
    if (!ok[0] || !ok[1]) acc = 0;
    else {
      static const uint8_t ONE[32] = {1};
      std::vector<uint8_t> pts(xy, xy + 64), scal(ONE, ONE + 32);
      int paired = 0;
      if ((rc = kzg_check_run(c, g2, tau_g2, pts, scal, kz.y, kz.z, xy + 64, &paired))) return rc;
      acc = paired;
    }
  }
  *accepted = acc ? 1 : 0;
  if (acc) tr->t = t;
  return SBN_OK;
}

extern "C" {

int sbn_snark_is_sat(sbn_ctx* c, const sbn_snark_key* k, const sbn_table* vars, const uint8_t* input, size_t num_inputs, int* sat, uint64_t* num_bad, uint64_t* first_bad) {
  if (!c || !k || !vars || (!input && num_inputs) || !sat || !num_bad || !first_bad) return SBN_EINVAL;
  int rc;
  if ((rc = snark_witness_check(c, "snark is_sat", k, vars, input, num_inputs))) return rc;
  std::lock_guard<std::mutex> g(c->mu); hipSetDevice(c->device);
  int s = 0; uint64_t nb = 0, fb = 0;
  if ((rc = r1cs_is_sat_locked(c, k->inst, vars, input, num_inputs, &s, &nb, &fb))) return rc;
  *sat = s; *num_bad = nb; *first_bad = fb;
  return SBN_OK;
}

int sbn_snark_prove(sbn_ctx* c, const sbn_snark_key* k, const sbn_table* vars, const uint8_t* input, size_t num_inputs, const sbn_snark_gens* gens, uint32_t flags,
                    const uint8_t* rnd, sbn_transcript* tr, uint8_t* out_proof) {
  if (!c || !k || !vars || (!input && num_inputs) || !gens || !rnd || !tr || !out_proof) return SBN_EINVAL;
  return snark_prove_entry(c, "snark prove", k, vars, input, num_inputs, gens, nullptr, nullptr, flags, rnd, tr, out_proof);
}

int sbn_snark_prove_kzg(sbn_ctx* c, const sbn_snark_key* k, const sbn_table* vars, const uint8_t* input, size_t num_inputs, const sbn_snark_gens* gens,
                        const sbn_bases* srs, const sbn_derefs_key* derefs_key, uint32_t flags, const uint8_t* rnd, sbn_transcript* tr, uint8_t* out_proof) {
  if (!c || !k || !vars || (!input && num_inputs) || !gens || !srs || !rnd || !tr || !out_proof) return SBN_EINVAL;
  return snark_prove_entry(c, "snark prove (KZG)", k, vars, input, num_inputs, gens, srs, derefs_key, flags, rnd, tr, out_proof);
}

int sbn_snark_verify(sbn_ctx* c, const sbn_snark_key* k, const uint8_t* input, size_t num_inputs, const sbn_snark_gens* gens, const uint8_t* proof, size_t proof_len,
                     sbn_transcript* tr, int* accepted) {
  if (!c || !k || (!input && num_inputs) || !gens || !proof || !tr || !accepted) return SBN_EINVAL;
  return snark_verify_entry(c, "snark verify", k, input, num_inputs, gens, nullptr, nullptr, proof, proof_len, tr, accepted);
}

int sbn_snark_verify_kzg(sbn_ctx* c, const sbn_snark_key* k, const uint8_t* input, size_t num_inputs, const sbn_snark_gens* gens, const sbn_g2_lines* g2, const sbn_g2_lines* tau_g2,
                         const uint8_t* proof, size_t proof_len, sbn_transcript* tr, int* accepted) {
  if (!c || !k || (!input && num_inputs) || !gens || !g2 || !tau_g2 || !proof || !tr || !accepted) return SBN_EINVAL;
  return snark_verify_entry(c, "snark verify (KZG)", k, input, num_inputs, gens, g2, tau_g2, proof, proof_len, tr, accepted);
}

const sbn_dense* sbn_snark_key_dense(const sbn_snark_key* k) { return k ? k->dense : nullptr; }

}  // extern "C"
