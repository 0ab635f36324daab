// abi_r1cs_proof.inc — C ABI: R1CSProof::prove (r1csproof.rs:241-459) in ONE call.  sbn_r1cs_proof_prove composes, on one working copy of the
// caller's Merlin transcript, the bodies of the calls that already hold its heavy parts:
//   the witness commitment      commit_rows_launch over the first R generators of gens_pc (commit_poly, r1csproof.rs:210-237): ONE L x R launch
//   eq(tau), z, Az / Bz / Cz    eq_evals_locked, k_r1cs_build_z (r1csproof.rs:268-277), r1cs_multiply_locked
//   phase 1 and phase 2         zk_prove_locked<KIND_R1CS> / <KIND_QUAD>   (r1csproof.rs:295, :394)
//   evals_ABC                   r1cs_eval_table_locked                      (r1csproof.rs:376-387)
//   vars(ry[1..]), the opening  eq_evals_locked + table_dot_locked, polyeval_prove_locked   (r1csproof.rs:409-420)
// and adds what had no device form: KnowledgeProof::prove, ProductProof::prove and EqualityProof::prove (nizk/mod.rs:34-59, :167-227, :96-124).
// Their 14 group elements are all v * G + b * h over gens_1, i.e. rows [0 ... 0 ‖ v ‖ b] over the (gens_1, gens_4) set of zk_ext, whose last
// two columns are gens_1's points.  EqualityProof's alpha = r * h is the row [0, r]; ProductProof's delta = b3 * X + b5 * h with
// X = x * G + rX * h (nizk/mod.rs:202-205) is the row [b3 x, b3 rX + b5] — the same group element, the same bytes.  The 11 elements behind
// phase 1 depend on no challenge of that step: ONE 11-row commit and ONE host wait; the 3 of the last equality proof are one more.  No scalar
// multiplication runs on the CPU; the host does the Fr arithmetic of the responses (host_field.hpp) and the transcript.
// Included by sbn254.hip.

struct R1csProofShape { size_t nx, ell, ny, ml, lg, L, R, rnd_scalars, proof_bytes; };
static bool r1cs_proof_shape(size_t num_cons, size_t num_vars, R1csProofShape* s) {
  if (num_cons < 2 || (num_cons & (num_cons - 1)) || num_vars < 2 || (num_vars & (num_vars - 1))) return false;
  s->nx = r1cs_log2(num_cons); s->ell = r1cs_log2(num_vars); s->ny = s->ell + 1;
  if (s->ell > 2 * (size_t)PE_SIDE_MAX || s->nx > 40) return false;
  s->ml = s->ell / 2; s->lg = s->ell - s->ml; s->L = (size_t)1 << s->ml; s->R = (size_t)1 << s->lg;
  s->rnd_scalars = s->L + 8 * s->nx + 7 * s->ny + 2 * s->lg + 17;
  s->proof_bytes = 32 * (s->L + 10 * s->nx + 9 * s->ny + 20) + 64 * s->lg + 128;
  return true;
}

// gens_n (the first R generators of gens_pc, with h) and gens_1 = (G[R], h) (DotProductProofGens::new, nizk/mod.rs:412-415) as handles of their
// own: sbn_bases_split_at's copies, made on the first call and owned by gens_pc
static int r1cs_proof_gens(sbn_ctx* c, const sbn_bases* pc, size_t R, const sbn_bases** gn, const sbn_bases** g1) {
  const uint8_t* p = (const uint8_t*)pc->d_pts; const void* h = p + 64 * pc->n;
  int rc;
  if ((rc = derived_set(pc, DERIVED_R1CS_GENS_N, std::string(), [&](sbn_bases** b) { return bases_from_device(c, p, R, h, b); }, gn))) return rc;
  return derived_set(pc, DERIVED_R1CS_GENS_1, std::string(), [&](sbn_bases** b) { return bases_from_device(c, p + 64 * R, 1, h, b); }, g1);
}

// nrows <= 11 elements v * G + b * h over gens_1 as ONE commit over the (gens_1, gens_4) set and ONE host wait; vb: v, b per row, canonical.
// out: nrows compressed points
static int r1cs_proof_sigma_rows(sbn_ctx* c, const sbn_bases* ext, const sbn_host::fr::El (*vb)[2], uint32_t nrows, uint8_t* out) {
  int rc;
  const size_t R = ext->n;                                          // gens_4's 4 + its h + gens_1's two points, no blind column
  if ((rc = ensure(c, c->sc_prove, (size_t)R1CS_SIGMA_ROWS_MAX * R * 32))) return rc;
  R1csSigmaRows A; memset(&A, 0, sizeof A);
  for (uint32_t i = 0; i < nrows; i++) { memcpy(A.vb[i], vb[i][0].v, 32); memcpy(A.vb[i] + 8, vb[i][1].v, 32); }
  uint32_t* rows = (uint32_t*)c->sc_prove.p;
  LAUNCH(c, "k_r1cs_sigma_rows", k_r1cs_sigma_rows, 1, 256, rows, (uint32_t)R, nrows, A);
  uint32_t seq = 0;
  uint8_t xy[R1CS_SIGMA_ROWS_MAX * 64];
  if ((rc = rows_to_host_launch(c, ext, rows, nullptr, nrows, R, nullptr, 0u, zk_slot_word(0), zk_flag_word(0), &seq))) return rc;
  if ((rc = rows_to_host_collect(c, zk_slot_word(0), zk_flag_word(0), seq, nrows, xy, nullptr, nullptr, 0))) return rc;
  sbn_g1_compress(xy, nrows, out);
  return SBN_OK;
}

// the proof on the transcript `t` (a copy of the caller's); arguments already checked
static int r1cs_proof_locked(sbn_ctx* c, const sbn_r1cs* m, const sbn_table* vars, const uint8_t* input, size_t num_inputs, const sbn_bases* gens_pc,
                             const sbn_bases* gens_3, const sbn_bases* gens_4, const R1csProofShape& s, const uint8_t* rnd, sbn_host::MerlinTranscript& t,
                             uint8_t* out_proof, uint8_t* out_rx, uint8_t* out_ry) {
  using namespace sbn_host::fr;
  TableScope T(c);                                                 // every intermediate table of the call
  sbn_table *eq = nullptr, *z = nullptr, *in = nullptr, *Az = nullptr, *Bz = nullptr, *Cz = nullptr, *abc = nullptr, *chi = nullptr;
  sbn_host::Script ts{t};
  auto put = [](uint8_t* o, const El& e) { memcpy(o, e.v, 32); };
  int rc;
  // rnd: the RandomTape draws in the reference's order
  const uint8_t* poly_blinds = rnd;
  const uint8_t* rnd_sc1 = poly_blinds + 32 * s.L;
  const uint8_t* claim_blinds = rnd_sc1 + 32 * 8 * s.nx;          // Az_blind, Bz_blind, Cz_blind, prod_Az_Bz_blind
  const uint8_t* kn_t = claim_blinds + 128;                        // t1, t2
  const uint8_t* pr_b = kn_t + 64;                                 // b1 .. b5
  const uint8_t* eq1_r = pr_b + 160;
  const uint8_t* rnd_sc2 = eq1_r + 32;
  const uint8_t* blind_eval = rnd_sc2 + 32 * 7 * s.ny;
  const uint8_t* rnd_open = blind_eval + 32;
  const uint8_t* eq2_r = rnd_open + 32 * (3 + 2 * s.lg);
  // out_proof: the fields of R1CSProof in declaration order (r1csproof.rs:187-202)
  uint8_t* o_comm = out_proof;
  uint8_t* o_sc1 = o_comm + 32 * s.L;
  uint8_t* o_claims = o_sc1 + 320 * s.nx;
  uint8_t* o_pok = o_claims + 128;
  uint8_t* o_eq1 = o_pok + 352;
  uint8_t* o_sc2 = o_eq1 + 64;
  uint8_t* o_cy = o_sc2 + 288 * s.ny;
  uint8_t* o_open = o_cy + 32;
  uint8_t* o_eq2 = o_open + 64 * s.lg + 128;

  const sbn_bases *gens_n = nullptr, *gens_1 = nullptr, *ext = nullptr;
  if ((rc = r1cs_proof_gens(c, gens_pc, s.R, &gens_n, &gens_1))) return rc;
  if ((rc = ensure_pin(c, 8192 + 32 * s.rnd_scalars + 65 * s.L))) return rc;      // (sized once: no call below grows it mid-flight)

  // ---- 1. the statement (r1csproof.rs:250-255; a slice of scalars is one message per scalar, transcript.rs:46-50) ----
  ts.protocol("R1CS proof");
  ts.scalars("input", input, num_inputs);

  // ---- 2. the witness commitment (commit_poly, r1csproof.rs:210-237): one L x R commit, absorbed as PolyCommitment (:28-36) ----
  {
    const size_t nv = vars->len;
    if ((rc = ensure(c, c->scal_canon, (nv + s.L) * 32))) return rc;
    uint32_t* o = (uint32_t*)c->scal_canon.p; uint32_t* dB = o + 8 * nv;
    memcpy((uint8_t*)c->pin + 4096, poly_blinds, s.L * 32);
    HIPCHK(c, hipMemcpyAsync(dB, (uint8_t*)c->pin + 4096, s.L * 32, hipMemcpyHostToDevice, c->stream));
    const uint32_t* dZ = (const uint32_t*)vars->d;
    RowInfo ri;
    if (gens_n->uniq) {                                             // merged duplicates: the merge pass converts table values on the way out (sbn_commit_rows_dev)
      LAUNCH(c, "k_fr_to_mont", k_fr_to_mont, stream_grid(s.L), 256, (const uint32_t*)dB, dB, s.L);
      ri.mont_scalars = true;
    } else {
      LAUNCH(c, "k_scalars_from_mont", k_scalars_from_internal, (unsigned)((nv + 255) / 256), 256, dZ, o, nv);
      dZ = o;
    }
    std::vector<uint8_t> xy(64 * s.L);
    if ((rc = commit_rows_device(c, gens_n, dZ, dB, s.L, s.R, xy.data(), nullptr, ri))) return rc;
    sbn_g1_compress(xy.data(), s.L, o_comm);
    ts.message("poly_commitment", "poly_commitment_begin", 21);
    for (size_t i = 0; i < s.L; i++) ts.point("poly_commitment_share", o_comm + 32 * i);
    ts.message("poly_commitment", "poly_commitment_end", 19);
  }

  // ---- 3. phase 1 (r1csproof.rs:268-313) ----
  std::vector<uint8_t> tau(32 * s.nx);
  ts.challenges("challenge_tau", tau.data(), s.nx);               // challenge_vector
  if ((rc = eq_evals_locked(c, tau.data(), s.nx, &eq))) return rc;
  T.keep(eq);
  if ((rc = T.alloc(2 * m->nv, "r1cs table", &z))) return rc;
  if (num_inputs) {                                                 // (canonical bytes, not table entries: k_r1cs_build_z converts them)
    if ((rc = T.alloc(num_inputs, "r1cs proof inputs", &in))) return rc;
    HIPCHK(c, hipMemcpyAsync(in->d, input, num_inputs * 32, hipMemcpyHostToDevice, c->stream));
  }
  LAUNCH(c, "k_r1cs_build_z", k_r1cs_build_z, stream_grid(2 * m->nv), 256, (const uint32_t*)vars->d, (const uint32_t*)(in ? in->d : nullptr), m->nv, num_inputs, (uint32_t*)z->d);
  LAUNCHCHK(c);
  if ((rc = r1cs_multiply_locked(c, m, z, &Az, &Bz, &Cz))) return rc;
  T.keep(Az); T.keep(Bz); T.keep(Cz);
  uint8_t fin1[128], blind_post1[32], zero32[32] = {0};
  {
    sbn_table* tabs[4] = {eq, Az, Bz, Cz};
    if ((rc = zk_prove_locked<KIND_R1CS>(c, tabs, gens_1, gens_4, s.nx, zero32, zero32, rnd_sc1, t, o_sc1, out_rx, fin1, blind_post1))) return rc;
  }
  if ((rc = zk_ext(c, gens_1, gens_4, &ext))) return rc;           // phase 1 built it

  // ---- 4. the Σ step behind phase 1 (r1csproof.rs:315-366) ----
  const El tau_c = el_from(fin1), Az_c = el_from(fin1 + 32), Bz_c = el_from(fin1 + 64), Cz_c = el_from(fin1 + 96);
  const El Az_b = el_from(claim_blinds), Bz_b = el_from(claim_blinds + 32), Cz_b = el_from(claim_blinds + 64), prod_b = el_from(claim_blinds + 96);
  {
    const El t1 = el_from(kn_t), t2 = el_from(kn_t + 32);
    const El b1 = el_from(pr_b), b2 = el_from(pr_b + 32), b3 = el_from(pr_b + 64), b4 = el_from(pr_b + 96), b5 = el_from(pr_b + 128);
    const El r1 = el_from(eq1_r);
    const El prod = fmul(Az_c, Bz_c);
    const El blind_expected = fmul(tau_c, sub(prod_b, Cz_b));       // :356
    const El claim_post = fmul(sub(prod, Cz_c), tau_c);             // :357
    const El vb[11][2] = {
      {Cz_c, Cz_b}, {t1, t2},                                       // KnowledgeProof: C, alpha               (nizk/mod.rs:47-51)
      {Az_c, Az_b}, {Bz_c, Bz_b}, {prod, prod_b},                   // ProductProof: X, Y, Z                  (:187-194)
      {b1, b2}, {b3, b4},                                           //   alpha, beta                           (:196-200)
      {fmul(b3, Az_c), add(fmul(b3, Az_b), b5)},                    //   delta = b3 * X + b5 * h               (:202-205)
      {claim_post, blind_expected}, {claim_post, el_from(blind_post1)}, {from_u64(0), r1},     // EqualityProof: C1, C2, alpha = r * h   (:110-117)
    };
    uint8_t P[11 * 32];
    if ((rc = r1cs_proof_sigma_rows(c, ext, vb, 11, P))) return rc;
    const uint8_t *pC = P, *pKa = P + 32, *pX = P + 64, *pY = P + 96, *pZ = P + 128, *pPa = P + 160, *pPb = P + 192, *pPd = P + 224, *pC1 = P + 256, *pC2 = P + 288, *pEa = P + 320;
    uint8_t cb[32];
    ts.protocol("knowledge proof");                                 // nizk/mod.rs:41
    ts.point("C", pC); ts.point("alpha", pKa);
    ts.challenge("c", cb);
    El cc = el_from(cb);
    memcpy(o_pok, pKa, 32); put(o_pok + 32, add(fmul(Cz_c, cc), t1)); put(o_pok + 64, add(fmul(Cz_b, cc), t2));      // :55-56
    ts.protocol("product proof");                                   // :178
    ts.point("X", pX); ts.point("Y", pY); ts.point("Z", pZ);
    ts.point("alpha", pPa); ts.point("beta", pPb); ts.point("delta", pPd);
    ts.challenge("c", cb);
    cc = el_from(cb);
    uint8_t* pp = o_pok + 96;
    memcpy(pp, pPa, 32); memcpy(pp + 32, pPb, 32); memcpy(pp + 64, pPd, 32);
    put(pp + 96, add(b1, fmul(cc, Az_c))); put(pp + 128, add(b2, fmul(cc, Az_b))); put(pp + 160, add(b3, fmul(cc, Bz_c))); put(pp + 192, add(b4, fmul(cc, Bz_b)));
    put(pp + 224, add(b5, fmul(cc, sub(prod_b, fmul(Az_b, Bz_c)))));                                                  // :210-214
    memcpy(o_claims, pX, 32); memcpy(o_claims + 32, pY, 32); memcpy(o_claims + 64, pC, 32); memcpy(o_claims + 96, pZ, 32);
    ts.point("comm_Az_claim", pX); ts.point("comm_Bz_claim", pY);                                                     // r1csproof.rs:349-352
    ts.point("comm_Cz_claim", pC); ts.point("comm_prod_Az_Bz_claims", pZ);
    ts.protocol("equality proof");                                  // nizk/mod.rs:105
    ts.point("C1", pC1); ts.point("C2", pC2); ts.point("alpha", pEa);
    ts.challenge("c", cb);
    cc = el_from(cb);
    memcpy(o_eq1, pEa, 32); put(o_eq1 + 32, add(fmul(cc, sub(blind_expected, el_from(blind_post1))), r1));            // :121
  }

  // ---- 5. phase 2 (r1csproof.rs:368-406) ----
  uint8_t rA[32], rB[32], rC[32];
  ts.challenge("challenge_Az", rA); ts.challenge("challenge_Bz", rB); ts.challenge("challenge_Cz", rC);
  const El claim2 = add(add(fmul(el_from(rA), Az_c), fmul(el_from(rB), Bz_c)), fmul(el_from(rC), Cz_c));              // :373
  const El blind2 = add(add(fmul(el_from(rA), Az_b), fmul(el_from(rB), Bz_b)), fmul(el_from(rC), Cz_b));              // :374
  if ((rc = r1cs_eval_table_locked(c, m, out_rx, s.nx, rA, rB, rC, &abc))) return rc;
  T.keep(abc);
  uint8_t fin2[64], blind_post2[32];
  {
    sbn_table* tabs[2] = {z, abc};
    uint8_t c2[32], b2[32]; put(c2, claim2); put(b2, blind2);
    if ((rc = zk_prove_locked<KIND_QUAD>(c, tabs, gens_1, gens_3, s.ny, c2, b2, rnd_sc2, t, o_sc2, out_ry, fin2, blind_post2))) return rc;
  }

  // ---- 6. vars(ry[1..]) and its opening (r1csproof.rs:409-420) ----
  uint8_t eval_vars[32];
  if ((rc = eq_evals_locked(c, out_ry + 32, s.ell, &chi))) return rc;
  T.keep(chi);
  if ((rc = table_dot_locked(c, (const uint32_t*)vars->d, (const uint32_t*)chi->d, vars->len, eval_vars))) return rc;
  {
    uint8_t cx[64], cy[64]; int xi = 0, yi = 0;
    if ((rc = polyeval_prove_locked(c, gens_pc, vars, poly_blinds, out_ry + 32, s.ell, eval_vars, blind_eval, rnd_open, t, o_open, cx, &xi, cy, &yi))) return rc;
    sbn_g1_compress(cy, 1, o_cy);                                   // comm_vars_at_ry = C_Zr_prime (hyrax.rs:116)
  }

  // ---- 7. the last equality proof (r1csproof.rs:423-435), over gens_pc.gens.gens_1 — the same two points ----
  {
    const El one_m_ry0 = sub(from_u64(1), el_from(out_ry));
    const El blind_expected = fmul(el_from(fin2 + 32), fmul(one_m_ry0, el_from(blind_eval)));                         // :424-425
    const El claim_post = fmul(el_from(fin2), el_from(fin2 + 32));                                                    // :426
    const El r2 = el_from(eq2_r);
    const El vb[3][2] = {{claim_post, blind_expected}, {claim_post, el_from(blind_post2)}, {from_u64(0), r2}};
    uint8_t P[3 * 32], cb[32];
    if ((rc = r1cs_proof_sigma_rows(c, ext, vb, 3, P))) return rc;
    ts.protocol("equality proof");
    ts.point("C1", P); ts.point("C2", P + 32); ts.point("alpha", P + 64);
    ts.challenge("c", cb);
    memcpy(o_eq2, P + 64, 32); put(o_eq2 + 32, add(fmul(el_from(cb), sub(blind_expected, el_from(blind_post2))), r2));
  }
  if (c->prof) { HIPCHK(c, hipStreamSynchronize(c->stream)); prof_drain(c); }
  return T.done();
}

extern "C" {

int sbn_r1cs_proof_sizes(size_t num_cons, size_t num_vars, size_t* rnd_scalars, size_t* proof_bytes) {
  R1csProofShape s;
  if (!r1cs_proof_shape(num_cons, num_vars, &s)) return SBN_EINVAL;
  if (rnd_scalars) *rnd_scalars = s.rnd_scalars;
  if (proof_bytes) *proof_bytes = s.proof_bytes;
  return SBN_OK;
}

int sbn_r1cs_proof_prove(sbn_ctx* c, const sbn_r1cs* inst, const sbn_table* vars, const uint8_t* input, size_t num_inputs,
                         const sbn_bases* gens_pc, const sbn_bases* gens_3, const sbn_bases* gens_4, const uint8_t* rnd, sbn_transcript* tr,
                         uint8_t* out_proof, uint8_t* out_rx, uint8_t* out_ry) {
  if (!c || !inst || !vars || (!input && num_inputs) || !gens_pc || !gens_3 || !gens_4 || !rnd || !tr || !out_proof || !out_rx || !out_ry) return SBN_EINVAL;
  std::lock_guard<std::mutex> g(c->mu); hipSetDevice(c->device);
  R1csProofShape s;
  if (inst->nv < 2) return fail(c, SBN_EINVAL, "r1cs proof: num_vars = %zu: the opening needs at least one variable  [hyrax.rs:77, as sbn_polyeval_prove]", inst->nv);
  if (inst->nc < 2) return fail(c, SBN_EINVAL, "r1cs proof: num_cons = %zu: phase 1 needs at least one round  [r1csproof.rs:280]", inst->nc);
  if (!r1cs_proof_shape(inst->nc, inst->nv, &s)) return fail(c, SBN_EINVAL, "r1cs proof: shape %zu x %zu is outside what the opening takes", inst->nc, inst->nv);
  if (vars->len != inst->nv) return fail(c, SBN_EINVAL, "r1cs proof: vars has %zu entries, the instance has num_vars = %zu  [r1cs.rs:139 assert_eq]", vars->len, inst->nv);
  if (num_inputs >= inst->nv) return fail(c, SBN_EINVAL, "r1cs proof: %zu inputs, num_vars = %zu  [r1csproof.rs:253 assert!(input.len() < vars.len())]", num_inputs, inst->nv);
  if (gens_pc->n != s.R + 1 || !gens_pc->has_h)
    return fail(c, SBN_EINVAL, "r1cs proof: gens_pc has %zu points%s, the opening needs %zu + 1 with h  [nizk/mod.rs:412-415, :455]", gens_pc->n, gens_pc->has_h ? "" : " and no h", s.R);
  if (gens_3->n != 3 || !gens_3->has_h) return fail(c, SBN_EINVAL, "r1cs proof: gens_3 has %zu points%s, 3 generators with h are needed  [nizk/mod.rs:322 assert_eq]", gens_3->n, gens_3->has_h ? "" : " and no h");
  if (gens_4->n != 4 || !gens_4->has_h) return fail(c, SBN_EINVAL, "r1cs proof: gens_4 has %zu points%s, 4 generators with h are needed  [nizk/mod.rs:322 assert_eq]", gens_4->n, gens_4->has_h ? "" : " and no h");
  for (size_t i = 0; i < num_inputs; i++) if (!fr_canonical(input + 32 * i)) return fail(c, SBN_EINVAL, "r1cs proof: input[%zu] is not canonical  [scalar.rs:87-95]", i);
  for (size_t i = 0; i < s.rnd_scalars; i++) if (!fr_canonical(rnd + 32 * i)) return fail(c, SBN_EINVAL, "r1cs proof: rnd[%zu] is not canonical  [scalar.rs:87-95]", i);
  return prove_on_copy(c, tr, [&](sbn_host::MerlinTranscript& t) { return r1cs_proof_locked(c, inst, vars, input, num_inputs, gens_pc, gens_3, gens_4, s, rnd, t, out_proof, out_rx, out_ry); });
}

}  // extern "C"
