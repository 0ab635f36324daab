// abi_r1cs_verify.inc — C ABI: R1CSProof::verify (r1csproof.rs:463-619) and ZKSumcheckInstanceProof::verify (sumcheck.rs:366-457) in ONE call each,
// with DotProductProof::verify (nizk/mod.rs:368-400), KnowledgeProof / ProductProof / EqualityProof::verify (nizk/mod.rs:61-81, :243-283, :126-149)
// and the Merlin transcript inside.  The opening of comm_vars is polyeval_verify_locked (abi_polyeval_verify.inc) on a handle made of the proof's bytes
// (bases_from_compressed_locked, abi_verify_common.inc).
//
// No fresh point is ever multiplied.  Every point of a check is a point of the proof or a generator, every coefficient a scalar the host derives
// from the transcript — c * Cy_i = (c w0) P_{i-1} + (c w1) comm_eval_i, and so on down to the proof's own points — so every check is a sum of
// entries of ONE table T[p][k] = 2^k P_p (k_pow2_table, once per call, behind ONE k_g1_decompress over all the proof's points) selected by
// scalar bits (k_select_sum).  A point whose BYTES the transcript needs (Cy of every round, phase 2's comm_claim, the `expected` points of the
// two equality proofs) is one such sum and one host wait: the kernel writes it to the hand-over area itself, the host brings it to affine form.
// Every equation, moved to one side, waits for the call's last launch, which answers "the sum is the identity" for all of them as packed
// bits.  Negated coefficients are r - x on the host; no scalar multiplication and no point addition runs on the CPU.
// The envelope (verify_on_copy), the hand-over area (vbox_ensure) and the device state's lease (SlabLease) are abi_verify_common.inc and ctx.hpp,
// g1_compressed_normalise and g1_xy_valid verify_host.hpp.
// Included by sbn254.hip; needs abi_verify_common.inc and abi_polyeval_verify.inc.

struct VSum {
  uint32_t n = 0; uint32_t idx[SEL_TERMS_MAX]; sbn_host::fr::El s[SEL_TERMS_MAX];
  bool over = false;
  void add(uint32_t i, const sbn_host::fr::El& x) { if (n == (uint32_t)SEL_TERMS_MAX) { over = true; return; } idx[n] = i; s[n] = x; n++; }
};

static const size_t RV_PIN_DESC = 8192;            // the descriptors' staging behind what the opening check stages in the pinned buffer
static inline size_t rv_desc_bytes(size_t max_eq) { return (4 * (size_t)SEL_DESC_WORDS * max_eq + 255) / 256 * 256; }
static inline size_t rv_pin_bytes(size_t np, size_t max_eq) { return RV_PIN_DESC + rv_desc_bytes(max_eq) + 32 * np + 64; }

// the device state of one call: the proof's points (compressed, canonical, flags, table layout), descriptors, sums, verdict bits, the table
struct VerifyRun {
  sbn_ctx* c; SlabLease slab;
  size_t np = 0, ntab = 0, max_eq = 0;
  uint32_t *d_comp = nullptr, *d_canon = nullptr, *d_mont = nullptr, *d_claim = nullptr, *d_desc = nullptr, *d_out = nullptr, *d_bits = nullptr, *d_table = nullptr;
  uint8_t* d_ok = nullptr;
  uint32_t xy_idx = 0; uint8_t xy[64];               // the one proof point the host needs in affine form, and its bytes once the first sum is back
  bool first = true, reject = false;                 // reject: a point of the proof does not decompress
  std::vector<VSum> eqs;
  explicit VerifyRun(sbn_ctx* c_) : c(c_), slab(c_) {}
};

// the proof's np compressed points (identity normalised) to the device, ONE decompress launch, ONE table launch over them and the generators in
// src.p[1 ..] (src.p[0] / n[0] are filled here).  claim_xy, or null: a canonical affine point that becomes source 1 (src.p[1] is filled here)
static int rv_begin(VerifyRun& V, const uint8_t* comp, size_t np, Pow2Src src, const uint8_t* claim_xy, size_t max_eq, uint32_t xy_idx) {
  sbn_ctx* c = V.c;
  int rc;
  if ((rc = vbox_ensure(c))) return rc;
  const size_t ok_words = (np + 3) / 4;
  if (32 + ok_words + 16 > (size_t)VBOX_FLAG_WORD) return fail(c, SBN_EINVAL, "r1cs verify: %zu points do not fit the hand-over area", np);
  V.np = np; V.max_eq = max_eq; V.xy_idx = xy_idx;
  size_t ntab = np;
  for (int s = 1; s < POW2_SRC_MAX; s++) ntab += src.n[s];
  V.ntab = ntab;
  auto up = [](size_t x) { return (x + 255) / 256 * 256; };
  const size_t o_comp = 0, o_canon = up(32 * np), o_ok = o_canon + 64 * np, o_mont = up(o_ok + 4 * ok_words), o_claim = up(o_mont + 64 * np), o_desc = o_claim + 256,
               o_out = up(o_desc + 4 * (size_t)SEL_DESC_WORDS * max_eq), o_bits = up(o_out + 128 * max_eq), o_table = up(o_bits + 4 * ((max_eq + 31) / 32)),
               total = o_table + 128 * (size_t)POW2_BITS * ntab;
  if ((rc = V.slab.get(total, "r1cs verify state"))) return rc;
  uint8_t* p0 = (uint8_t*)V.slab.p;
  V.d_comp = (uint32_t*)(p0 + o_comp); V.d_canon = (uint32_t*)(p0 + o_canon); V.d_ok = p0 + o_ok; V.d_mont = (uint32_t*)(p0 + o_mont); V.d_claim = (uint32_t*)(p0 + o_claim);
  V.d_desc = (uint32_t*)(p0 + o_desc); V.d_out = (uint32_t*)(p0 + o_out); V.d_bits = (uint32_t*)(p0 + o_bits); V.d_table = (uint32_t*)(p0 + o_table);
  uint8_t* pin = (uint8_t*)c->pin + RV_PIN_DESC + rv_desc_bytes(max_eq);      // (behind the descriptors, which the first sum stages while these copies may be in flight)
  memcpy(pin, comp, 32 * np);
  if (claim_xy) memcpy(pin + 32 * np, claim_xy, 64);
  HIPCHK(c, hipMemsetAsync(V.d_ok, 0, 4 * ok_words, c->stream));
  HIPCHK(c, hipMemcpyAsync(V.d_comp, pin, 32 * np, hipMemcpyHostToDevice, c->stream));
  LAUNCH(c, "k_g1_decompress", k_g1_decompress, (unsigned)((np + 63) / 64), 64, (const uint32_t*)V.d_comp, np, V.d_canon, V.d_mont, V.d_ok);
  if (claim_xy) {
    HIPCHK(c, hipMemcpyAsync(V.d_claim, pin + 32 * np, 64, hipMemcpyHostToDevice, c->stream));
    LAUNCH(c, "k_points_to_mont", k_points_to_mont, 1, 256, (const uint32_t*)V.d_claim, V.d_claim, (size_t)1);
    src.p[1] = V.d_claim;
  }
  src.p[0] = V.d_mont; src.n[0] = (uint32_t)np;
  LAUNCH(c, "k_pow2_table", k_pow2_table, (unsigned)((ntab + 63) / 64), 64, src, (uint32_t)ntab, V.d_table);
  LAUNCHCHK(c);
  return SBN_OK;
}

// descriptors of `n` sums into the pinned staging area; indices and sizes are checked here, before any launch reads them
static int rv_stage(VerifyRun& V, const VSum* sums, size_t n) {
  sbn_ctx* c = V.c;
  if (n == 0 || n > V.max_eq) return fail(c, SBN_EINVAL, "r1cs verify: %zu sums, room for %zu", n, V.max_eq);
  uint32_t* h = (uint32_t*)((uint8_t*)c->pin + RV_PIN_DESC);
  memset(h, 0, 4 * (size_t)SEL_DESC_WORDS * n);
  for (size_t i = 0; i < n; i++) {
    const VSum& s = sums[i];
    if (s.over || s.n > (uint32_t)SEL_TERMS_MAX) return fail(c, SBN_EINVAL, "r1cs verify: a sum of more than %d terms", SEL_TERMS_MAX);
    uint32_t* d = h + (size_t)SEL_DESC_WORDS * i;
    d[0] = s.n;
    for (uint32_t t = 0; t < s.n; t++) {
      if (s.idx[t] >= V.ntab) return fail(c, SBN_EINVAL, "r1cs verify: point index %u, the table has %zu", s.idx[t], V.ntab);
      d[1 + t] = s.idx[t];
      memcpy(d + 16 + 8 * t, s.s[t].v, 32);
    }
  }
  HIPCHK(c, hipMemcpyAsync(V.d_desc, h, 4 * (size_t)SEL_DESC_WORDS * n, hipMemcpyHostToDevice, c->stream));
  return SBN_OK;
}

// ONE sum and ONE wait: the point as canonical affine bytes.  The first of a call brings the decompression flags and V.xy with it
static int rv_sum(VerifyRun& V, const VSum& s, uint8_t xy[64]) {
  sbn_ctx* c = V.c;
  int rc;
  if ((rc = rv_stage(V, &s, 1))) return rc;
  const uint32_t seq = ++c->mbox_seq;
  const uint32_t na = V.first ? (uint32_t)((V.np + 3) / 4) : 0u, nb = V.first ? 16u : 0u;
  LAUNCH(c, "k_select_sum", k_select_sum, 1, 256, (const uint32_t*)V.d_desc, (const uint32_t*)V.d_table, (uint32_t*)nullptr, (uint32_t*)nullptr,
         (const uint32_t*)V.d_ok, na, (const uint32_t*)(V.d_canon + 16 * (size_t)V.xy_idx), nb, c->vbox, c->vbox + VBOX_FLAG_WORD, seq);
  LAUNCHCHK(c);
  if ((rc = sc_flag_wait(c, c->vbox + VBOX_FLAG_WORD, seq))) return rc;
  sbn_host::Pt S; memcpy(&S, c->vbox, 128);
  if (V.first) {
    const uint8_t* ok = (const uint8_t*)(c->vbox + 32);
    for (size_t i = 0; i < V.np; i++) if (!ok[i]) V.reject = true;
    memcpy(V.xy, c->vbox + 32 + na, 64);
    V.first = false;
  }
  sbn_host::to_affine_bytes(sbn_host::pt_from_device(S), xy, nullptr);
  return SBN_OK;
}

// every equation of the call in ONE launch; accepted: each sum is the identity
static int rv_finish(VerifyRun& V, int* accepted) {
  sbn_ctx* c = V.c;
  int rc;
  const size_t n = V.eqs.size(), words = (n + 31) / 32;
  if ((rc = rv_stage(V, V.eqs.data(), n))) return rc;
  HIPCHK(c, hipMemsetAsync(V.d_bits, 0, 4 * words, c->stream));
  LAUNCH(c, "k_select_sum", k_select_sum, (unsigned)n, 256, (const uint32_t*)V.d_desc, (const uint32_t*)V.d_table, V.d_out, V.d_bits,
         (const uint32_t*)nullptr, 0u, (const uint32_t*)nullptr, 0u, (uint32_t*)nullptr, (uint32_t*)nullptr, 0u);
  LAUNCHCHK(c);
  uint32_t* hb = (uint32_t*)c->pin;
  HIPCHK(c, hipMemcpyAsync(hb, V.d_bits, 4 * words, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  if (c->prof) prof_drain(c);
  bool all = true;
  for (size_t i = 0; i < n; i++) if (!((hb[i >> 5] >> (i & 31)) & 1u)) all = false;
  *accepted = all ? 1 : 0;
  return SBN_OK;
}

// where the generators of one sumcheck sit in the table
struct ZkVerifyGens { uint32_t G1, H1, Gn, Hn; };

// ZKSumcheckInstanceProof::verify (sumcheck.rs:366-457) on the transcript: `rounds` x (comm_poly, comm_eval, delta, beta | z[N], z_delta, z_beta) at
// `proof`, whose points are table entries base + 4 i + 0 .. 3 with the normalised bytes `comp`.  prev / prev_comp: comm_claim as a sum of table
// points and as bytes; on return the last comm_eval.  The round's two equations join V.eqs; the proof's scalars are canonical (checked by the caller)
static int zk_verify_rounds(VerifyRun& V, sbn_host::Script& ts, const uint8_t* comp, const uint8_t* proof, size_t rounds, int N, uint32_t base, const ZkVerifyGens& g,
                            VSum& prev, uint8_t prev_comp[32], uint8_t* out_r) {
  using namespace sbn_host::fr;
  const size_t stride = (size_t)(6 + N) * 32;
  const El zero = from_u64(0), one = from_u64(1);
  int rc;
  for (size_t i = 0; i < rounds; i++) {
    const uint32_t iP = base + 4 * (uint32_t)i, iE = iP + 1, iD = iP + 2, iB = iP + 3;
    const uint8_t* cp = comp + 32 * (size_t)iP; const uint8_t* ce = cp + 32; const uint8_t* delta = cp + 64; const uint8_t* beta = cp + 96;
    const uint8_t* zb = proof + stride * i + 128;
    ts.point("comm_poly", cp);                                      // sumcheck.rs:384
    uint8_t rj[32], wb[64], cb[32], cy[32], xy[64];
    ts.challenge("challenge_nextround", rj);                        // :387
    memcpy(out_r + 32 * i, rj, 32);
    ts.point("comm_claim_per_round", prev_comp);                    // :399-400
    ts.point("comm_eval", ce);
    ts.challenges("combine_two_claims_to_one", wb, 2);              // :403
    const El r = el_from(rj), w0 = el_from(wb), w1 = el_from(wb + 32);
    El a[4], pw = one, za = zero;
    for (int k = 0; k < N; k++) {                                   // a = w0 * [2, 1, 1 ..] + w1 * [1, r, r^2 ..]   (:416-438)
      a[k] = add(k == 0 ? add(w0, w0) : w0, fmul(w1, pw));
      za = add(za, fmul(a[k], el_from(zb + 32 * k)));               // <z, a>, nizk/mod.rs:393
      pw = fmul(pw, r);
    }
    VSum target;                                                    // comm_target = w0 * comm_claim_per_round + w1 * comm_eval   (:406-413)
    for (uint32_t t = 0; t < prev.n; t++) target.add(prev.idx[t], fmul(w0, prev.s[t]));
    target.add(iE, w1);
    if ((rc = rv_sum(V, target, xy))) return rc;
    if (V.reject) return SBN_OK;
    ts.protocol("dot product proof");                               // nizk/mod.rs:380
    ts.point("Cx", cp);
    ts.point_xy("Cy", xy, cy);
    ts.scalars("a", a, (size_t)N);
    ts.point("delta", delta);
    ts.point("beta", beta);
    ts.challenge("c", cb);
    const El cc = el_from(cb);
    VSum e1, e2;
    e1.add(iP, cc); e1.add(iD, one);                                // c Cx + delta - sum z_k G_k - z_delta h_n = 0   (:389-390)
    for (int k = 0; k < N; k++) e1.add(g.Gn + (uint32_t)k, sub(zero, el_from(zb + 32 * k)));
    e1.add(g.Hn, sub(zero, el_from(zb + 32 * N)));
    for (uint32_t t = 0; t < target.n; t++) e2.add(target.idx[t], fmul(cc, target.s[t]));      // c Cy + beta - <z, a> G - z_beta h = 0   (:392-394)
    e2.add(iB, one); e2.add(g.G1, sub(zero, za)); e2.add(g.H1, sub(zero, el_from(zb + 32 * N + 32)));
    V.eqs.push_back(e1); V.eqs.push_back(e2);
    prev = VSum(); prev.add(iE, one);
    memcpy(prev_comp, ce, 32);
  }
  return SBN_OK;
}

// EqualityProof::verify (nizk/mod.rs:126-149): C1 is a sum of table points, C2 and alpha are points of the proof
static int rv_equality(VerifyRun& V, sbn_host::Script& ts, const VSum& C1, uint32_t iC2, const uint8_t* c2_comp, uint32_t iAlpha, const uint8_t* alpha_comp, const uint8_t* z, uint32_t iH1) {
  using namespace sbn_host::fr;
  int rc;
  uint8_t xy[64], c1[32], cb[32];
  if ((rc = rv_sum(V, C1, xy))) return rc;
  if (V.reject) return SBN_OK;
  ts.protocol("equality proof");
  ts.point_xy("C1", xy, c1);
  ts.point("C2", c2_comp);
  ts.point("alpha", alpha_comp);
  ts.challenge("c", cb);
  const El cc = el_from(cb), zero = from_u64(0);
  VSum e;                                                           // c (C1 - C2) + alpha - z h = 0   (:141-146)
  for (uint32_t t = 0; t < C1.n; t++) e.add(C1.idx[t], fmul(cc, C1.s[t]));
  e.add(iC2, sub(zero, cc)); e.add(iAlpha, from_u64(1)); e.add(iH1, sub(zero, el_from(z)));
  V.eqs.push_back(e);
  return SBN_OK;
}

static int zk_sumcheck_verify_locked(sbn_ctx* c, const sbn_bases* g1, const sbn_bases* gn, const uint8_t* claim_xy, size_t rounds, int N, const uint8_t* proof,
                                     sbn_host::MerlinTranscript& t, uint8_t* r_out, uint8_t* eval_xy, int* accepted) {
  using namespace sbn_host::fr;
  *accepted = 0;
  const size_t stride = (size_t)(6 + N) * 32, np = 4 * rounds, max_eq = 2 * rounds;
  for (size_t i = 0; i < rounds; i++)
    for (int k = 0; k < N + 2; k++) if (!fr_canonical(proof + stride * i + 128 + 32 * k)) return SBN_OK;      // Scalar::from_bytes fails (scalar.rs:87-95)
  int rc;
  if ((rc = ensure_pin(c, rv_pin_bytes(np, max_eq)))) return rc;
  std::vector<uint8_t> comp(32 * np);
  for (size_t i = 0; i < rounds; i++) for (int k = 0; k < 4; k++) g1_compressed_normalise(proof + stride * i + 32 * k, comp.data() + 32 * (4 * i + k));
  VerifyRun V(c);
  Pow2Src src; memset(&src, 0, sizeof src);
  src.n[1] = 1; src.p[2] = (const uint32_t*)g1->d_pts; src.n[2] = 2; src.p[3] = (const uint32_t*)gn->d_pts; src.n[3] = (uint32_t)N + 1;
  if ((rc = rv_begin(V, comp.data(), np, src, claim_xy, max_eq, (uint32_t)(4 * (rounds - 1) + 1)))) return rc;
  ZkVerifyGens g; g.G1 = (uint32_t)np + 1; g.H1 = g.G1 + 1; g.Gn = g.H1 + 1; g.Hn = g.Gn + (uint32_t)N;
  sbn_host::Script ts{t};
  VSum prev; prev.add((uint32_t)np, from_u64(1));
  uint8_t prev_comp[32];
  sbn_host::g1_compress(claim_xy, prev_comp);
  if ((rc = zk_verify_rounds(V, ts, comp.data(), proof, rounds, N, 0, g, prev, prev_comp, r_out))) return rc;
  if (V.reject) return SBN_OK;
  memcpy(eval_xy, V.xy, 64);
  return rv_finish(V, accepted);
}

static int r1cs_verify_locked(sbn_ctx* c, const R1csProofShape& s, const uint8_t* input, size_t num_inputs, const uint8_t* evals, const sbn_bases* gens_pc,
                              const sbn_bases* gens_3, const sbn_bases* gens_4, const uint8_t* proof, sbn_host::MerlinTranscript& t, uint8_t* rx, uint8_t* ry, int* accepted) {
  using namespace sbn_host::fr;
  *accepted = 0;
  // the fields of R1CSProof in declaration order (r1csproof.rs:187-202), as sbn_r1cs_proof_prove writes them
  const uint8_t* o_comm = proof;
  const uint8_t* o_sc1 = o_comm + 32 * s.L;
  const uint8_t* o_claims = o_sc1 + 320 * s.nx;
  const uint8_t* o_pok = o_claims + 128;
  const uint8_t* o_eq1 = o_pok + 352;
  const uint8_t* o_sc2 = o_eq1 + 64;
  const uint8_t* o_cy = o_sc2 + 288 * s.ny;
  const uint8_t* o_open = o_cy + 32;
  const uint8_t* o_eq2 = o_open + 64 * s.lg + 128;
  const uint8_t* kz = o_pok + 32; const uint8_t* pz = o_pok + 192;      // KnowledgeProof's z1, z2; ProductProof's z1 .. z5
  // a scalar of the proof >= r: Scalar::from_bytes fails (scalar.rs:87-95) — the opening's two are checked by the opening
  for (size_t i = 0; i < s.nx; i++) for (int k = 0; k < 6; k++) if (!fr_canonical(o_sc1 + 320 * i + 128 + 32 * k)) return SBN_OK;
  for (size_t i = 0; i < s.ny; i++) for (int k = 0; k < 5; k++) if (!fr_canonical(o_sc2 + 288 * i + 128 + 32 * k)) return SBN_OK;
  for (int k = 0; k < 2; k++) if (!fr_canonical(kz + 32 * k)) return SBN_OK;
  for (int k = 0; k < 5; k++) if (!fr_canonical(pz + 32 * k)) return SBN_OK;
  if (!fr_canonical(o_eq1 + 32) || !fr_canonical(o_eq2 + 32)) return SBN_OK;

  int rc;
  const size_t nr = s.nx + s.ny, np = 4 * nr + 11, max_eq = 2 * nr + 6;
  if ((rc = ensure_pin(c, rv_pin_bytes(np, max_eq)))) return rc;      // (sized once: the opening asks for less)

  // the commitment of the witness as a handle, as sbn_bases_from_compressed builds one
  sbn_bases* comm = nullptr;
  {
    size_t bad = SIZE_MAX;
    rc = bases_from_compressed_locked(c, o_comm, s.L, &comm, &bad);
    if (rc == SBN_EINVAL && bad != SIZE_MAX) return SBN_OK;        // a row commitment does not decompress
    if (rc) return rc;
  }
  struct FreeBases { sbn_ctx* c; sbn_bases* b; ~FreeBases() { sbn_bases_free(c, b); } } drop{c, comm};

  // the table's points: phase 1's rounds, phase 2's rounds, then the eleven others; the generators behind them
  const uint32_t b1 = 0, b2 = 4 * (uint32_t)s.nx, iAz = 4 * (uint32_t)nr, iBz = iAz + 1, iCz = iAz + 2, iPr = iAz + 3, iKa = iAz + 4, iPa = iAz + 5, iPb = iAz + 6, iPd = iAz + 7,
                 iE1 = iAz + 8, iE2 = iAz + 9, iCv = iAz + 10;
  std::vector<uint8_t> comp(32 * np);
  auto put = [&](uint32_t idx, const uint8_t* b) { g1_compressed_normalise(b, comp.data() + 32 * (size_t)idx); };
  for (size_t i = 0; i < s.nx; i++) for (uint32_t k = 0; k < 4; k++) put(b1 + 4 * (uint32_t)i + k, o_sc1 + 320 * i + 32 * k);
  for (size_t i = 0; i < s.ny; i++) for (uint32_t k = 0; k < 4; k++) put(b2 + 4 * (uint32_t)i + k, o_sc2 + 288 * i + 32 * k);
  for (uint32_t k = 0; k < 4; k++) put(iAz + k, o_claims + 32 * k);
  put(iKa, o_pok); put(iPa, o_pok + 96); put(iPb, o_pok + 128); put(iPd, o_pok + 160); put(iE1, o_eq1); put(iE2, o_eq2); put(iCv, o_cy);
  auto cb_of = [&](uint32_t idx) { return (const uint8_t*)comp.data() + 32 * (size_t)idx; };
  const uint32_t iG1 = (uint32_t)np, iH1 = iG1 + 1;
  ZkVerifyGens g4, g3;
  g4.G1 = g3.G1 = iG1; g4.H1 = g3.H1 = iH1; g4.Gn = iH1 + 1; g4.Hn = g4.Gn + 4; g3.Gn = g4.Hn + 1; g3.Hn = g3.Gn + 3;
  VerifyRun V(c);
  {
    Pow2Src src; memset(&src, 0, sizeof src);
    src.p[1] = (const uint32_t*)gens_pc->d_pts + 16 * s.R; src.n[1] = 2;      // gens_1 = (G[R], h) of gens_pc (nizk/mod.rs:412-415): its last two points
    src.p[2] = (const uint32_t*)gens_4->d_pts; src.n[2] = 5;
    src.p[3] = (const uint32_t*)gens_3->d_pts; src.n[3] = 4;
    if ((rc = rv_begin(V, comp.data(), np, src, nullptr, max_eq, iCv))) return rc;
  }

  sbn_host::Script ts{t};
  const El zero = from_u64(0), one = from_u64(1);
  auto neg = [&](const El& x) { return sub(zero, x); };
  ts.protocol("R1CS proof");                                        // r1csproof.rs:478
  ts.scalars("input", input, num_inputs);
  ts.message("poly_commitment", "poly_commitment_begin", 21);
  for (size_t i = 0; i < s.L; i++) { uint8_t b[32]; g1_compressed_normalise(o_comm + 32 * i, b); ts.point("poly_commitment_share", b); }
  ts.message("poly_commitment", "poly_commitment_end", 19);
  std::vector<uint8_t> tau(32 * s.nx);
  ts.challenges("challenge_tau", tau.data(), s.nx);

  // ---- phase 1 (r1csproof.rs:489-497): the claim is the commitment of zero with blind zero, the identity ----
  uint8_t post1[32], post2[32];
  {
    VSum prev; memset(post1, 0, 32); post1[31] = 0x40;
    if ((rc = zk_verify_rounds(V, ts, comp.data(), o_sc1, s.nx, 4, b1, g4, prev, post1, rx))) return rc;
    if (V.reject) return SBN_OK;
  }
  const uint32_t iPost1 = b1 + 4 * (uint32_t)(s.nx - 1) + 1, iPost2 = b2 + 4 * (uint32_t)(s.ny - 1) + 1;

  // ---- the Σ step (r1csproof.rs:499-541) ----
  uint8_t cb[32];
  {
    ts.protocol("knowledge proof");                                 // nizk/mod.rs:68
    ts.point("C", cb_of(iCz)); ts.point("alpha", cb_of(iKa));
    ts.challenge("c", cb);
    VSum e;                                                         // c C + alpha - z1 G - z2 h = 0   (:75-78)
    e.add(iCz, el_from(cb)); e.add(iKa, one); e.add(iG1, neg(el_from(kz))); e.add(iH1, neg(el_from(kz + 32)));
    V.eqs.push_back(e);
  }
  {
    ts.protocol("product proof");                                   // nizk/mod.rs:252
    ts.point("X", cb_of(iAz)); ts.point("Y", cb_of(iBz)); ts.point("Z", cb_of(iPr));
    ts.point("alpha", cb_of(iPa)); ts.point("beta", cb_of(iPb)); ts.point("delta", cb_of(iPd));
    ts.challenge("c", cb);
    const El cc = el_from(cb);
    // check_equality (:229-240): P + c X' - za G' - zb h = 0 for (alpha, X; z1, z2), (beta, Y; z3, z4) and, over the base X, (delta, Z; z3, z5)
    VSum ea, eb, ed;
    ea.add(iPa, one); ea.add(iAz, cc); ea.add(iG1, neg(el_from(pz))); ea.add(iH1, neg(el_from(pz + 32)));
    eb.add(iPb, one); eb.add(iBz, cc); eb.add(iG1, neg(el_from(pz + 64))); eb.add(iH1, neg(el_from(pz + 96)));
    ed.add(iPd, one); ed.add(iPr, cc); ed.add(iAz, neg(el_from(pz + 64))); ed.add(iH1, neg(el_from(pz + 128)));
    V.eqs.push_back(ea); V.eqs.push_back(eb); V.eqs.push_back(ed);
  }
  ts.point("comm_Az_claim", cb_of(iAz)); ts.point("comm_Bz_claim", cb_of(iBz));      // r1csproof.rs:519-522
  ts.point("comm_Cz_claim", cb_of(iCz)); ts.point("comm_prod_Az_Bz_claims", cb_of(iPr));
  {
    El tb = one;                                                    // taus_bound_rx (:524-527)
    for (size_t i = 0; i < s.nx; i++) {
      const El ri = el_from(rx + 32 * i), ti = el_from(tau.data() + 32 * i);
      tb = fmul(tb, add(fmul(ri, ti), fmul(sub(one, ri), sub(one, ti))));
    }
    VSum C1; C1.add(iPr, tb); C1.add(iCz, neg(tb));                 // expected = taus_bound_rx * (comm_prod - comm_Cz)   (:528)
    if ((rc = rv_equality(V, ts, C1, iPost1, post1, iE1, cb_of(iE1), o_eq1 + 32, iH1))) return rc;
    if (V.reject) return SBN_OK;
  }

  // ---- phase 2 (r1csproof.rs:543-566) ----
  uint8_t rA[32], rB[32], rC[32];
  ts.challenge("challenge_Az", rA); ts.challenge("challenge_Bz", rB); ts.challenge("challenge_Cz", rC);
  {
    VSum claim2; claim2.add(iAz, el_from(rA)); claim2.add(iBz, el_from(rB)); claim2.add(iCz, el_from(rC));      // :549-553
    uint8_t xy[64];
    if ((rc = rv_sum(V, claim2, xy))) return rc;
    if (V.reject) return SBN_OK;
    sbn_host::g1_compress(xy, post2);
    if ((rc = zk_verify_rounds(V, ts, comp.data(), o_sc2, s.ny, 3, b2, g3, claim2, post2, ry))) return rc;
    if (V.reject) return SBN_OK;
  }

  // ---- the opening of comm_vars at ry[1..] (r1csproof.rs:568-578) ----
  {
    int ok = 0;
    if ((rc = polyeval_verify_check(c, gens_pc, comm, ry + 32, s.ell, V.xy, nullptr))) return rc;
    if ((rc = polyeval_verify_locked(c, gens_pc, comm, ry + 32, s.ell, V.xy, nullptr, o_open, t, &ok))) return rc;
    if (!ok) return SBN_OK;
  }

  // ---- poly_input_eval (:580-594) and the last equality proof (:596-616) ----
  {
    auto chi = [&](size_t i) {                                      // EqPolynomial::evals of ry[1..] at index i: bit j of i, counted from the top, takes ry[1 + j]
      El e = one;
      for (size_t j = 0; j < s.ell; j++) { const El rj = el_from(ry + 32 * (1 + j)); e = fmul(e, ((i >> (s.ell - 1 - j)) & 1) ? rj : sub(one, rj)); }
      return e;
    };
    El pie = chi(0);
    for (size_t i = 0; i < num_inputs; i++) pie = add(pie, fmul(el_from(input + 32 * i), chi(i + 1)));
    const El ry0 = el_from(ry);
    const El sc = add(add(fmul(el_from(rA), el_from(evals)), fmul(el_from(rB), el_from(evals + 32))), fmul(el_from(rC), el_from(evals + 64)));
    VSum C1;                                                        // expected = (comm_vars_at_ry (1 - ry[0]) + poly_input_eval G ry[0]) * (rA A + rB B + rC C)
    C1.add(iCv, fmul(sc, sub(one, ry0))); C1.add(iG1, fmul(sc, fmul(ry0, pie)));
    if ((rc = rv_equality(V, ts, C1, iPost2, post2, iE2, cb_of(iE2), o_eq2 + 32, iH1))) return rc;
    if (V.reject) return SBN_OK;
  }
  return rv_finish(V, accepted);
}

static int zk_verify_gens_check(sbn_ctx* c, const char* who, const sbn_bases* b, size_t n) {
  if (b->n != n || !b->has_h) return fail(c, SBN_EINVAL, "%s: a generator set has %zu points%s, %zu with h are needed  [nizk/mod.rs:322-323 assert_eq]", who, b->n, b->has_h ? "" : " and no h", n);
  return SBN_OK;
}

extern "C" {

int sbn_zk_sumcheck_verify(sbn_ctx* c, const sbn_bases* gens_1, const sbn_bases* gens_n, const uint8_t comm_claim_xy[64], size_t num_rounds, size_t degree_bound,
                           const uint8_t* proof, sbn_transcript* tr, uint8_t* out_r, uint8_t out_comm_eval_xy[64], int* accepted) {
  if (!c || !gens_1 || !gens_n || !comm_claim_xy || !proof || !tr || !out_r || !out_comm_eval_xy || !accepted) return SBN_EINVAL;
  if (degree_bound != 2 && degree_bound != 3) return fail(c, SBN_EINVAL, "zk sumcheck verify: degree_bound = %zu (2 or 3)", degree_bound);
  if (num_rounds == 0 || num_rounds > 64) return fail(c, SBN_EINVAL, "zk sumcheck verify: %zu rounds (1 .. 64)", num_rounds);
  int rc;
  if ((rc = zk_verify_gens_check(c, "zk sumcheck verify", gens_1, 1))) return rc;
  if ((rc = zk_verify_gens_check(c, "zk sumcheck verify", gens_n, degree_bound + 1))) return rc;
  if (!g1_xy_valid(comm_claim_xy)) return fail(c, SBN_EINVAL, "zk sumcheck verify: comm_claim is not a canonical point of the curve");
  std::lock_guard<std::mutex> g(c->mu); hipSetDevice(c->device);
  std::vector<uint8_t> r(32 * num_rounds); uint8_t exy[64];
  rc = verify_on_copy(c, tr, accepted, [&](sbn_host::MerlinTranscript& t) {
    return zk_sumcheck_verify_locked(c, gens_1, gens_n, comm_claim_xy, num_rounds, (int)degree_bound + 1, proof, t, r.data(), exy, accepted);
  });
  if (rc == SBN_OK && *accepted) { memcpy(out_r, r.data(), r.size()); memcpy(out_comm_eval_xy, exy, 64); }
  return rc;
}

int sbn_r1cs_proof_verify(sbn_ctx* c, size_t num_cons, size_t num_vars, const uint8_t* input, size_t num_inputs, const uint8_t evals[96],
                          const sbn_bases* gens_pc, const sbn_bases* gens_3, const sbn_bases* gens_4, const uint8_t* proof,
                          sbn_transcript* tr, uint8_t* out_rx, uint8_t* out_ry, int* accepted) {
  if (!c || (!input && num_inputs) || !evals || !gens_pc || !gens_3 || !gens_4 || !proof || !tr || !out_rx || !out_ry || !accepted) return SBN_EINVAL;
  R1csProofShape s;
  if (!r1cs_proof_shape(num_cons, num_vars, &s)) return fail(c, SBN_EINVAL, "r1cs verify: shape %zu x %zu (powers of two from 2 on, within what the opening takes)", num_cons, num_vars);
  if (num_inputs >= num_vars) return fail(c, SBN_EINVAL, "r1cs verify: %zu inputs, num_vars = %zu  [r1csproof.rs:475 assert!(input.len() < num_vars)]", num_inputs, num_vars);
  int rc;
  if ((rc = zk_verify_gens_check(c, "r1cs verify: gens_pc", gens_pc, s.R + 1))) return rc;
  if ((rc = zk_verify_gens_check(c, "r1cs verify: gens_3", gens_3, 3))) return rc;
  if ((rc = zk_verify_gens_check(c, "r1cs verify: gens_4", gens_4, 4))) return rc;
  for (size_t i = 0; i < num_inputs; i++) if (!fr_canonical(input + 32 * i)) return fail(c, SBN_EINVAL, "r1cs verify: input[%zu] is not canonical  [scalar.rs:87-95]", i);
  for (size_t i = 0; i < 3; i++) if (!fr_canonical(evals + 32 * i)) return fail(c, SBN_EINVAL, "r1cs verify: evals[%zu] is not canonical  [scalar.rs:87-95]", i);
  std::lock_guard<std::mutex> g(c->mu); hipSetDevice(c->device);
  std::vector<uint8_t> rx(32 * s.nx), ry(32 * s.ny);
  rc = verify_on_copy(c, tr, accepted, [&](sbn_host::MerlinTranscript& t) {
    return r1cs_verify_locked(c, s, input, num_inputs, evals, gens_pc, gens_3, gens_4, proof, t, rx.data(), ry.data(), accepted);
  });
  if (rc == SBN_OK && *accepted) { memcpy(out_rx, rx.data(), rx.size()); memcpy(out_ry, ry.data(), ry.size()); }
  return rc;
}

}  // extern "C"
