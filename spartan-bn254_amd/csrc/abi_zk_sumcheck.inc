// abi_zk_sumcheck.inc — C ABI: the two ZK sumchecks of R1CSProof::prove (r1csproof.rs:295, :394) in ONE call each.
// sbn_zk_sumcheck_prove_r1cs is ZKSumcheckInstanceProof::prove_cubic_with_additive_term (sumcheck.rs:465-649), sbn_zk_sumcheck_prove_quad is
// ::prove_quad (sumcheck.rs:657-811), each with UniPoly::from_evals, the four commitments of a round and DotProductProof::prove
// (nizk/mod.rs:306-366) inside, the Merlin transcript on the host.
//
// Every group element of a round is a commitment over the one fixed set  gens_n.G ‖ gens_n.h ‖ gens_1.G[0] ‖ gens_1.h  (n + 3 points; the
// two h are DIFFERENT points, r1csproof.rs R1CSSumcheckGens::new, so they are ordinary columns and the set has no blind column), copied once
// per (gens_1, gens_n) pair with its lookup table and kept by gens_n.  A round is three two-row commits on the lookup path:
//   A_j = { comm_poly_j = [coeffs ‖ blinds_poly[j] ‖ 0 ‖ 0],  delta_j = [d_vec_j ‖ r_delta_j ‖ 0 ‖ 0] }      rows written by k_zk_round_tail
//   B_j = { comm_eval_j = [0 ‖ 0 ‖ eval ‖ blinds_evals[j]],  (round 0) comm_claim = [0 ‖ 0 ‖ claim ‖ blind_claim] }
//   C_j = { Cy_j = [0 ‖ 0 ‖ target ‖ blind],  beta_j = [0 ‖ 0 ‖ <a, d> ‖ r_beta_j] }
// (Cx of the dot product proof IS comm_poly_j: it is absorbed twice and computed once.)  B and C need only scalars the host holds; A_{j+1}
// needs the tables bound with r_j.  Queue order once r_j is drawn:  B_j, bind+eval(r_j), tail, A_{j+1}, then (w known) C_j — so the streaming
// round kernel runs under the host's transcript work, and the chain sums -> polynomial -> comm_poly has no host wait inside it.  The host
// waits three times a round: for B_j, for C_j, for A_{j+1}.  Each commit in flight has its own mailbox slot and sequence number (rows_to_host_launch /
// _collect, abi_proof_common.inc; the bullet rounds keep their words, which are slot 0's, under the same context mutex).
// Included by sbn254.hip.

// the derived set has 7 (r1cs) or 6 (quad) points: a lookup table of at most 64 MiB.  bases_build_comb takes the widest window that fits:
// 7 points get 13-bit windows (20 table points per scalar, 140 per row, 7 * 20 * 4096 * 64 B = 36.7 MB; 14 bits would need 69.7 MB),
// 6 points get 14-bit windows (19 per scalar, 114 per row, 6 * 19 * 8192 * 64 B = 59.8 MB) — the bullet sets' 3 GiB budget would buy
// 17-bit windows (15 points per scalar) at 440 MB per generator pair
static const size_t ZK_COMB_BYTES = (size_t)64 << 20;
template <int KIND> struct ZkShape { static constexpr int NT = KIND == KIND_QUAD ? 2 : 4, N = KIND == KIND_QUAD ? 3 : 4; };

// the derived set of a (gens_1, gens_n) pair, built on the first call and owned by gens_n; what tells it apart is gens_1's two points, which are
// read back on gens_1's first call only and kept on its handle — a later call finds its set without a copy or a wait
static int zk_ext(sbn_ctx* c, const sbn_bases* g1, const sbn_bases* gn, const sbn_bases** out) {
  int rc;
  {
    // (gens_1's handle is shared between contexts as the sets are: the sets' mutex; written once, so derived_set below may read it unlocked)
    std::lock_guard<std::mutex> tg(g_derived_mu);
    if (g1->zk_key.empty()) {
      if ((rc = ensure_pin(c, 4096))) return rc;
      HIPCHK(c, hipMemcpyAsync(c->pin, g1->d_pts, 128, hipMemcpyDeviceToHost, c->stream));
      HIPCHK(c, hipStreamSynchronize(c->stream));
      g1->zk_key.assign((const char*)c->pin, 128);
    }
  }
  return derived_set(gn, DERIVED_ZK, g1->zk_key, [&](sbn_bases** ext) -> int {
    const size_t n = gn->n;
    if ((rc = ensure(c, c->stage_pts, (n + 3) * 64))) return rc;
    uint8_t* P = (uint8_t*)c->stage_pts.p;
    HIPCHK(c, hipMemcpyAsync(P, gn->d_pts, (n + 1) * 64, hipMemcpyDeviceToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(P + 64 * (n + 1), g1->d_pts, 128, hipMemcpyDeviceToDevice, c->stream));
    if ((rc = bases_from_device(c, P, n + 3, nullptr, ext))) return rc;
    if (bases_build_comb(c, (*ext)->uniq ? (*ext)->uniq : *ext, ZK_COMB_BYTES) != SBN_OK) (void)hipGetLastError();     // best effort, as in bullet_begin_impl
    return SBN_OK;
  }, out);
}

// a commit in flight has its own words of the host mailbox: result slot `slot` and the flag word that belongs to it
static inline uint32_t zk_slot_word(int slot) { return (uint32_t)(SC_MBOX_FINALS + ZK_MBOX_SLOT_WORDS * slot); }
static inline uint32_t zk_flag_word(int slot) { return (uint32_t)(SC_MBOX_FLAGS + SC_PACK_MAX + 1 + slot); }
static inline uint32_t* zk_slot(sbn_ctx* c, int slot) { return c->mbox + zk_slot_word(slot); }
static inline uint32_t* zk_flag(sbn_ctx* c, int slot) { return c->mbox + zk_flag_word(slot); }

// the round kernel on the tables' current buffers: round 0's sums (bind == false) or the bind with rs fused with the next round's sums — the
// launches of sbn_sc_eval_* / sbn_sc_bind_eval_* for one instance (abi_tables.inc: sc_eval_launch / sc_fused_launch), results to `dmbox` (device memory)
template <int KIND>
static int zk_round_launch(sbn_ctx* c, sbn_table* const* T, bool bind, const ScScalar& rs, uint32_t* dmbox) {
  constexpr int NT = ZkShape<KIND>::NT;
  const size_t len = T[0]->len;
  int rc;
  const uint32_t seq = ++c->mbox_seq;
  if (!bind) {
    const unsigned gx = sc_eval_grid(c, len / 2, 1);
    if ((rc = ensure(c, c->sc_partial, (size_t)gx * 96))) return rc;
    ScArgsPack pack; memset(&pack, 0, sizeof pack);
    for (int j = 0; j < NT; j++) pack.a[0].t[j] = (const uint32_t*)T[j]->d;
    return sc_eval_launch<KIND>(c, pack, 1, len / 2, gx, dmbox, seq);
  }
  const size_t q = len / 4;
  const bool single = sc_fused_single(c, q);
  for (int j = 0; j < NT; j++) if ((rc = sc_second_buffer(c, T[j], len))) return rc;
  ScFusedPack pack; memset(&pack, 0, sizeof pack);
  for (int j = 0; j < NT; j++) { pack.a[0].src[j] = (const uint32_t*)T[j]->d; pack.a[0].dst[j] = (uint32_t*)T[j]->d2; }
  const unsigned gx = sc_fused_grid(c, q, 1, single);
  if ((rc = ensure(c, c->sc_partial, (size_t)gx * 96))) return rc;
  if ((rc = sc_fused_launch<KIND>(c, pack, 1, q, gx, single, rs, dmbox, seq))) return rc;
  for (int j = 0; j < NT; j++) sc_swap_bound(T[j], len);
  return SBN_OK;
}

static int zk_check(sbn_ctx* c, sbn_table* const* T, int nt, int n, const sbn_bases* g1, const sbn_bases* gn, const uint8_t* claim, const uint8_t* blind_claim, const uint8_t* rnd, size_t* rounds_out) {
  const size_t len = T[0]->len;
  for (int j = 1; j < nt; j++) if (T[j]->len != len) return fail(c, SBN_EINVAL, "zk sumcheck: tables differ in length");
  for (int j = 0; j < nt; j++) for (int k = 0; k < j; k++) if (T[j] == T[k]) return fail(c, SBN_EINVAL, "zk sumcheck: the same table handle was passed twice (each table is bound in place)");
  if (len < 2 || (len & (len - 1))) return fail(c, SBN_EINVAL, "zk sumcheck: table length %zu (a power of two >= 2 is needed)", len);
  if (g1->n != 1 || !g1->has_h) return fail(c, SBN_EINVAL, "zk sumcheck: gens_1 has %zu points%s, one generator with h is needed  [nizk/mod.rs:323 assert_eq]", g1->n, g1->has_h ? "" : " and no h");
  if (gn->n != (size_t)n || !gn->has_h) return fail(c, SBN_EINVAL, "zk sumcheck: gens_n has %zu points%s, %d generators with h are needed  [nizk/mod.rs:322 assert_eq]", gn->n, gn->has_h ? "" : " and no h", n);
  if (!fr_canonical(claim) || !fr_canonical(blind_claim)) return fail(c, SBN_EINVAL, "zk sumcheck: claim / blind_claim is not canonical");
  size_t rounds = 0; while (((size_t)1 << rounds) < len) rounds++;
  for (size_t i = 0; i < rounds * (size_t)(n + 4); i++) if (!fr_canonical(rnd + 32 * i)) return fail(c, SBN_EINVAL, "zk sumcheck: rnd[%zu] is not canonical", i);
  *rounds_out = rounds;
  return SBN_OK;
}

// the proof on the transcript `t` (a copy of the caller's); arguments already checked
template <int KIND>
static int zk_prove_locked(sbn_ctx* c, sbn_table* const* T, const sbn_bases* g1, const sbn_bases* gn, size_t rounds, const uint8_t* claim0, const uint8_t* blind_claim,
                           const uint8_t* rnd, sbn_host::MerlinTranscript& t, uint8_t* out_proof, uint8_t* out_r, uint8_t* out_finals, uint8_t* out_blind) {
  using namespace sbn_host::fr;
  constexpr int NT = ZkShape<KIND>::NT, N = ZkShape<KIND>::N, R = N + 3;
  const size_t stride = (size_t)(6 + N) * 32;                    // bytes of one round in out_proof
  const uint8_t* blinds_poly = rnd; const uint8_t* blinds_evals = rnd + 32 * rounds;
  auto dp_rnd = [&](size_t j) { return rnd + 32 * (2 * rounds + j * (size_t)(N + 2)); };     // d_vec_j[N], r_delta_j, r_beta_j
  sbn_host::Script ts{t};
  int rc;
  const sbn_bases* ext = nullptr;
  if ((rc = zk_ext(c, g1, gn, &ext))) return rc;
  if ((rc = sc_tickets(c))) return rc;
  if ((rc = ensure(c, c->wsum, 4096))) return rc;                // (the commits ask for 2 x 128 B: sized here so that it never reallocates mid-call)
  // device scratch: [the mailbox's twin | rnd | rows A | rows B | rows C | coefficients]
  const size_t nrnd = rounds * (size_t)(N + 4);
  const size_t o_mbox = 0, o_rnd = ((size_t)SC_MBOX_WORDS * 4 + 255) / 256 * 256, o_ra = o_rnd + (nrnd * 32 + 255) / 256 * 256, o_rb = o_ra + 512, o_rc = o_rb + 512, o_co = o_rc + 512, total = o_co + 256;
  static_assert(2 * R * 32 <= 512, "two rows fit their area");
  if ((rc = ensure(c, c->sc_prove, total))) return rc;
  if ((rc = ensure_pin(c, 4096 + nrnd * 32))) return rc;
  uint8_t* d = (uint8_t*)c->sc_prove.p;
  uint32_t* dmbox = (uint32_t*)(d + o_mbox); uint32_t* d_rnd = (uint32_t*)(d + o_rnd);
  uint32_t* rowsA = (uint32_t*)(d + o_ra); uint32_t* rowsB = (uint32_t*)(d + o_rb); uint32_t* rowsC = (uint32_t*)(d + o_rc); uint32_t* d_co = (uint32_t*)(d + o_co);
  memcpy((uint8_t*)c->pin + 4096, rnd, nrnd * 32);
  HIPCHK(c, hipMemcpyAsync(d_rnd, (uint8_t*)c->pin + 4096, nrnd * 32, hipMemcpyHostToDevice, c->stream));

  auto tail_and_A = [&](size_t j, const El& claim, uint32_t* seq) -> int {
    ZkTailArgs a; a.sums = dmbox; a.rnd = d_rnd; a.rows = rowsA; a.coeffs = d_co; a.blind_idx = (uint32_t)j; a.d_idx = (uint32_t)(2 * rounds + j * (size_t)(N + 2));
    LAUNCH(c, "k_zk_round_tail", k_zk_round_tail<KIND>, 1, 64, a, scs_from(to_dev_mont(claim)));
    return rows_to_host_launch(c, ext, rowsA, nullptr, 2, R, d_co, 8 * N, zk_slot_word(0), zk_flag_word(0), seq);
  };
  auto collect = [&](int slot, uint32_t seq, uint8_t xy[128], uint8_t* extra, size_t nextra) { return rows_to_host_collect(c, zk_slot_word(slot), zk_flag_word(slot), seq, 2, xy, nullptr, extra, nextra); };
  auto host_rows = [&](uint32_t* rows, const El& v0, const uint8_t* b0, const El* v1, const uint8_t* b1, int slot, uint32_t* seq) -> int {
    ScScalar s0 = scs_from(v0), s1, s2, s3; memcpy(s1.v, b0, 32); memset(&s2, 0, sizeof s2); memset(&s3, 0, sizeof s3);
    if (v1) { s2 = scs_from(*v1); memcpy(s3.v, b1, 32); }
    LAUNCH(c, "k_zk_host_rows", k_zk_host_rows, 1, 64, rows, (uint32_t)N, s0, s1, s2, s3);
    return rows_to_host_launch(c, ext, rows, nullptr, 2, R, nullptr, 0u, zk_slot_word(slot), zk_flag_word(slot), seq);
  };

  El claim = el_from(claim0);
  const uint8_t* blind_sc = blind_claim;
  uint8_t comm_claim[32];                                         // comm_claim_per_round, compressed
  ScScalar zero_s; memset(&zero_s, 0, sizeof zero_s);
  uint32_t seqA = 0, seqB = 0, seqC = 0, seqF = 0;
  if ((rc = zk_round_launch<KIND>(c, T, false, zero_s, dmbox))) return rc;
  if ((rc = tail_and_A(0, claim, &seqA))) return rc;
  for (size_t j = 0; j < rounds; j++) {
    uint8_t* pr = out_proof + stride * j;
    uint8_t* comm_poly = pr; uint8_t* comm_eval = pr + 32; uint8_t* delta = pr + 64; uint8_t* beta = pr + 96;
    uint8_t xy[128], co[32 * N];
    if ((rc = collect(0, seqA, xy, co, 32 * N))) return rc;
    sbn_host::g1_compress(xy + 64, delta);
    ts.point_xy("comm_poly", xy, comm_poly);                      // sumcheck.rs:544
    uint8_t rj[32];
    ts.challenge("challenge_nextround", rj);                      // :548
    memcpy(out_r + 32 * j, rj, 32);
    const El r = el_from(rj);
    El x[N], pw[N];                                               // the coefficients; 1, r, r^2 ..
    for (int k = 0; k < N; k++) x[k] = el_from(co + 32 * k);
    pw[0] = from_u64(1); for (int k = 1; k < N; k++) pw[k] = fmul(pw[k - 1], r);
    El eval = x[0]; for (int k = 1; k < N; k++) eval = add(eval, fmul(pw[k], x[k]));      // poly.evaluate(r_j), unipoly.rs:77-85
    // B_j, then the bind with r_j fused with the next round's sums, its tail and A_{j+1}
    if ((rc = host_rows(rowsB, eval, blinds_evals + 32 * j, j == 0 ? &claim : nullptr, blind_claim, 1, &seqB))) return rc;
    const ScScalar rs = scs_from(to_dev_mont(r));
    if (T[0]->len >= 4) {
      if ((rc = zk_round_launch<KIND>(c, T, true, rs, dmbox))) return rc;
      if ((rc = tail_and_A(j + 1, eval, &seqA))) return rc;
    } else {
      ZkTabs zt; memset(&zt, 0, sizeof zt);
      for (int k = 0; k < NT; k++) zt.p[k] = (uint32_t*)T[k]->d;
      seqF = ++c->mbox_seq;
      LAUNCH(c, "k_bind_top", k_zk_bind_last, 1, 64, zt, (uint32_t)NT, rs, zk_slot(c, 3), zk_flag(c, 3), seqF);
      LAUNCHCHK(c);
      for (int k = 0; k < NT; k++) T[k]->len = 1;
    }
    if ((rc = collect(1, seqB, xy, nullptr, 0))) return rc;
    if (j == 0) sbn_host::g1_compress(xy + 64, comm_claim);       // claim.commit(blind_claim, gens_1), sumcheck.rs:487
    ts.point("comm_claim_per_round", comm_claim);                 // :571-572
    ts.point_xy("comm_eval", xy, comm_eval);
    uint8_t wb[64];
    ts.challenges("combine_two_claims_to_one", wb, 2);            // :575
    const El w0 = el_from(wb), w1 = el_from(wb + 32);
    const El target = add(fmul(w0, claim), fmul(w1, eval));       // :578
    const El blind = add(fmul(w0, el_from(blind_sc)), fmul(w1, el_from(blinds_evals + 32 * j)));      // :586-594
    El a[N], ad = from_u64(0);
    const uint8_t* dv = dp_rnd(j); const uint8_t* r_delta = dv + 32 * N; const uint8_t* r_beta = r_delta + 32;
    for (int k = 0; k < N; k++) {                                 // a = w0 * [2, 1, 1 ..] + w1 * [1, r, r^2 ..]   (:597-619)
      a[k] = add(k == 0 ? add(w0, w0) : w0, fmul(w1, pw[k]));
      ad = add(ad, fmul(a[k], el_from(dv + 32 * k)));             // <a, d>, nizk/mod.rs:341
    }
    uint8_t blind_b[32]; memcpy(blind_b, blind.v, 32);
    if ((rc = host_rows(rowsC, target, blind_b, &ad, r_beta, 2, &seqC))) return rc;
    ts.protocol("dot product proof");                             // nizk/mod.rs:318
    ts.point("Cx", comm_poly);                                    // :330-331: x_vec.commit(blind_x, gens_n) is comm_poly_j
    uint8_t cy[32];
    if ((rc = collect(2, seqC, xy, nullptr, 0))) return rc;
    ts.point_xy("Cy", xy, cy);
    ts.scalars("a", a, N);                                        // :336
    ts.point("delta", delta);
    ts.point_xy("beta", xy + 64, beta);
    uint8_t cb[32];
    ts.challenge("c", cb);
    const El cc = el_from(cb);
    uint8_t* z = pr + 128;
    for (int k = 0; k < N; k++) { const El zk = add(fmul(cc, x[k]), el_from(dv + 32 * k)); memcpy(z + 32 * k, zk.v, 32); }      // :348-350
    const El z_delta = add(fmul(cc, el_from(blinds_poly + 32 * j)), el_from(r_delta)), z_beta = add(fmul(cc, blind), el_from(r_beta));
    memcpy(z + 32 * N, z_delta.v, 32); memcpy(z + 32 * N + 32, z_beta.v, 32);
    claim = eval; blind_sc = blinds_evals + 32 * j;               // sumcheck.rs:637-640
    memcpy(comm_claim, comm_eval, 32);
  }
  if ((rc = sc_flag_wait(c, zk_flag(c, 3), seqF))) return rc;
  memcpy(out_finals, zk_slot(c, 3), 32 * NT);
  memcpy(out_blind, blinds_evals + 32 * (rounds - 1), 32);
  if (c->prof) { HIPCHK(c, hipStreamSynchronize(c->stream)); prof_drain(c); }
  return SBN_OK;
}

template <int KIND>
static int zk_prove_entry(sbn_ctx* c, sbn_table* const* T, const sbn_bases* g1, const sbn_bases* gn, const uint8_t* claim, const uint8_t* blind_claim, const uint8_t* rnd,
                          sbn_transcript* tr, uint8_t* out_proof, uint8_t* out_r, uint8_t* out_finals, uint8_t* out_blind) {
  if (!c || !g1 || !gn || !claim || !blind_claim || !rnd || !tr || !out_proof || !out_r || !out_finals || !out_blind) return SBN_EINVAL;
  for (int j = 0; j < ZkShape<KIND>::NT; j++) if (!T[j]) return SBN_EINVAL;
  std::lock_guard<std::mutex> g(c->mu); hipSetDevice(c->device);
  int rc; size_t rounds = 0;
  if ((rc = zk_check(c, T, ZkShape<KIND>::NT, ZkShape<KIND>::N, g1, gn, claim, blind_claim, rnd, &rounds))) return rc;
  return prove_on_copy(c, tr, [&](sbn_host::MerlinTranscript& t) { return zk_prove_locked<KIND>(c, T, g1, gn, rounds, claim, blind_claim, rnd, t, out_proof, out_r, out_finals, out_blind); });
}

extern "C" {

int sbn_zk_sumcheck_prove_r1cs(sbn_ctx* c, sbn_table* tau, sbn_table* Az, sbn_table* Bz, sbn_table* Cz, const sbn_bases* gens_1, const sbn_bases* gens_4,
                               const uint8_t claim[32], const uint8_t blind_claim[32], const uint8_t* rnd, sbn_transcript* tr,
                               uint8_t* out_proof, uint8_t* out_r, uint8_t out_finals[128], uint8_t out_blind[32]) {
  sbn_table* T[4] = {tau, Az, Bz, Cz};
  return zk_prove_entry<KIND_R1CS>(c, T, gens_1, gens_4, claim, blind_claim, rnd, tr, out_proof, out_r, out_finals, out_blind);
}

int sbn_zk_sumcheck_prove_quad(sbn_ctx* c, sbn_table* Z, sbn_table* ABC, const sbn_bases* gens_1, const sbn_bases* gens_3,
                               const uint8_t claim[32], const uint8_t blind_claim[32], const uint8_t* rnd, sbn_transcript* tr,
                               uint8_t* out_proof, uint8_t* out_r, uint8_t out_finals[64], uint8_t out_blind[32]) {
  sbn_table* T[2] = {Z, ABC};
  return zk_prove_entry<KIND_QUAD>(c, T, gens_1, gens_3, claim, blind_claim, rnd, tr, out_proof, out_r, out_finals, out_blind);
}

}  // extern "C"
