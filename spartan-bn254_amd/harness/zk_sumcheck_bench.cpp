// zk_sumcheck_bench.cpp — a compiled CALLER of the C ABI (plain g++, no HIP) that times one ZK sumcheck of R1CSProof::prove
// (ZKSumcheckInstanceProof::prove_cubic_with_additive_term, sumcheck.rs:465-649, or ::prove_quad, sumcheck.rs:657-811) two ways, Merlin
// transcript included:
//   mode 0: the round loop a caller had to write before sbn_zk_sumcheck_prove_* — sbn_sc_eval_* / sbn_sc_bind_eval_* / sbn_bind_top_many,
//           sbn_unipoly_from_evals, one-row sbn_commit_rows for comm_poly, comm_eval, Cy, delta and beta, sbn_g1_compress and sbn_transcript_*
//           — with its own Fr arithmetic for eval, target, blind, a, <a, d>, z, z_delta and z_beta (Montgomery products on 4 x 64-bit limbs);
//   mode 1: sbn_zk_sumcheck_prove_r1cs / _quad;
//   mode 2: mode 0 with a lookup table on both generator handles (sbn_bases_precompute, 64 MiB each — what the one call gives its derived
//           set), built outside the timed region: the loop a caller who cares about time writes, and the leg the one call is compared with.
// Both prove the same tables with the same claim and draws from the same transcript state and must end with the same bytes (the digest
// returned).  Generator handles (and the sets derived from them) are made once, outside the timed region; the tables are uploaded afresh
// before every proof (a proof binds them in place), outside it too.  tools/bench_zk_sumcheck.py drives it.
#include "../../include/sbn254.h"
#include <chrono>
#include <cstdint>
#include <cstring>
#include <vector>

typedef unsigned __int128 u128;
struct El { uint64_t v[4]; };
static const uint64_t P[4] = {0x43e1f593f0000001ull, 0x2833e84879b97091ull, 0xb85045b68181585dull, 0x30644e72e131a029ull};
static const uint64_t NINV = 0xc2e1f593efffffffull;
static const uint64_t R2[4] = {0x1bb8e645ae216da7ull, 0x53fe3ab1e35c59e3ull, 0x8c49833d53bb8085ull, 0x0216d0b17f4e44a5ull};   // 2^512 mod r
static bool geq(const uint64_t a[4]) { for (int i = 3; i >= 0; i--) { if (a[i] > P[i]) return true; if (a[i] < P[i]) return false; } return true; }
static void subp(uint64_t a[4]) { uint64_t br = 0; for (int i = 0; i < 4; i++) { u128 d = (u128)a[i] - P[i] - br; a[i] = (uint64_t)d; br = (uint64_t)(d >> 127); } }
static El add(const El& a, const El& b) {
  El r; uint64_t c = 0;
  for (int i = 0; i < 4; i++) { u128 s = (u128)a.v[i] + b.v[i] + c; r.v[i] = (uint64_t)s; c = (uint64_t)(s >> 64); }
  if (c || geq(r.v)) subp(r.v);
  return r;
}
static El sub(const El& a, const El& b) {
  El r; uint64_t br = 0;
  for (int i = 0; i < 4; i++) { u128 d = (u128)a.v[i] - b.v[i] - br; r.v[i] = (uint64_t)d; br = (uint64_t)(d >> 127); }
  if (br) { uint64_t c = 0; for (int i = 0; i < 4; i++) { u128 s = (u128)r.v[i] + P[i] + c; r.v[i] = (uint64_t)s; c = (uint64_t)(s >> 64); } }
  return r;
}
static El mmul(const El& a, const El& b) {               // a * b * 2^-256 mod r (CIOS)
  uint64_t t[6] = {0, 0, 0, 0, 0, 0};
  for (int i = 0; i < 4; i++) {
    uint64_t c = 0;
    for (int j = 0; j < 4; j++) { u128 s = (u128)a.v[j] * b.v[i] + t[j] + c; t[j] = (uint64_t)s; c = (uint64_t)(s >> 64); }
    u128 s = (u128)t[4] + c; t[4] = (uint64_t)s; t[5] = (uint64_t)(s >> 64);
    const uint64_t m = t[0] * NINV;
    s = (u128)m * P[0] + t[0]; c = (uint64_t)(s >> 64);
    for (int j = 1; j < 4; j++) { s = (u128)m * P[j] + t[j] + c; t[j - 1] = (uint64_t)s; c = (uint64_t)(s >> 64); }
    s = (u128)t[4] + c; t[3] = (uint64_t)s; t[4] = t[5] + (uint64_t)(s >> 64);
  }
  El r = {{t[0], t[1], t[2], t[3]}};
  if (t[4] || geq(r.v)) subp(r.v);
  return r;
}
static El to_m(const El& a) { El r2; memcpy(r2.v, R2, 32); return mmul(a, r2); }
static El mul(const El& a, const El& b) { return mmul(to_m(a), b); }     // canonical in, canonical out
static El ld(const uint8_t* b) { El e; memcpy(e.v, b, 32); return e; }
static uint64_t fnv(uint64_t h, const uint8_t* p, size_t n) { for (size_t i = 0; i < n; i++) { h ^= p[i]; h *= 0x100000001b3ull; } return h; }
static void append(sbn_transcript* tr, const char* label, const uint8_t* msg, size_t n) { sbn_transcript_append_message(tr, (const uint8_t*)label, strlen(label), msg, n); }
static void challenge(sbn_transcript* tr, const char* label, uint8_t out[32]) { sbn_transcript_challenge_scalar(tr, (const uint8_t*)label, strlen(label), out); }

struct Setup { sbn_bases* g1 = nullptr; sbn_bases* gn = nullptr; int nt = 0, n = 0; size_t len = 0, rounds = 0; void* master = nullptr; sbn_table* T[4] = {nullptr, nullptr, nullptr, nullptr}; };

// one commitment: a one-row sbn_commit_rows over `b` (k scalars, one blind), compressed
static int commit1(sbn_ctx* ctx, const sbn_bases* b, const uint8_t* scalars, size_t k, const uint8_t* blind, uint8_t out32[32]) {
  uint8_t xy[64], inf = 0;
  int rc = sbn_commit_rows(ctx, b, scalars, blind, 1, k, 0, xy, &inf);
  if (rc) return rc;
  return sbn_g1_compress(xy, 1, out32);
}

// the prover through the calls that existed before sbn_zk_sumcheck_prove_*; out_* as the one call lays them out
static int loop_prove(sbn_ctx* ctx, Setup& S, const uint8_t* claim0, const uint8_t* blind_claim, const uint8_t* rnd, sbn_transcript* tr,
                      uint8_t* proof, uint8_t* out_r, uint8_t* finals, uint8_t* out_blind) {
  const int n = S.n; const bool quad = S.nt == 2;
  const size_t rounds = S.rounds, stride = (size_t)(6 + n) * 32;
  const uint8_t* blinds_poly = rnd; const uint8_t* blinds_evals = rnd + 32 * rounds;
  int rc;
  uint8_t sums[96], comm_claim[32];
  El claim = ld(claim0);
  const uint8_t* blind_sc = blind_claim;
  if ((rc = commit1(ctx, S.g1, claim0, 1, blind_claim, comm_claim))) return rc;
  rc = quad ? sbn_sc_eval_quad(ctx, S.T[0], S.T[1], sums) : sbn_sc_eval_r1cs(ctx, S.T[0], S.T[1], S.T[2], S.T[3], sums);
  if (rc) return rc;
  for (size_t j = 0; j < rounds; j++) {
    uint8_t* pr = proof + stride * j;
    uint8_t* comm_poly = pr; uint8_t* comm_eval = pr + 32; uint8_t* delta = pr + 64; uint8_t* beta = pr + 96; uint8_t* z = pr + 128;
    const uint8_t* dv = rnd + 32 * (2 * rounds + j * (size_t)(n + 2)); const uint8_t* r_delta = dv + 32 * n; const uint8_t* r_beta = r_delta + 32;
    uint8_t ev[128], co[128];
    const El e1 = sub(claim, ld(sums));
    memcpy(ev, sums, 32); memcpy(ev + 32, e1.v, 32); memcpy(ev + 64, sums + 32, 32 * (size_t)(n - 2));
    if ((rc = sbn_unipoly_from_evals(ev, (size_t)n, co))) return rc;
    if ((rc = commit1(ctx, S.gn, co, (size_t)n, blinds_poly + 32 * j, comm_poly))) return rc;
    append(tr, "comm_poly", comm_poly, 32);
    uint8_t rj[32];
    challenge(tr, "challenge_nextround", rj);
    memcpy(out_r + 32 * j, rj, 32);
    if (S.len >> j >= 4) rc = quad ? sbn_sc_bind_eval_quad(ctx, S.T[0], S.T[1], rj, sums) : sbn_sc_bind_eval_r1cs(ctx, S.T[0], S.T[1], S.T[2], S.T[3], rj, sums);
    else rc = sbn_bind_top_many(ctx, S.T, (size_t)S.nt, rj);
    if (rc) return rc;
    const El r = ld(rj);
    El x[4], pw[4];
    for (int k = 0; k < n; k++) x[k] = ld(co + 32 * k);
    pw[0] = El{{1, 0, 0, 0}}; for (int k = 1; k < n; k++) pw[k] = mul(pw[k - 1], r);
    El eval = x[0]; for (int k = 1; k < n; k++) eval = add(eval, mul(pw[k], x[k]));
    if ((rc = commit1(ctx, S.g1, (const uint8_t*)eval.v, 1, blinds_evals + 32 * j, comm_eval))) return rc;
    append(tr, "comm_claim_per_round", comm_claim, 32); append(tr, "comm_eval", comm_eval, 32);
    uint8_t wb[64];
    challenge(tr, "combine_two_claims_to_one", wb); challenge(tr, "combine_two_claims_to_one", wb + 32);
    const El w0 = ld(wb), w1 = ld(wb + 32);
    const El target = add(mul(w0, claim), mul(w1, eval));
    const El blind = add(mul(w0, ld(blind_sc)), mul(w1, ld(blinds_evals + 32 * j)));
    El a[4], ad = {{0, 0, 0, 0}};
    for (int k = 0; k < n; k++) { a[k] = add(k == 0 ? add(w0, w0) : w0, mul(w1, pw[k])); ad = add(ad, mul(a[k], ld(dv + 32 * k))); }
    append(tr, "protocol-name", (const uint8_t*)"dot product proof", 17);
    append(tr, "Cx", comm_poly, 32);
    uint8_t cy[32];
    if ((rc = commit1(ctx, S.g1, (const uint8_t*)target.v, 1, (const uint8_t*)blind.v, cy))) return rc;
    append(tr, "Cy", cy, 32);
    for (int k = 0; k < n; k++) append(tr, "a", (const uint8_t*)a[k].v, 32);
    if ((rc = commit1(ctx, S.gn, dv, (size_t)n, r_delta, delta))) return rc;
    append(tr, "delta", delta, 32);
    if ((rc = commit1(ctx, S.g1, (const uint8_t*)ad.v, 1, r_beta, beta))) return rc;
    append(tr, "beta", beta, 32);
    uint8_t cb[32];
    challenge(tr, "c", cb);
    const El cc = ld(cb);
    for (int k = 0; k < n; k++) { const El zk = add(mul(cc, x[k]), ld(dv + 32 * k)); memcpy(z + 32 * k, zk.v, 32); }
    const El z_delta = add(mul(cc, ld(blinds_poly + 32 * j)), ld(r_delta)), z_beta = add(mul(cc, blind), ld(r_beta));
    memcpy(z + 32 * n, z_delta.v, 32); memcpy(z + 32 * n + 32, z_beta.v, 32);
    claim = eval; blind_sc = blinds_evals + 32 * j; memcpy(comm_claim, comm_eval, 32);
  }
  if ((rc = sbn_table_read0_many(ctx, (const sbn_table* const*)S.T, (size_t)S.nt, finals))) return rc;
  memcpy(out_blind, blinds_evals + 32 * (rounds - 1), 32);
  return SBN_OK;
}

// kind 0: r1cs (4 tables, 4 coefficients), 1: quad (2 tables, 3 coefficients); log_len: the tables have 2^log_len entries
extern "C" int sbn_bench_zk_sumcheck(sbn_ctx* ctx, int kind, int log_len, int mode, int reps, double* out_us /* reps */, uint64_t* out_digest) {
  if (!ctx || kind < 0 || kind > 1 || log_len < 1 || log_len > 26 || mode < 0 || mode > 2 || reps < 1 || !out_us || !out_digest) return SBN_EINVAL;
  Setup S; int rc;
  S.nt = kind ? 2 : 4; S.n = kind ? 3 : 4; S.rounds = (size_t)log_len; S.len = (size_t)1 << log_len;
  const size_t tab_bytes = S.len * 32, nrnd = S.rounds * (size_t)(S.n + 4);
  rc = sbn_gens_new(ctx, 1, (const uint8_t*)"gens_zk_bench_pc", 16, nullptr, &S.g1);
  if (!rc) rc = sbn_gens_new(ctx, (size_t)S.n, (const uint8_t*)"gens_zk_bench_sc", 16, nullptr, &S.gn);
  if (!rc && mode == 2) rc = sbn_bases_precompute(ctx, S.g1, (size_t)64 << 20, nullptr);
  if (!rc && mode == 2) rc = sbn_bases_precompute(ctx, S.gn, (size_t)64 << 20, nullptr);
  if (!rc) rc = sbn_dev_alloc(ctx, tab_bytes * S.nt, &S.master);
  if (!rc) rc = sbn_scalars_synthetic(ctx, 0x2c5a17e5ull + (uint64_t)kind, 0, S.len * S.nt, S.master);
  std::vector<uint8_t> host;
  std::vector<uint8_t> rnd(32 * nrnd, 0), proof((size_t)(6 + S.n) * 32 * S.rounds), rs(32 * S.rounds);
  for (size_t j = 0; j < nrnd; j++) { rnd[32 * j] = (uint8_t)(9 + j); rnd[32 * j + 11] = (uint8_t)(0x33 + 5 * j); rnd[32 * j + 30] = (uint8_t)(1 + j); }
  uint8_t claim[32] = {7, 1, 0, 9}, blind_claim[32] = {3, 0, 5};
  uint64_t digest = 0xcbf29ce484222325ull;
  if (!rc) { host.resize(tab_bytes * S.nt); rc = sbn_dev_download(ctx, host.data(), S.master, host.size()); }
  for (int rep = -1; rep < reps && !rc; rep++) {             // rep -1: untimed — the derived set and its lookup table are built there
    // fresh tables for every proof (they are bound in place): re-uploaded outside the timed region
    for (int t = 0; t < S.nt && !rc; t++) rc = sbn_table_upload(ctx, host.data() + tab_bytes * t, S.len, 0, &S.T[t]);
    sbn_transcript* tr = nullptr; uint8_t fin[128], bl[32];
    if (!rc) rc = sbn_transcript_new((const uint8_t*)"zk sumcheck bench", 17, &tr);
    if (!rc) rc = sbn_ctx_sync(ctx);
    if (!rc) {
      const auto t0 = std::chrono::steady_clock::now();
      if (mode == 1)
        rc = kind ? sbn_zk_sumcheck_prove_quad(ctx, S.T[0], S.T[1], S.g1, S.gn, claim, blind_claim, rnd.data(), tr, proof.data(), rs.data(), fin, bl)
                  : sbn_zk_sumcheck_prove_r1cs(ctx, S.T[0], S.T[1], S.T[2], S.T[3], S.g1, S.gn, claim, blind_claim, rnd.data(), tr, proof.data(), rs.data(), fin, bl);
      else rc = loop_prove(ctx, S, claim, blind_claim, rnd.data(), tr, proof.data(), rs.data(), fin, bl);
      const auto t1 = std::chrono::steady_clock::now();
      if (rep >= 0) out_us[rep] = std::chrono::duration<double, std::micro>(t1 - t0).count();
      if (!rc && rep == 0) {
        uint8_t state[203]; sbn_transcript_state(tr, state);
        digest = fnv(fnv(fnv(fnv(fnv(digest, proof.data(), proof.size()), rs.data(), rs.size()), fin, 32 * (size_t)S.nt), bl, 32), state, 203);
      }
    }
    if (tr) sbn_transcript_free(tr);
    for (int t = 0; t < S.nt; t++) if (S.T[t]) { sbn_table_free(ctx, S.T[t]); S.T[t] = nullptr; }
  }
  *out_digest = digest;
  if (S.master) sbn_dev_free(ctx, S.master);
  if (S.gn) sbn_bases_free(ctx, S.gn);
  if (S.g1) sbn_bases_free(ctx, S.g1);
  return rc;
}
