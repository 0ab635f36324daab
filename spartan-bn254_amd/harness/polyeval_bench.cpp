// polyeval_bench.cpp — a compiled CALLER of the C ABI (plain g++, no HIP) that times one Hyrax opening (PolyEvalProof::prove, hyrax.rs:65-116)
// two ways, Merlin transcript included:
//   mode 0: the loop a caller had to write before sbn_polyeval_prove — sbn_eq_evals, sbn_table_bound, sbn_commit_table (Cx), sbn_msm (Cy, delta,
//           beta), sbn_bullet_begin_scaled / _cross / _fold_cross / _fold / _finish, sbn_g1_compress and sbn_transcript_* — with its own Fr
//           arithmetic for u^-1, the blind fold, d * r, z1 and z2 (Montgomery products on 4 x 64-bit limbs, Fermat inversion);
//   mode 1: sbn_polyeval_prove.
// Both open the same table at the same point with the same draws from the same transcript state and must end with the same bytes (the digest
// returned).  The generator handle (and the sets derived from it) is made once, outside the timed region.  tools/bench_polyeval.py drives it.
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
static El inv(const El& a) {                              // a^(r - 2)
  const uint64_t e[4] = {P[0] - 2, P[1], P[2], P[3]};
  const El am = to_m(a); El one = {{1, 0, 0, 0}}; El acc = to_m(one);
  for (int i = 255; i >= 0; i--) { acc = mmul(acc, acc); if ((e[i >> 6] >> (i & 63)) & 1) acc = mmul(acc, am); }
  return mmul(acc, one);
}
static El ld(const uint8_t* b) { El e; memcpy(e.v, b, 32); return e; }
static uint64_t fnv(uint64_t h, const uint8_t* p, size_t n) { for (size_t i = 0; i < n; i++) { h ^= p[i]; h *= 0x100000001b3ull; } return h; }
static void append_point(sbn_transcript* tr, const char* label, const uint8_t xy[64], uint8_t out32[32]) {
  sbn_g1_compress(xy, 1, out32);
  sbn_transcript_append_message(tr, (const uint8_t*)label, strlen(label), out32, 32);
}

struct Setup { sbn_bases* gens = nullptr; sbn_bases* Gn = nullptr; sbn_bases* G1 = nullptr; std::vector<uint8_t> xy; void* mem = nullptr; sbn_table* Z = nullptr; };

// the opening through the calls that existed before sbn_polyeval_prove (no blinds: the HashLayerProof openings' shape)
static int loop_opening(sbn_ctx* ctx, const Setup& S, const uint8_t* r, size_t ell, const uint8_t* Zr, const uint8_t* rnd, sbn_transcript* tr, uint8_t* proof, uint8_t* Cx, uint8_t* Cy) {
  const size_t ml = ell / 2, mr = ell - ml, n = (size_t)1 << mr, lg = mr;
  const uint8_t* Qb = S.xy.data() + 64 * n; const uint8_t* H = Qb + 64;
  sbn_table *Lt = nullptr, *Rt = nullptr, *LZ = nullptr; sbn_bullet* st = nullptr;
  int rc;
  auto done = [&](int code) { if (st) sbn_bullet_free(ctx, st); if (LZ) sbn_table_free(ctx, LZ); if (Rt) sbn_table_free(ctx, Rt); if (Lt) sbn_table_free(ctx, Lt); return code; };
  sbn_transcript_append_message(tr, (const uint8_t*)"protocol-name", 13, (const uint8_t*)"polynomial evaluation proof", 27);
  sbn_transcript_append_message(tr, (const uint8_t*)"protocol-name", 13, (const uint8_t*)"dot product proof (log)", 23);
  if ((rc = sbn_eq_evals(ctx, r, ml, &Lt)) || (rc = sbn_eq_evals(ctx, r + 32 * ml, mr, &Rt)) || (rc = sbn_table_bound(ctx, S.Z, Lt, &LZ))) return done(rc);
  uint8_t inf1 = 0; int inf = 0;
  if ((rc = sbn_commit_table(ctx, S.Gn, LZ, nullptr, 1, n, Cx, &inf1))) return done(rc);
  uint8_t sc[64], pts[128], comp[32];
  memcpy(sc, Zr, 32); memset(sc + 32, 0, 32); memcpy(pts, Qb, 64); memcpy(pts + 64, H, 64);
  if ((rc = sbn_msm(ctx, sc, pts, 2, 0, Cy, &inf))) return done(rc);
  append_point(tr, "Cx", Cx, comp); append_point(tr, "Cy", Cy, comp);
  std::vector<uint8_t> Rb(32 * n);
  if ((rc = sbn_table_download(ctx, Rt, Rb.data()))) return done(rc);
  for (size_t i = 0; i < n; i++) sbn_transcript_append_message(tr, (const uint8_t*)"a", 1, &Rb[32 * i], 32);
  uint8_t rq[32];
  sbn_transcript_challenge_scalar(tr, (const uint8_t*)"r", 1, rq);
  if ((rc = sbn_bullet_begin_scaled(ctx, S.Gn, Qb, rq, LZ, Rt, nullptr, nullptr, nullptr, &st))) return done(rc);
  El blind_G = {{0, 0, 0, 0}};
  uint8_t u[32], ui[32];
  for (size_t j = 0; j < lg; j++) {
    const uint8_t* bL = rnd + 96 + 64 * j; const uint8_t* bR = bL + 32;
    uint8_t Lxy[64], Rxy[64], cl[32], cr[32]; int li, ri;
    rc = j == 0 ? sbn_bullet_cross(ctx, st, bL, bR, Lxy, &li, Rxy, &ri, cl, cr) : sbn_bullet_fold_cross(ctx, st, u, ui, bL, bR, Lxy, &li, Rxy, &ri, cl, cr);
    if (rc) return done(rc);
    append_point(tr, "L", Lxy, proof + 32 * j); append_point(tr, "R", Rxy, proof + 32 * (lg + j));
    sbn_transcript_challenge_scalar(tr, (const uint8_t*)"u", 1, u);
    const El eu = ld(u), eui = inv(eu);
    memcpy(ui, eui.v, 32);
    blind_G = add(add(mul(mul(eu, eu), ld(bL)), blind_G), mul(mul(eui, eui), ld(bR)));
  }
  uint8_t ah[32], bh[32], gh[64];
  if ((rc = sbn_bullet_fold(ctx, st, u, ui)) || (rc = sbn_bullet_finish(ctx, st, ah, bh, gh, &inf))) return done(rc);
  uint8_t dxy[64], bxy[64];
  memcpy(sc, rnd, 32); memcpy(sc + 32, rnd + 32, 32); memcpy(pts, gh, 64);
  if ((rc = sbn_msm(ctx, sc, pts, 2, 0, dxy, &inf))) return done(rc);
  const El dr = mul(ld(rnd), ld(rq));
  memcpy(sc, dr.v, 32); memcpy(sc + 32, rnd + 64, 32); memcpy(pts, Qb, 64);
  if ((rc = sbn_msm(ctx, sc, pts, 2, 0, bxy, &inf))) return done(rc);
  append_point(tr, "delta", dxy, proof + 64 * lg); append_point(tr, "beta", bxy, proof + 64 * lg + 32);
  uint8_t cc[32];
  sbn_transcript_challenge_scalar(tr, (const uint8_t*)"c", 1, cc);
  const El z1 = add(ld(rnd), mul(ld(cc), mul(ld(ah), ld(bh))));
  const El z2 = add(mul(ld(bh), add(mul(ld(cc), blind_G), ld(rnd + 64))), ld(rnd + 32));
  memcpy(proof + 64 * lg + 64, z1.v, 32); memcpy(proof + 64 * lg + 96, z2.v, 32);
  return done(SBN_OK);
}

extern "C" int sbn_bench_polyeval(sbn_ctx* ctx, int ell, int mode, int reps, double* out_us /* reps */, double* out_host_us /* reps x 3: sbn_prof_last_polyeval, mode 1 */, uint64_t* out_digest) {
  if (!ctx || ell < 2 || ell > 28 || reps < 1 || !out_us || !out_digest) return SBN_EINVAL;
  const size_t ml = (size_t)ell / 2, mr = (size_t)ell - ml, n = (size_t)1 << mr, N = (size_t)1 << ell, lg = mr;
  Setup S; int rc;
  S.xy.resize(64 * (n + 2));
  if ((rc = sbn_gens_new(ctx, n + 1, (const uint8_t*)"gens_polyeval_bench", 19, S.xy.data(), &S.gens))) return rc;
  if (!rc) rc = sbn_bases_split_at(ctx, S.gens, n, &S.Gn, &S.G1);
  if (!rc) rc = sbn_dev_alloc(ctx, N * 32, &S.mem);
  if (!rc) rc = sbn_scalars_synthetic(ctx, 0x90171e5a1ull, 0, N, S.mem);
  if (!rc) rc = sbn_table_from_dev(ctx, S.mem, N, 0, &S.Z);
  std::vector<uint8_t> r(32 * ell, 0), rnd(32 * (3 + 2 * lg), 0), proof(64 * lg + 128), proof0;
  for (int j = 0; j < ell; j++) { r[32 * j] = (uint8_t)(5 + j); r[32 * j + 13] = (uint8_t)(0x61 + j); r[32 * j + 27] = (uint8_t)(0x17 + 3 * j); }
  for (size_t j = 0; j < 3 + 2 * lg; j++) { rnd[32 * j] = (uint8_t)(9 + j); rnd[32 * j + 11] = (uint8_t)(0x33 + j); rnd[32 * j + 30] = (uint8_t)(1 + j); }
  uint8_t Zr[32];
  if (!rc) rc = sbn_table_evaluate(ctx, S.Z, r.data(), (size_t)ell, Zr);
  uint64_t digest = 0xcbf29ce484222325ull;
  for (int rep = -1; rep < reps && !rc; rep++) {             // rep -1: untimed — the sets derived from the fresh handles and their lookup tables are built there
    sbn_transcript* tr = nullptr; uint8_t Cx[64], Cy[64]; int xi = 0, yi = 0;
    if ((rc = sbn_transcript_new((const uint8_t*)"polyeval bench", 14, &tr))) break;
    const auto t0 = std::chrono::steady_clock::now();
    if (mode == 1) rc = sbn_polyeval_prove(ctx, S.gens, S.Z, nullptr, r.data(), (size_t)ell, Zr, nullptr, rnd.data(), tr, proof.data(), Cx, &xi, Cy, &yi);
    else rc = loop_opening(ctx, S, r.data(), (size_t)ell, Zr, rnd.data(), tr, proof.data(), Cx, Cy);
    const auto t1 = std::chrono::steady_clock::now();
    if (rep < 0) { sbn_transcript_free(tr); continue; }
    out_us[rep] = std::chrono::duration<double, std::micro>(t1 - t0).count();
    if (!rc && out_host_us) { if (mode == 1) sbn_prof_last_polyeval(ctx, out_host_us + 3 * rep); else memset(out_host_us + 3 * rep, 0, 24); }
    if (!rc && rep == 0) {
      uint8_t state[203]; sbn_transcript_state(tr, state);
      digest = fnv(fnv(fnv(fnv(digest, proof.data(), proof.size()), Cx, 64), Cy, 64), state, 203);
    }
    sbn_transcript_free(tr);
  }
  *out_digest = digest;
  if (S.Z) sbn_table_free(ctx, S.Z);
  if (S.mem) sbn_dev_free(ctx, S.mem);
  if (S.G1) sbn_bases_free(ctx, S.G1);
  if (S.Gn) sbn_bases_free(ctx, S.Gn);
  if (S.gens) sbn_bases_free(ctx, S.gens);
  return rc;
}
