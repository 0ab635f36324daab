// product_proof_bench.cpp — a compiled CALLER of the C ABI (plain g++, no HIP) that times ProductCircuitEvalProofBatched::prove
// (product_tree.rs:251-392) two ways over the same inputs and the same Merlin transcript:
//   mode 0: the layer loop over the entry points that existed before sbn_product_proof_prove — per layer sbn_table_halves,
//           sbn_transcript_challenge_scalar x n, the joint claim, sbn_sumcheck_begin_eq + sbn_sumcheck_prove + sbn_sumcheck_free, the claim
//           appends, challenge_r_layer, the folded claims.  It uses no newer symbol, so this file links against an older library too;
//   mode 1: sbn_product_proof_prove (looked up at run time: an older library does not have it), one call.
// Both must end with the same bytes (the digest returned).  tools/bench_product_proof.py drives it.
#include "../../include/sbn254.h"
#include <chrono>
#include <cstdint>
#include <cstring>
#include <dlfcn.h>
#include <vector>

static const uint8_t R_LE[32] = {0x01, 0x00, 0x00, 0xf0, 0x93, 0xf5, 0xe1, 0x43, 0x91, 0x70, 0xb9, 0x79, 0x48, 0xe8, 0x33, 0x28,
                                 0x5d, 0x58, 0x81, 0x81, 0xb6, 0x45, 0x50, 0xb8, 0x29, 0xa0, 0x31, 0xe1, 0x72, 0x4e, 0x64, 0x30};
static bool geq_r(const uint8_t a[32]) { for (int i = 31; i >= 0; i--) if (a[i] != R_LE[i]) return a[i] > R_LE[i]; return true; }
// a + b, a - b mod r on canonical little-endian scalars
static void fr_add(const uint8_t a[32], const uint8_t b[32], uint8_t out[32]) {
  uint8_t t[32]; int c = 0;
  for (int i = 0; i < 32; i++) { int s = a[i] + b[i] + c; t[i] = (uint8_t)s; c = s >> 8; }      // < 2 r < 2^255: no carry out
  if (geq_r(t)) { int borrow = 0; for (int i = 0; i < 32; i++) { int d = (int)t[i] - R_LE[i] - borrow; borrow = d < 0; t[i] = (uint8_t)(d + (borrow << 8)); } }
  memcpy(out, t, 32);
}
static void fr_sub(const uint8_t a[32], const uint8_t b[32], uint8_t out[32]) {
  int borrow = 0; uint8_t t[32];
  for (int i = 0; i < 32; i++) { int d = (int)a[i] - b[i] - borrow; borrow = d < 0; t[i] = (uint8_t)(d + (borrow << 8)); }
  if (borrow) { int c = 0; for (int i = 0; i < 32; i++) { int s = t[i] + R_LE[i] + c; t[i] = (uint8_t)s; c = s >> 8; } }
  memcpy(out, t, 32);
}
// a + b x through the library's polynomial evaluation (the caller has no field multiplication of its own)
static int fr_lin(const uint8_t a[32], const uint8_t b[32], const uint8_t x[32], uint8_t out[32]) {
  uint8_t co[64]; memcpy(co, a, 32); memcpy(co + 32, b, 32);
  return sbn_unipoly_eval(co, 2, x, out);
}
static uint64_t fnv(uint64_t h, const uint8_t* p, size_t n) { for (size_t i = 0; i < n; i++) { h ^= p[i]; h *= 0x100000001b3ull; } return h; }

typedef int (*pp_fn)(sbn_ctx*, const sbn_table* const*, size_t, size_t, const sbn_table* const*, const sbn_table* const*, const sbn_table* const*, size_t,
                     sbn_transcript*, uint8_t*, uint8_t*, uint8_t*, uint8_t*);

struct Job {
  sbn_ctx* ctx; size_t n, L, nd;
  std::vector<sbn_table*> layers;                 // [i * L + j]
  std::vector<sbn_table*> dl, dr, dw;
};

static int loop_prove(Job& J, sbn_transcript* tr, uint8_t* polys, uint8_t* claims, uint8_t* rand_out, uint8_t* cfinal) {
  const size_t n = J.n, L = J.L, nd = J.nd;
  sbn_ctx* ctx = J.ctx;
  int rc = SBN_OK;
  const uint8_t zero[32] = {0};
  std::vector<uint8_t> ctv(32 * (n + nd)), rand(32 * L), rnext(32 * L), fin(32 * (2 * n + 1 + 3 * nd)), co(32 * (n + nd));
  std::vector<sbn_table*> Lh(n), Rh(n);
  auto halves = [&](size_t layer) { for (size_t i = 0; i < n && !rc; i++) rc = sbn_table_halves(ctx, J.layers[i * L + layer], &Lh[i], &Rh[i]); };
  auto drop = [&]() { for (size_t i = 0; i < n; i++) { if (Lh[i]) sbn_table_free(ctx, Lh[i]); if (Rh[i]) sbn_table_free(ctx, Rh[i]); Lh[i] = Rh[i] = nullptr; } };
  // ProductCircuit::evaluate of every circuit (:262-264)
  {
    std::vector<uint8_t> a(32 * n), b(32 * n);
    halves(L - 1);
    if (!rc) rc = sbn_table_read0_many(ctx, Lh.data(), n, a.data());
    if (!rc) rc = sbn_table_read0_many(ctx, Rh.data(), n, b.data());
    for (size_t i = 0; i < n && !rc; i++) rc = fr_lin(zero, a.data() + 32 * i, b.data() + 32 * i, ctv.data() + 32 * i);
    drop();
  }
  size_t poly_off = 0, nrand = 0;
  uint8_t* cl = claims;
  for (size_t s = 0; s < L && !rc; s++) {
    const size_t layer = L - 1 - s, rounds = s, nseq = layer == 0 ? nd : 0, ninst = n + nseq;
    if (nseq) {                                   // DotProductCircuit::evaluate (:296-299): sum left * right * weight = <left * right, weight>
      for (size_t k = 0; k < nd && !rc; k++) {
        // left and right are the halves of one table (see the set-up): its product layer is left * right
        sbn_table* lr = nullptr;
        if ((rc = sbn_product_layer(ctx, J.dl[k + nd], &lr))) break;           // (dl[nd + k] holds the joined table)
        rc = sbn_table_dot(ctx, lr, J.dw[k], ctv.data() + 32 * (n + k));
        sbn_table_free(ctx, lr);
      }
    }
    for (size_t i = 0; i < ninst && !rc; i++) rc = sbn_transcript_challenge_scalar(tr, (const uint8_t*)"rand_coeffs_next_layer", 22, co.data() + 32 * i);
    uint8_t claim[32] = {0};
    for (size_t i = 0; i < ninst && !rc; i++) { uint8_t t[32]; rc = fr_lin(zero, ctv.data() + 32 * i, co.data() + 32 * i, t); fr_add(claim, t, claim); }
    halves(layer);
    if (rc) { drop(); break; }
    if (rounds == 0) {
      rc = sbn_table_read0_many(ctx, Lh.data(), n, fin.data());
      if (!rc) rc = sbn_table_read0_many(ctx, Rh.data(), n, fin.data() + 32 * n);
      if (!rc && nseq) rc = sbn_table_read0_many(ctx, J.dl.data(), nd, fin.data() + 32 * (2 * n + 1));
      if (!rc && nseq) rc = sbn_table_read0_many(ctx, J.dr.data(), nd, fin.data() + 32 * (2 * n + 1 + nd));
      if (!rc && nseq) rc = sbn_table_read0_many(ctx, J.dw.data(), nd, fin.data() + 32 * (2 * n + 1 + 2 * nd));
    } else {
      sbn_sumcheck* st = nullptr; uint8_t ev[96];
      rc = sbn_sumcheck_begin_eq(ctx, Lh.data(), Rh.data(), n, rand.data(), rounds, J.dl.data(), J.dr.data(), J.dw.data(), nseq, co.data(), ev, &st);
      if (!rc) rc = sbn_sumcheck_prove(ctx, st, tr, claim, polys + 128 * poly_off, rnext.data() + 32, fin.data());
      if (st) sbn_sumcheck_free(ctx, st);
      poly_off += rounds;
    }
    drop();
    if (rc) break;
    for (size_t i = 0; i < n; i++) {
      sbn_transcript_append_message(tr, (const uint8_t*)"claim_prod_left", 15, fin.data() + 32 * i, 32);
      sbn_transcript_append_message(tr, (const uint8_t*)"claim_prod_right", 16, fin.data() + 32 * (n + i), 32);
    }
    memcpy(cl, fin.data(), 64 * n); cl += 64 * n;
    if (nseq) {
      const uint8_t* d = fin.data() + 32 * (2 * n + 1);
      for (size_t k = 0; k < nd; k++) {
        sbn_transcript_append_message(tr, (const uint8_t*)"claim_dotp_left", 15, d + 32 * k, 32);
        sbn_transcript_append_message(tr, (const uint8_t*)"claim_dotp_right", 16, d + 32 * (nd + k), 32);
        sbn_transcript_append_message(tr, (const uint8_t*)"claim_dotp_weight", 17, d + 32 * (2 * nd + k), 32);
      }
      memcpy(cl, d, 96 * nd); cl += 96 * nd;
    }
    rc = sbn_transcript_challenge_scalar(tr, (const uint8_t*)"challenge_r_layer", 17, rnext.data());
    for (size_t i = 0; i < n && !rc; i++) {
      uint8_t diff[32]; fr_sub(fin.data() + 32 * (n + i), fin.data() + 32 * i, diff);
      rc = fr_lin(fin.data() + 32 * i, diff, rnext.data(), ctv.data() + 32 * i);
    }
    nrand = rounds + 1;
    memcpy(rand.data(), rnext.data(), 32 * nrand);
  }
  if (!rc) { memcpy(rand_out, rand.data(), 32 * nrand); memcpy(cfinal, ctv.data(), 32 * n); }
  return rc;
}

extern "C" int sbn_bench_product_proof(sbn_ctx* ctx, int n_circ, int n_dotp, int n_layers, int mode, int reps, double* out_us, uint64_t* out_digest) {
  if (!ctx || n_circ < 1 || n_dotp < 0 || n_circ + n_dotp > 24 || n_layers < 1 || n_layers > 24 || reps < 1 || !out_us || !out_digest) return SBN_EINVAL;
  pp_fn one_call = nullptr;
  if (mode == 1 && !(one_call = (pp_fn)dlsym(RTLD_DEFAULT, "sbn_product_proof_prove"))) return SBN_EINVAL;
  Job J; J.ctx = ctx; J.n = (size_t)n_circ; J.L = (size_t)n_layers; J.nd = (size_t)n_dotp;
  const size_t n = J.n, L = J.L, nd = J.nd, N = (size_t)1 << L, h = N / 2;
  std::vector<void*> mem; std::vector<sbn_table*> owned;
  int rc = SBN_OK;
  auto synth = [&](size_t len, uint64_t seed, sbn_table** out) {
    void* p = nullptr;
    if ((rc = sbn_dev_alloc(ctx, len * 32, &p))) return;
    mem.push_back(p);
    if ((rc = sbn_scalars_synthetic(ctx, 0x9c0de0000ull + seed, 0, len, p))) return;
    if ((rc = sbn_table_from_dev(ctx, p, len, 0, out))) return;
    owned.push_back(*out);
  };
  // the circuits: inputs of 2^L uniform scalars, layers from sbn_product_circuit_many (the last, one-entry table is the product, not a layer)
  std::vector<sbn_table*> ins(n, nullptr), pcs(n * (L + 1), nullptr);
  for (size_t i = 0; i < n && !rc; i++) synth(N, i, &ins[i]);
  size_t cnt = 0;
  if (!rc) rc = sbn_product_circuit_many(ctx, ins.data(), n, pcs.data(), L + 1, &cnt);
  for (sbn_table* t : pcs) if (t) owned.push_back(t);
  if (!rc && cnt != L) rc = SBN_EINVAL;
  J.layers.assign(n * L, nullptr);
  for (size_t i = 0; i < n && !rc; i++) { J.layers[i * L] = ins[i]; for (size_t j = 1; j < L; j++) J.layers[i * L + j] = pcs[i * (L + 1) + j - 1]; }
  // the dot-product circuits: left and right are the halves of ONE table of 2^L entries (so that the loop can form left * right with
  // sbn_product_layer); dl[nd + k] keeps the joined table
  J.dl.assign(2 * nd, nullptr); J.dr.assign(nd, nullptr); J.dw.assign(nd, nullptr);
  for (size_t k = 0; k < nd && !rc; k++) {
    synth(N, 100 + k, &J.dl[nd + k]);
    if (!rc) rc = sbn_table_halves(ctx, J.dl[nd + k], &J.dl[k], &J.dr[k]);
    if (!rc) { owned.push_back(J.dl[k]); owned.push_back(J.dr[k]); }
    if (!rc) synth(h, 200 + k, &J.dw[k]);
  }
  const size_t npoly = L * (L - 1) / 2;
  std::vector<uint8_t> polys(128 * (npoly ? npoly : 1)), claims(32 * (2 * n * L + 3 * nd)), rand(32 * L), cfinal(32 * n);
  uint64_t digest = 0xcbf29ce484222325ull;
  for (int rep = 0; rep < reps && !rc; rep++) {
    sbn_transcript* tr = nullptr;
    if ((rc = sbn_transcript_new((const uint8_t*)"product proof bench", 19, &tr))) break;
    if ((rc = sbn_ctx_sync(ctx))) { sbn_transcript_free(tr); break; }
    const auto t0 = std::chrono::steady_clock::now();
    if (mode == 1) rc = one_call(ctx, J.layers.data(), n, L, J.dl.data(), J.dr.data(), J.dw.data(), nd, tr, polys.data(), claims.data(), rand.data(), cfinal.data());
    else rc = loop_prove(J, tr, polys.data(), claims.data(), rand.data(), cfinal.data());
    const auto t1 = std::chrono::steady_clock::now();
    out_us[rep] = std::chrono::duration<double, std::micro>(t1 - t0).count();
    if (!rc && rep == 0) {
      uint8_t state[203]; sbn_transcript_state(tr, state);
      digest = fnv(fnv(fnv(fnv(fnv(digest, polys.data(), 128 * npoly), claims.data(), claims.size()), rand.data(), rand.size()), cfinal.data(), cfinal.size()), state, 203);
    }
    sbn_transcript_free(tr);
  }
  *out_digest = digest;
  for (size_t i = owned.size(); i-- > 0;) sbn_table_free(ctx, owned[i]);
  for (void* p : mem) sbn_dev_free(ctx, p);
  return rc;
}
