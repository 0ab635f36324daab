// random_tape_host.hpp — the prover's RandomTape (reference src/random.rs:15-31) and the draw plans of the one-call provers, host only: no HIP, no
// context, no launches.  A tape is a Merlin transcript of its own: Transcript::new(name), append_scalar(b"init_randomness", init), and every draw is
// challenge_scalar(label) (transcript.rs:56-71).  A tape started from the same `init` gives the draws the reference's tape gives, so a Rust caller and a C
// caller with one seed make one proof.
// A draw plan fills `rnd` exactly as the matching prove call documents it (include/sbn254.h), with the reference's labels in the reference's order:
//   plan_zk_sumcheck   sumcheck.rs:483-484, :673-674 (blinds_poly, blinds_evals), then per round DotProductProof::prove's d_vec[n], r_delta, r_beta (nizk/mod.rs:326-328)
//   plan_polyeval      DotProductProofLog::prove (nizk/mod.rs:458-464): d, r_delta, r_beta, blinds_vec_1[lg], blinds_vec_2[lg].  TWO THINGS TO KEEP:
//                        * :460 draws r_beta under the label b"r_delta".  It is copied literally: another label gives another scalar;
//                        * blinds_vec_1 is drawn whole and then blinds_vec_2, but rnd stores them as (v1[i], v2[i]) pairs
//   plan_r1cs_proof    r1csproof.rs:225 (poly_blinds[L]), phase 1, :318-321, KnowledgeProof's t1, t2 (nizk/mod.rs:44-45), ProductProof's b1 .. b5 (:181-185),
//                      EqualityProof's r (:108), phase 2, blind_eval (r1csproof.rs:410), the opening, EqualityProof's r
//   plan_sparse_eval   the three openings of HashLayerProof::prove: derefs (absent in the KZG build), ops, mem
// Nothing here prints, logs or keeps `init` or a draw; wipe() clears the state through a volatile pointer before the memory is released.
// tests/random_tape_check.cpp builds this header alone, under ASan + UBSan.
#pragma once
#include "proof_host.hpp"

namespace sbn_host {
namespace tape {

static inline void secure_zero(void* p, size_t n) { volatile uint8_t* v = (volatile uint8_t*)p; for (size_t i = 0; i < n; i++) v[i] = 0; }

struct RandomTape {
  MerlinTranscript t;
  // RandomTape::new (random.rs:15-23) with the scalar the reference takes from OsRng given by the caller: 32 canonical bytes
  void init(const uint8_t* name, size_t name_len, const uint8_t init32[32]) {
    t.init(name, name_len);
    t.append_message((const uint8_t*)"init_randomness", 15, init32, 32);
  }
  // random_scalar / random_vector (random.rs:25-31): n x challenge_scalar(label), canonical bytes
  void draw(Label l, uint8_t* out, size_t n) {
    for (size_t i = 0; i < n; i++) {
      uint8_t b[64];
      t.challenge_bytes(l.p, l.n, b, 64);
      transcript_wide_reduce(b, out + 32 * i);
      secure_zero(b, sizeof b);
    }
  }
  void wipe() { secure_zero(this, sizeof *this); }
};

// ---- the counts, as the *_sizes calls of the C ABI give them ----
static inline size_t count_zk_sumcheck(size_t num_rounds, size_t n) { return num_rounds * (n + 4); }
static inline size_t count_polyeval(size_t lg) { return 3 + 2 * lg; }
static inline size_t count_r1cs_proof(size_t L, size_t nx, size_t ny, size_t lg) { return L + 8 * nx + 7 * ny + 2 * lg + 17; }
static inline size_t count_sparse_eval(size_t lg_derefs, size_t lg_ops, size_t lg_mem, bool kzg) {
  return kzg ? 6 + 2 * (lg_ops + lg_mem) : 9 + 2 * (lg_derefs + lg_ops + lg_mem);
}

// ---- the plans: each writes its count of scalars at `out` and returns the first byte behind them ----
static inline uint8_t* plan_zk_sumcheck(RandomTape& T, size_t num_rounds, size_t n, uint8_t* out) {
  T.draw("blinds_poly", out, num_rounds); out += 32 * num_rounds;                 // sumcheck.rs:483, :673
  T.draw("blinds_evals", out, num_rounds); out += 32 * num_rounds;                // :484, :674
  for (size_t j = 0; j < num_rounds; j++) {                                       // DotProductProof::prove, once a round
    T.draw("d_vec", out, n); out += 32 * n;                                       // nizk/mod.rs:326
    T.draw("r_delta", out, 1); out += 32;                                         // :327
    T.draw("r_beta", out, 1); out += 32;                                          // :328
  }
  return out;
}

// beta_label: "r_delta" is the reference's (nizk/mod.rs:460); anything else is for a test that pins the quirk
static inline uint8_t* plan_polyeval(RandomTape& T, size_t lg, uint8_t* out, const char* beta_label = "r_delta") {
  T.draw("d", out, 1);                                                            // nizk/mod.rs:458
  T.draw("r_delta", out + 32, 1);                                                 // :459
  T.draw(beta_label, out + 64, 1);                                                // :460: r_beta, drawn under b"r_delta"
  uint8_t* pairs = out + 96;
  for (size_t i = 0; i < lg; i++) T.draw("blinds_vec_1", pairs + 64 * i, 1);      // :463: the whole of v1 first ...
  for (size_t i = 0; i < lg; i++) T.draw("blinds_vec_2", pairs + 64 * i + 32, 1); // :464: ... then v2, stored as (v1[i], v2[i])
  return pairs + 64 * lg;
}

// nx = log2 num_cons, ny = log2(2 num_vars), (L, R) = 2^factored_lens(log2 num_vars), lg = log2 R
static inline uint8_t* plan_r1cs_proof(RandomTape& T, size_t L, size_t nx, size_t ny, size_t lg, uint8_t* out) {
  T.draw("poly_blinds", out, L); out += 32 * L;                                   // r1csproof.rs:225
  out = plan_zk_sumcheck(T, nx, 4, out);                                          // phase 1, :295
  T.draw("Az_blind", out, 1); T.draw("Bz_blind", out + 32, 1); T.draw("Cz_blind", out + 64, 1); T.draw("prod_Az_Bz_blind", out + 96, 1);      // :318-321
  out += 128;
  T.draw("t1", out, 1); T.draw("t2", out + 32, 1); out += 64;                     // KnowledgeProof::prove, nizk/mod.rs:44-45
  T.draw("b1", out, 1); T.draw("b2", out + 32, 1); T.draw("b3", out + 64, 1); T.draw("b4", out + 96, 1); T.draw("b5", out + 128, 1);      // ProductProof::prove, :181-185
  out += 160;
  T.draw("r", out, 1); out += 32;                                                 // EqualityProof::prove, :108
  out = plan_zk_sumcheck(T, ny, 3, out);                                          // phase 2, r1csproof.rs:394
  T.draw("blind_eval", out, 1); out += 32;                                        // :410
  out = plan_polyeval(T, lg, out);                                                // PolyEvalProof::prove, :413
  T.draw("r", out, 1); out += 32;                                                 // the second EqualityProof
  return out;
}

static inline uint8_t* plan_sparse_eval(RandomTape& T, size_t lg_derefs, size_t lg_ops, size_t lg_mem, bool kzg, uint8_t* out) {
  if (!kzg) out = plan_polyeval(T, lg_derefs, out);                               // DerefsEvalProof::prove; the KZG build draws nothing there
  out = plan_polyeval(T, lg_ops, out);
  return plan_polyeval(T, lg_mem, out);
}

}  // namespace tape
}  // namespace sbn_host
