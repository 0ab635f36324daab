// sumcheck_prove_bench.cpp — a compiled CALLER of the C ABI (plain g++, no HIP) that times one batched cubic sumcheck two ways:
//   mode 0: the round-by-round loop (sbn_sumcheck_round per round; UniPoly::from_evals, the Merlin transcript and poly(r_j) on the host
//           between the calls, as the Rust shim's prove_cubic_batched does), one host round trip per round;
//   mode 1: sbn_sumcheck_prove, every round queued at once with the transcript step on the device, one wait.
// Both start from sbn_sumcheck_begin on the same tables and the same transcript state, and must end with the same bytes
// (the digest returned).  tools/bench_sumcheck_prove.py drives it; a Python loop would add ~40 us per round and is no baseline.
#include "../../include/sbn254.h"
#include <chrono>
#include <cstdint>
#include <cstring>
#include <vector>

static const uint8_t R_LE[32] = {0x01, 0x00, 0x00, 0xf0, 0x93, 0xf5, 0xe1, 0x43, 0x91, 0x70, 0xb9, 0x79, 0x48, 0xe8, 0x33, 0x28,
                                 0x5d, 0x58, 0x81, 0x81, 0xb6, 0x45, 0x50, 0xb8, 0x29, 0xa0, 0x31, 0xe1, 0x72, 0x4e, 0x64, 0x30};
// a - b mod r on canonical little-endian scalars
static void fr_sub(const uint8_t a[32], const uint8_t b[32], uint8_t out[32]) {
  int borrow = 0; uint8_t t[32];
  for (int i = 0; i < 32; i++) { int d = (int)a[i] - b[i] - borrow; borrow = d < 0; t[i] = (uint8_t)(d + (borrow << 8)); }
  if (borrow) { int c = 0; for (int i = 0; i < 32; i++) { int s = t[i] + R_LE[i] + c; t[i] = (uint8_t)s; c = s >> 8; } }
  memcpy(out, t, 32);
}
static uint64_t fnv(uint64_t h, const uint8_t* p, size_t n) { for (size_t i = 0; i < n; i++) { h ^= p[i]; h *= 0x100000001b3ull; } return h; }

extern "C" int sbn_bench_sumcheck_prove(sbn_ctx* ctx, int n_par, int n_seq, int logn, int mode, int reps, double* out_us /* reps: begin excluded */,
                                        double* out_begin_us /* reps */, uint64_t* out_digest) {
  if (!ctx || n_par < 0 || n_seq < 0 || n_par + n_seq < 1 || n_par + n_seq > 24 || logn < 1 || logn > 24 || reps < 1 || !out_us || !out_digest) return SBN_EINVAL;
  const size_t n = (size_t)1 << logn, ntab = 2 * n_par + (n_par ? 1 : 0) + 3 * n_seq;
  std::vector<void*> mem(ntab, nullptr); std::vector<sbn_table*> tab(ntab, nullptr);
  int rc = SBN_OK;
  for (size_t t = 0; t < ntab && !rc; t++) {
    if ((rc = sbn_dev_alloc(ctx, n * 32, &mem[t]))) break;
    if ((rc = sbn_scalars_synthetic(ctx, 0xbe9c40000ull + t, 0, n, mem[t]))) break;
    rc = sbn_table_from_dev(ctx, mem[t], n, 0, &tab[t]);
  }
  std::vector<uint8_t> co(32 * (n_par + n_seq), 0), claim(32, 0), polys(128 * logn), rs(32 * logn), fin(32 * ntab);
  for (int i = 0; i < n_par + n_seq; i++) { co[32 * i] = (uint8_t)(3 + i); co[32 * i + 9] = (uint8_t)(0x51 + i); }
  claim[0] = 7; claim[20] = 0x33;
  const size_t o = 2 * n_par + (n_par ? 1 : 0);
  const sbn_table* const* Ap = tab.data(); const sbn_table* const* Bp = tab.data() + n_par; const sbn_table* Cp = n_par ? tab[2 * n_par] : nullptr;
  const sbn_table* const* As = tab.data() + o; const sbn_table* const* Bs = As + n_seq; const sbn_table* const* Cs = Bs + n_seq;
  uint64_t digest = 0xcbf29ce484222325ull;
  for (int rep = 0; rep < reps && !rc; rep++) {
    sbn_transcript* tr = nullptr; sbn_sumcheck* st = nullptr; uint8_t ev[96];
    if ((rc = sbn_transcript_new((const uint8_t*)"sumcheck bench", 14, &tr))) break;
    const auto t0 = std::chrono::steady_clock::now();
    rc = sbn_sumcheck_begin(ctx, Ap, Bp, Cp, (size_t)n_par, As, Bs, Cs, (size_t)n_seq, co.data(), ev, &st);
    const auto t1 = std::chrono::steady_clock::now();
    if (!rc && mode == 1) rc = sbn_sumcheck_prove(ctx, st, tr, claim.data(), polys.data(), rs.data(), fin.data());
    else if (!rc) {
      uint8_t e[32]; memcpy(e, claim.data(), 32);
      for (int j = 0; j < logn && !rc; j++) {
        uint8_t evals[128], *cj = polys.data() + 128 * j, *rj = rs.data() + 32 * j;
        memcpy(evals, ev, 32); fr_sub(e, ev, evals + 32); memcpy(evals + 64, ev + 32, 64);
        if ((rc = sbn_unipoly_from_evals(evals, 4, cj))) break;
        sbn_transcript_append_message(tr, (const uint8_t*)"poly", 4, (const uint8_t*)"UniPoly_begin", 13);
        for (int k = 0; k < 4; k++) sbn_transcript_append_message(tr, (const uint8_t*)"coeff", 5, cj + 32 * k, 32);
        sbn_transcript_append_message(tr, (const uint8_t*)"poly", 4, (const uint8_t*)"UniPoly_end", 11);
        sbn_transcript_challenge_scalar(tr, (const uint8_t*)"challenge_nextround", 19, rj);
        if ((rc = sbn_sumcheck_round(ctx, st, rj, ev))) break;
        rc = sbn_unipoly_eval(cj, 4, rj, e);
      }
      if (!rc) rc = sbn_sumcheck_finish(ctx, st, fin.data());
    }
    const auto t2 = std::chrono::steady_clock::now();
    out_us[rep] = std::chrono::duration<double, std::micro>(t2 - t1).count();
    if (out_begin_us) out_begin_us[rep] = std::chrono::duration<double, std::micro>(t1 - t0).count();
    if (!rc && rep == 0) {
      uint8_t state[203]; sbn_transcript_state(tr, state);
      digest = fnv(fnv(fnv(fnv(digest, polys.data(), polys.size()), rs.data(), rs.size()), fin.data(), fin.size()), state, 203);
    }
    if (st) sbn_sumcheck_free(ctx, st);
    sbn_transcript_free(tr);
  }
  *out_digest = digest;
  for (size_t t = 0; t < ntab; t++) { if (tab[t]) sbn_table_free(ctx, tab[t]); if (mem[t]) sbn_dev_free(ctx, mem[t]); }
  return rc;
}
