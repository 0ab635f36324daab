// verify_host.hpp — the host arithmetic a verdict of the one-call verifiers rests on, host only: no HIP, no context, no launches; built on
// proof_host.hpp (Script, fr::) and includable alone, like it.  tests/verify_host_check.cpp builds this header alone, under ASan + UBSan, and
// tests/test_verify_host_cpu.py compares it with tests/polyeval_verify_model.py, tests/polyeval_model.py, tests/transcript_model.py and plain integers.
//   g1_xy_valid, g1_compressed_normalise, g1_is_identity, g1_neg_bytes, fr_neg_bytes, fq_to_dev_mont     points and scalars as bytes
//   OpeningShape / opening_shape      the split of an opening's ell variables: the only place that derives it
//   polyeval_host_eq, joint_reduce    EqPolynomial::evals and the n-to-1 reduction in front of a joint opening (the provers call them too)
//   polyeval_verify_script, polyeval_verify_scalars      the transcript lines and the O(lg n) field work of every Hyrax opening check
// The device half of the same vocabulary is abi_verify_common.inc.
#pragma once
#include "proof_host.hpp"
#include <vector>

namespace sbn_host {

// canonical affine x || y on the curve y^2 = x^3 + 3, or the all-zero identity
static inline bool g1_xy_valid(const uint8_t xy[64]) {
  bool inf = true; for (int k = 0; k < 64; k++) if (xy[k]) { inf = false; break; }
  if (inf) return true;
  sbn_host::Fq x, y; memcpy(x.v, xy, 32); memcpy(y.v, xy + 32, 32);
  if (sbn_host::geq_p(x.v) || sbn_host::geq_p(y.v)) return false;
  const sbn_host::Fq three = {{3, 0, 0, 0}};
  const sbn_host::Fq xm = sbn_host::to_mont(x), ym = sbn_host::to_mont(y);
  const sbn_host::Fq rhs = sbn_host::add(sbn_host::mul(sbn_host::sqr(xm), xm), sbn_host::to_mont(three)), lhs = sbn_host::sqr(ym);
  return memcmp(lhs.v, rhs.v, 32) == 0;
}
// a compressed point as the reference's deserialisation and serialisation leave it: the identity in the form sbn_g1_compress writes
static inline void g1_compressed_normalise(const uint8_t in[32], uint8_t out[32]) {
  memcpy(out, in, 32);
  if (out[31] & 0x40) { memset(out, 0, 32); out[31] = 0x40; }
}
static inline void fr_neg_bytes(const uint8_t in[32], uint8_t out[32]) {
  sbn_host::fr::El x; memcpy(x.v, in, 32);
  const sbn_host::fr::El z = sbn_host::fr::sub(sbn_host::fr::from_u64(0), x);
  memcpy(out, z.v, 32);
}
// -P of a canonical affine point (the identity, 64 zero bytes, stays)
static inline void g1_neg_bytes(const uint8_t in[64], uint8_t out[64]) {
  memcpy(out, in, 64);
  sbn_host::Fq y; memcpy(y.v, in + 32, 32);
  if (sbn_host::is_zero(y)) return;
  uint64_t br = 0, r[4];
  for (int i = 0; i < 4; i++) { sbn_host::u128 d = (sbn_host::u128)sbn_host::QP[i] - y.v[i] - br; r[i] = (uint64_t)d; br = (uint64_t)(d >> 127); }
  memcpy(out + 32, r, 32);
}
static inline bool g1_is_identity(const uint8_t xy[64]) { for (int k = 0; k < 64; k++) if (xy[k]) return false; return true; }
// a canonical coordinate in the device's Montgomery form (R = 2^261), canonical again: a generator table's entry (k_points_to_mont)
static inline sbn_host::Fq fq_to_dev_mont(const uint8_t b[32]) {
  sbn_host::Fq x; memcpy(x.v, b, 32);
  const sbn_host::Fq k32 = {{32, 0, 0, 0}};
  return sbn_host::mul(sbn_host::to_mont(x), sbn_host::to_mont(k32));
}

// how an opening splits its ell variables (hyrax.rs:371-373): L_size = 2^ml rows of n = 2^mr columns, lg = mr bullet rounds, and the np points of
// its proof (L, R, delta, beta)
struct OpeningShape { size_t ell, ml, mr, L_size, n, lg, np; };
static inline OpeningShape opening_shape(size_t ell) {
  OpeningShape s;
  s.ell = ell; s.ml = ell / 2; s.mr = ell - s.ml; s.L_size = (size_t)1 << s.ml; s.n = (size_t)1 << s.mr; s.lg = s.mr; s.np = 2 * s.lg + 2;
  return s;
}

// EqPolynomial::evals (hyrax.rs:355-369) on the host, canonical bytes out: the values stay plain integers, the point is in Montgomery form
// (mmul(s, r R) = s r), so a level costs one product per new pair
static inline void polyeval_host_eq(const uint8_t* r, size_t m, std::vector<uint8_t>& out) {
  using namespace sbn_host::fr;
  const size_t N = (size_t)1 << m;
  std::vector<El> e(N);
  e[0] = from_u64(1);
  size_t size = 1;
  for (size_t j = 0; j < m; j++) {
    const El rj = to_m(el_from(r + 32 * j));
    for (size_t k = size; k-- > 0;) { const El s = e[k]; const El hi = mmul(s, rj); e[2 * k + 1] = hi; e[2 * k] = sub(s, hi); }
    size *= 2;
  }
  out.resize(32 * N);
  for (size_t i = 0; i < N; i++) memcpy(&out[32 * i], e[i].v, 32);
}
// the reduction both builds' joint openings start with (sparse_mlpoly_full.rs:384-397, :514-535): the evals under `label_evals`, lc challenges, the fold
// of the evals from the last challenge down, the joint claim under `label_claim`.  rj: the lc challenges, then r; claim: canonical
static inline void joint_reduce(const uint8_t* evals, size_t count, size_t lc, sbn_host::Label label_evals, sbn_host::Label label_chal, sbn_host::Label label_claim,
                                const uint8_t* r, size_t ell_r, sbn_host::MerlinTranscript& t, std::vector<uint8_t>& rj, uint8_t claim[32]) {
  using namespace sbn_host::fr;
  const size_t ell = lc + ell_r;
  sbn_host::Script ts{t};
  ts.scalars(label_evals, evals, count);                           // sparse_mlpoly_full.rs:384
  rj.assign(32 * ell, 0);
  ts.challenges(label_chal, rj.data(), lc);                        // :387
  if (ell_r) memcpy(&rj[32 * lc], r, 32 * ell_r);
  std::vector<El> pe(count);
  for (size_t i = 0; i < count; i++) pe[i] = el_from(evals + 32 * i);
  size_t len = count;
  for (size_t j = lc; j-- > 0;) {                                  // bound_poly_var_bot from the last challenge down (:389-391, hyrax.rs:206-214)
    const El cj = to_m(el_from(&rj[32 * j]));
    len /= 2;
    for (size_t i = 0; i < len; i++) pe[i] = add(pe[2 * i], mmul(cj, sub(pe[2 * i + 1], pe[2 * i])));
  }
  memcpy(claim, pe[0].v, 32);
  ts.scalar(label_claim, claim);                                   // :397
}

// the transcript lines of PolyEvalProof::verify_plain / verify with DotProductProofLog::verify and BulletReductionProof::verify inside (hyrax.rs:127,
// nizk/mod.rs:538-556, bullet.rs:147-153), as every opening check writes them.  Cxy: Cx ‖ Cy; Rv: a_vec = R, n scalars; comp: the proof's 2 lg + 2
// normalised points.  Out: the challenges r and c, u and their inverses.  false: a challenge u = 0 has no inverse (bullet.rs:161-165)
static inline bool polyeval_verify_script(sbn_host::Script& ts, const uint8_t Cxy[128], const uint8_t* Rv, size_t n, const uint8_t* comp, size_t lg,
                                          uint8_t rq[32], uint8_t cc[32], std::vector<sbn_host::fr::El>& u, std::vector<sbn_host::fr::El>& ui) {
  using namespace sbn_host::fr;
  uint8_t c32[32];
  ts.protocol("polynomial evaluation proof");                     // hyrax.rs:127
  ts.protocol("dot product proof (log)");                         // nizk/mod.rs:538
  ts.point_xy("Cx", Cxy, c32);                                    // :543-545
  ts.point_xy("Cy", Cxy + 64, c32);
  ts.scalars("a", Rv, n);
  ts.challenge("r", rq);                                          // :548
  u.assign(lg, from_u64(0)); ui.assign(lg, from_u64(0));
  for (size_t j = 0; j < lg; j++) {                               // bullet.rs:147-153
    ts.point("L", comp + 32 * j);
    ts.point("R", comp + 32 * (lg + j));
    uint8_t ub[32];
    ts.challenge("u", ub);
    u[j] = el_from(ub);
    if (is_zero(u[j])) return false;                              // no inverse (bullet.rs:161-165)
    ui[j] = inv(u[j]);
  }
  ts.point("delta", comp + 64 * lg);                              // nizk/mod.rs:555-556
  ts.point("beta", comp + 64 * lg + 32);
  ts.challenge("c", cc);
  return true;
}
// b_hat = <s, R> in closed form over the right-hand coordinates r_right, the scalars of the final equation's 2 lg + 4 points (L, R, delta, beta, Cx,
// Cy) into hs, and the constants of the row -z1 s ‖ -z1 a r with blind -z2
struct PolyevalFinal { sbn_host::fr::El a_hat, nz1, nz2, tail; };
static inline PolyevalFinal polyeval_verify_scalars(const uint8_t* r_right, size_t lg, const std::vector<sbn_host::fr::El>& u, const std::vector<sbn_host::fr::El>& ui,
                                                    const uint8_t rq[32], const uint8_t cc[32], const uint8_t* z1b, const uint8_t* z2b, uint8_t* hs) {
  using namespace sbn_host::fr;
  const El one = from_u64(1), zero = from_u64(0);
  El a_hat = one;
  for (size_t k = 0; k < lg; k++) {
    const El rk = el_from(r_right + 32 * k);
    a_hat = fmul(a_hat, add(fmul(ui[k], sub(one, rk)), fmul(u[k], rk)));
  }
  const El ec = el_from(cc), er = el_from(rq), ac = fmul(a_hat, ec), z1 = el_from(z1b), z2 = el_from(z2b);
  for (size_t j = 0; j < lg; j++) {
    const El sl = fmul(ac, fmul(u[j], u[j])), sr = fmul(ac, fmul(ui[j], ui[j]));
    memcpy(hs + 32 * j, sl.v, 32); memcpy(hs + 32 * (lg + j), sr.v, 32);
  }
  memcpy(hs + 64 * lg, one.v, 32); memcpy(hs + 64 * lg + 32, a_hat.v, 32);               // delta, beta
  { const El sy = fmul(ac, er); memcpy(hs + 64 * lg + 64, ac.v, 32); memcpy(hs + 64 * lg + 96, sy.v, 32); }   // Cx, Cy
  PolyevalFinal f; f.a_hat = a_hat; f.nz1 = sub(zero, z1); f.nz2 = sub(zero, z2); f.tail = fmul(f.nz1, fmul(a_hat, er));
  return f;
}

}  // namespace sbn_host
