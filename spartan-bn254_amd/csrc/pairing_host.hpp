// pairing_host.hpp — the host half of the BN254 optimal-ate pairing: a FIXED G2 point made ready for k_pairing_products (pairing_kernels.cuh).
// Host only: no HIP, no context, no launches; built on host_field.hpp and includable alone.  tests/pairing_host_check.cpp builds this header alone
// and tests/test_pairing_host_cpu.py compares its tables byte for byte with the literal model of tests/pairing_model.py.  abi_pairing.inc
// (sbn_g2_prepare) is its caller in the library.  Stands in for what the reference gets from ark-bn254's G2Prepared inside Bn254::pairing
// (kzg.rs:212-214): the point is parsed, checked and its line coefficients are computed ONCE per SRS, never on a proof's path.
//   Fq2 = Fq[u]/(u^2 + 1), xi = 9 + u;  E': y^2 = x^3 + 3/xi (D-type twist), untwist (x, y) -> (x w^2, y w^3), w^6 = xi
//   g2_parse            128 bytes x.c0 | x.c1 | y.c0 | y.c1 (canonical little-endian integers, or ark-ff Montgomery limbs), canonical / identity / on E'
//   g2_in_subgroup      the literal [r]Q == O: #E'(Fq2) = r (2q - r), so a point of E' need not be in G2 (254 affine doublings, once per point)
//   naf_schedule        the signed digits of 6u + 2, most significant first: 66 digits, 22 of them set
//   line_table          one line per doubling and per addition of the loop over the schedule, then the two Frobenius lines (pi(Q), -pi^2(Q)): 88 lines
// G2 arithmetic is AFFINE with slopes by inversion (a 3 us binary-Euclid inversion, ~90 of them): a line through T with slope lam is
//     l(P) = yP - lam xP w + (lam xT - yT) w^3
// and the table keeps (-lam, lam xT - yT).  That normal form has two Fq2 values a line where a projective step emits three, and it does not depend
// on how the point is represented: the model's table and this one are the same bytes.
#pragma once
#include "host_field.hpp"
#include <vector>

namespace sbn_host {
namespace pairing {

#include "pairing_consts.inc"

struct Fq2 { Fq c0, c1; };
static inline Fq neg(const Fq& a) { return sub(zero(), a); }
static inline Fq2 f2_add(const Fq2& a, const Fq2& b) { return {add(a.c0, b.c0), add(a.c1, b.c1)}; }
static inline Fq2 f2_sub(const Fq2& a, const Fq2& b) { return {sub(a.c0, b.c0), sub(a.c1, b.c1)}; }
static inline Fq2 f2_neg(const Fq2& a) { return {neg(a.c0), neg(a.c1)}; }
static inline Fq2 f2_conj(const Fq2& a) { return {a.c0, neg(a.c1)}; }
static inline Fq2 f2_dbl(const Fq2& a) { return f2_add(a, a); }
static inline bool f2_is_zero(const Fq2& a) { return is_zero(a.c0) && is_zero(a.c1); }
static inline bool f2_eq(const Fq2& a, const Fq2& b) { return eq(a.c0, b.c0) && eq(a.c1, b.c1); }
static inline Fq2 f2_mul(const Fq2& a, const Fq2& b) {                       // Karatsuba: three products
  const Fq t0 = mul(a.c0, b.c0), t1 = mul(a.c1, b.c1), t2 = mul(add(a.c0, a.c1), add(b.c0, b.c1));
  return {sub(t0, t1), sub(sub(t2, t0), t1)};
}
static inline Fq2 f2_sqr(const Fq2& a) { return {mul(add(a.c0, a.c1), sub(a.c0, a.c1)), dbl(mul(a.c0, a.c1))}; }
static inline Fq2 f2_inv(const Fq2& a) {                                     // conj(a) / (c0^2 + c1^2); 0 -> 0
  const Fq n = inv(add(sqr(a.c0), sqr(a.c1)));
  return {mul(a.c0, n), neg(mul(a.c1, n))};
}
static inline Fq2 f2_const(const uint64_t k[2][4]) { Fq2 r; memcpy(r.c0.v, k[0], 32); memcpy(r.c1.v, k[1], 32); return r; }
static inline Fq2 b_twist() { static const uint64_t k[2][4] = SBN_PAIRING_B_TWIST; return f2_const(k); }
static inline Fq2 gamma_x() { static const uint64_t k[2][4] = SBN_PAIRING_GAMMA_X; return f2_const(k); }
static inline Fq2 gamma_y() { static const uint64_t k[2][4] = SBN_PAIRING_GAMMA_Y; return f2_const(k); }

struct G2 { Fq2 x, y; bool inf; };
static inline G2 g2_inf() { G2 r; r.x = r.y = {zero(), zero()}; r.inf = true; return r; }
static inline G2 g2_neg(const G2& p) { G2 r = p; r.y = f2_neg(p.y); return r; }
static inline bool g2_on_curve(const G2& p) { return p.inf || f2_eq(f2_sqr(p.y), f2_add(f2_mul(f2_sqr(p.x), p.x), b_twist())); }
// the slope of the line through a and b (the tangent when they are equal); false when that line is vertical
static inline bool g2_slope(const G2& a, const G2& b, Fq2* lam) {
  if (f2_eq(a.x, b.x)) {
    if (!f2_eq(a.y, b.y) || f2_is_zero(a.y)) return false;
    const Fq2 xx = f2_sqr(a.x);
    *lam = f2_mul(f2_add(f2_dbl(xx), xx), f2_inv(f2_dbl(a.y)));
    return true;
  }
  *lam = f2_mul(f2_sub(b.y, a.y), f2_inv(f2_sub(b.x, a.x)));
  return true;
}
static inline G2 g2_add_slope(const G2& a, const G2& b, const Fq2& lam) {
  G2 r; r.inf = false;
  r.x = f2_sub(f2_sub(f2_sqr(lam), a.x), b.x);
  r.y = f2_sub(f2_mul(lam, f2_sub(a.x, r.x)), a.y);
  return r;
}
static inline G2 g2_add(const G2& a, const G2& b) {
  if (a.inf) return b;
  if (b.inf) return a;
  Fq2 lam;
  if (!g2_slope(a, b, &lam)) return g2_inf();
  return g2_add_slope(a, b, lam);
}
// [k]P for a 256-bit k (4 x 64-bit limbs)
static inline G2 g2_mul(const G2& p, const uint64_t k[4]) {
  G2 acc = g2_inf();
  for (int i = 255; i >= 0; i--) { acc = g2_add(acc, acc); if ((k[i >> 6] >> (i & 63)) & 1) acc = g2_add(acc, p); }
  return acc;
}
static inline bool g2_in_subgroup(const G2& p) { return g2_on_curve(p) && g2_mul(p, fr::P).inf; }
static inline G2 g2_frobenius(const G2& p) { G2 r; r.inf = p.inf; r.x = f2_mul(f2_conj(p.x), gamma_x()); r.y = f2_mul(f2_conj(p.y), gamma_y()); return r; }

enum ParseResult { G2_OK = 0, G2_NOT_CANONICAL, G2_IDENTITY, G2_OFF_CURVE, G2_NOT_IN_SUBGROUP };
// 128 bytes -> a point of E' (no subgroup test here); mont: the coordinates are ark-ff's Montgomery limbs (this file's own form)
static inline ParseResult g2_parse(const uint8_t b[128], bool mont, G2* out) {
  Fq c[4]; bool all_zero = true;
  for (int i = 0; i < 4; i++) {
    memcpy(c[i].v, b + 32 * i, 32);
    if (geq_p(c[i].v)) return G2_NOT_CANONICAL;
    if (!is_zero(c[i])) all_zero = false;
    if (!mont) c[i] = to_mont(c[i]);
  }
  if (all_zero) return G2_IDENTITY;
  out->x = {c[0], c[1]}; out->y = {c[2], c[3]}; out->inf = false;
  return g2_on_curve(*out) ? G2_OK : G2_OFF_CURVE;
}
static inline ParseResult g2_parse_checked(const uint8_t b[128], bool mont, G2* out) {
  const ParseResult r = g2_parse(b, mont, out);
  if (r != G2_OK) return r;
  return g2_in_subgroup(*out) ? G2_OK : G2_NOT_IN_SUBGROUP;
}

// the non-adjacent form of 6u + 2, most significant digit first (it is 1 and starts the loop)
static inline std::vector<int> naf_schedule() {
  unsigned __int128 n = ((unsigned __int128)SBN_PAIRING_ATE_HI << 64) | SBN_PAIRING_ATE_LO;
  std::vector<int> d;
  while (n) {
    int z = 0;
    if (n & 1) { z = 2 - (int)(n & 3); if (z > 0) n -= 1; else n += 1; }
    d.push_back(z);
    n >>= 1;
  }
  return std::vector<int>(d.rbegin(), d.rend());
}

struct Line { uint32_t square_first; Fq2 neg_lam, c; };     // square_first: the accumulator is squared before this line (a doubling step)
// the lines of Q (a point of order r: no line of the loop is vertical; false if one is, which a checked point cannot cause)
static inline bool line_table(const G2& q, std::vector<Line>* out) {
  const std::vector<int> sch = naf_schedule();
  out->clear();
  G2 t = q;
  auto step = [&](const G2& b, uint32_t sq) {
    Fq2 lam;
    if (t.inf || b.inf || !g2_slope(t, b, &lam)) return false;
    out->push_back({sq, f2_neg(lam), f2_sub(f2_mul(lam, t.x), t.y)});
    t = g2_add_slope(t, b, lam);
    return true;
  };
  const G2 nq = g2_neg(q);
  for (size_t i = 1; i < sch.size(); i++) {
    if (!step(t, 1)) return false;
    if (sch[i] && !step(sch[i] > 0 ? q : nq, 0)) return false;
  }
  const G2 q1 = g2_frobenius(q), q2 = g2_neg(g2_frobenius(q1));
  return step(q1, 0) && step(q2, 0);
}
static const size_t LINE_BYTES = 128;      // -lam.c0 | -lam.c1 | c.c0 | c.c1
// canonical little-endian integers: what the model prints
static inline void lines_to_canonical(const std::vector<Line>& t, uint8_t* out) {
  for (size_t i = 0; i < t.size(); i++) {
    const Fq v[4] = {from_mont(t[i].neg_lam.c0), from_mont(t[i].neg_lam.c1), from_mont(t[i].c.c0), from_mont(t[i].c.c1)};
    for (int k = 0; k < 4; k++) memcpy(out + LINE_BYTES * i + 32 * k, v[k].v, 32);
  }
}
// the device's table: the same four values in fp.cuh's Montgomery form (R = 2^261), canonical; x 2^256 -> x 2^261 is one product with 32 * 2^256
static inline Fq to_device(const Fq& m) { const Fq k32 = {{32, 0, 0, 0}}; return mul(m, to_mont(k32)); }
static inline void lines_to_device(const std::vector<Line>& t, uint8_t* out, uint32_t* square_first) {
  for (size_t i = 0; i < t.size(); i++) {
    const Fq v[4] = {to_device(t[i].neg_lam.c0), to_device(t[i].neg_lam.c1), to_device(t[i].c.c0), to_device(t[i].c.c1)};
    for (int k = 0; k < 4; k++) memcpy(out + LINE_BYTES * i + 32 * k, v[k].v, 32);
    square_first[i] = t[i].square_first;
  }
}

}  // namespace pairing
}  // namespace sbn_host
