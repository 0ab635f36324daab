// srs_host.hpp — the host half of the KZG SRS file (abi_kzg_srs.inc): the length field, the two G2 points and arkworks' G2 generator.
// Host only: no HIP, no context, no launches; built on pairing_host.hpp and includable alone.  tests/srs_host_check.cpp builds this header alone,
// under ASan + UBSan, and tests/test_srs_host_cpu.py compares it line by line with the literal model of tests/srs_model.py.
// The file is what #[derive(CanonicalSerialize)] writes for KZGSrs { powers_g1: Vec<G1Affine>, tau_g2: G2Affine, g2: G2Affine } in compressed mode
// (kzg.rs:66-115, ark-serialize 0.5):
//     n (u64 LE) | n x 32 B compressed G1 | tau_g2 64 B | g2 64 B | anything (ignored, as a read from a slice ignores it)
// A compressed G2 point is x.c0 then x.c1, 32 B each, little-endian canonical; bit 7 of byte 63 = "y is the larger of y and -y", bit 6 = identity.
// "Larger" orders Fq2 by c1 first and c0 on a tie (arkworks' Ord of a quadratic extension).  No arkworks source was at hand when this was written:
// the G2 byte order rests on that description (DESIGN, "the SRS from a file").
//   scan              n and the offsets, with 8 + 32 n + 128 <= len checked without overflow
//   f2_sqrt           the complex method for q = 3 mod 4 (tests/pairing_model.py: f2_sqrt)
//   g2_decompress     64 B -> 128 canonical bytes, through g2_parse_checked: every refusal of sbn_g2_prepare, and the flag refusals in front
//   g2_compress       128 B (canonical, or ark-ff Montgomery limbs) -> 64 B, through g2_parse_checked as well
//   g2_from_tau       g2 = arkworks' generator, tau_g2 = [tau] g2 (KZGSrs::setup, kzg.rs:37-56)
#pragma once
#include "pairing_host.hpp"

namespace sbn_host {
namespace srs {

using namespace pairing;

enum Err { SRS_OK = 0, SRS_SHORT, SRS_EMPTY, SRS_G2_NOT_CANONICAL, SRS_G2_FLAGS, SRS_G2_IDENTITY, SRS_G2_OFF_CURVE, SRS_G2_NOT_IN_SUBGROUP };
static inline const char* err_text(int e) {
  static const char* const t[] = {"", "the file is shorter than its length field says", "the file holds no powers (n = 0)", "a G2 coordinate is not canonical (>= q)",
                                  "a G2 point has both flag bits set", "a G2 point is the identity", "a G2 x has no y on the twist E'",
                                  "a G2 point is on E' but outside the r-torsion"};
  return t[e];
}

static const size_t HEAD_BYTES = 8, G1_BYTES = 32, G2_BYTES = 64, TAIL_BYTES = 2 * G2_BYTES;
struct Scan { uint64_t n; size_t powers_off, tau_g2_off, g2_off, end; };
// the size of a file of n powers; false where it does not fit a size_t
static inline bool file_bytes(uint64_t n, size_t* out) {
  if (n > (SIZE_MAX - HEAD_BYTES - TAIL_BYTES) / G1_BYTES) return false;
  *out = HEAD_BYTES + G1_BYTES * (size_t)n + TAIL_BYTES;
  return true;
}
static inline int scan(const uint8_t* b, size_t len, Scan* s) {
  if (len < HEAD_BYTES) return SRS_SHORT;
  uint64_t n = 0;
  for (int i = 7; i >= 0; i--) n = (n << 8) | b[i];
  if (n == 0) return SRS_EMPTY;
  size_t need = 0;
  if (!file_bytes(n, &need) || need > len) return SRS_SHORT;
  s->n = n; s->powers_off = HEAD_BYTES; s->tau_g2_off = HEAD_BYTES + G1_BYTES * (size_t)n; s->g2_off = s->tau_g2_off + G2_BYTES; s->end = need;
  return SRS_OK;
}

static inline Fq2 f2_one() { return {one(), zero()}; }
static inline Fq2 f2_pow(const Fq2& a, const uint64_t e[4]) {
  Fq2 r = f2_one();
  for (int i = 255; i >= 0; i--) { r = f2_sqr(r); if ((e[i >> 6] >> (i & 63)) & 1) r = f2_mul(r, a); }
  return r;
}
// (q - k) >> sh for the two exponents of the square root: q = ...47 in hex, so q - 3 and q - 1 do not borrow past limb 0
static inline void q_minus_shift(uint64_t k, int sh, uint64_t out[4]) {
  uint64_t t[4] = {QP[0] - k, QP[1], QP[2], QP[3]};
  for (int i = 0; i < 4; i++) out[i] = (t[i] >> sh) | (i < 3 ? t[i + 1] << (64 - sh) : 0);
}
// a square root of a in Fq2, or false (Montgomery form in and out)
static inline bool f2_sqrt(const Fq2& a, Fq2* out) {
  if (f2_is_zero(a)) { *out = a; return true; }
  uint64_t e34[4], e12[4];
  q_minus_shift(3, 2, e34); q_minus_shift(1, 1, e12);
  const Fq2 a1 = f2_pow(a, e34), x0 = f2_mul(a1, a), alpha = f2_mul(a1, x0);
  Fq2 x;
  if (f2_eq(alpha, f2_neg(f2_one()))) x = f2_mul({zero(), one()}, x0);
  else x = f2_mul(f2_pow(f2_add(f2_one(), alpha), e12), x0);
  if (!f2_eq(f2_sqr(x), a)) return false;
  *out = x;
  return true;
}
// a > b as canonical integers (Montgomery form in)
static inline bool fq_gt(const Fq& a, const Fq& b) {
  const Fq x = from_mont(a), y = from_mont(b);
  for (int i = 3; i >= 0; i--) { if (x.v[i] > y.v[i]) return true; if (x.v[i] < y.v[i]) return false; }
  return false;
}
// y > -y in arkworks' order of Fq2: c1 first, c0 on a tie
static inline bool f2_is_larger(const Fq2& y) {
  const Fq2 ny = f2_neg(y);
  if (!eq(y.c1, ny.c1)) return fq_gt(y.c1, ny.c1);
  return fq_gt(y.c0, ny.c0);
}
static inline void g2_to_bytes(const G2& p, uint8_t out[128]) {
  const Fq c[4] = {from_mont(p.x.c0), from_mont(p.x.c1), from_mont(p.y.c0), from_mont(p.y.c1)};
  for (int i = 0; i < 4; i++) memcpy(out + 32 * i, c[i].v, 32);
}
static inline int from_parse(ParseResult r) {
  switch (r) {
    case G2_OK: return SRS_OK;
    case G2_NOT_CANONICAL: return SRS_G2_NOT_CANONICAL;
    case G2_IDENTITY: return SRS_G2_IDENTITY;
    case G2_OFF_CURVE: return SRS_G2_OFF_CURVE;
    default: return SRS_G2_NOT_IN_SUBGROUP;
  }
}

// 64 compressed bytes -> 128 canonical bytes x.c0 | x.c1 | y.c0 | y.c1 of a point of G2; the order of the refusals is the order in which
// deserialize_compressed meets them (c0, the flags of c1, c1, the identity), then the curve and the subgroup
static inline int g2_decompress(const uint8_t in[64], uint8_t out_xy[128], G2* out_pt = nullptr) {
  Fq c0, c1;
  memcpy(c0.v, in, 32);
  if (geq_p(c0.v)) return SRS_G2_NOT_CANONICAL;
  const unsigned flags = in[63] >> 6;                   // bit 1: the larger root, bit 0: identity
  if (flags == 3) return SRS_G2_FLAGS;
  uint8_t hi[32]; memcpy(hi, in + 32, 32); hi[31] &= 0x3f;
  memcpy(c1.v, hi, 32);
  if (geq_p(c1.v)) return SRS_G2_NOT_CANONICAL;
  if (flags & 1) return SRS_G2_IDENTITY;
  G2 p; p.inf = false;
  p.x = {to_mont(c0), to_mont(c1)};
  Fq2 y;
  if (!f2_sqrt(f2_add(f2_mul(f2_sqr(p.x), p.x), b_twist()), &y)) return SRS_G2_OFF_CURVE;
  p.y = (f2_is_larger(y) == ((flags & 2) != 0)) ? y : f2_neg(y);
  g2_to_bytes(p, out_xy);
  G2 q;
  const int e = from_parse(g2_parse_checked(out_xy, false, &q));
  if (e == SRS_OK && out_pt) *out_pt = q;
  return e;
}
// 128 bytes (canonical, or ark-ff Montgomery limbs with mont) -> 64 compressed bytes; a point g2_parse_checked refuses is refused here
static inline int g2_compress(const uint8_t xy[128], bool mont, uint8_t out[64]) {
  G2 p;
  const int e = from_parse(g2_parse_checked(xy, mont, &p));
  if (e != SRS_OK) return e;
  uint8_t c[128]; g2_to_bytes(p, c);
  memcpy(out, c, 64);
  if (f2_is_larger(p.y)) out[63] |= 0x80;
  return SRS_OK;
}

// arkworks' generator of G2 (ark-bn254 g2.rs: G2_GENERATOR_X, _Y; tests/pairing_model.py: G2), canonical limbs x.c0, x.c1, y.c0, y.c1
static inline G2 g2_generator() {
  static const uint64_t k[4][4] = {{0x46debd5cd992f6edull, 0x674322d4f75edaddull, 0x426a00665e5c4479ull, 0x1800deef121f1e76ull},
                                   {0x97e485b7aef312c2ull, 0xf1aa493335a9e712ull, 0x7260bfb731fb5d25ull, 0x198e9393920d483aull},
                                   {0x4ce6cc0166fa7daaull, 0xe3d1e7690c43d37bull, 0x4aab71808dcb408full, 0x12c85ea5db8c6debull},
                                   {0x55acdadcd122975bull, 0xbc4b313370b38ef3ull, 0xec9e99ad690c3395ull, 0x090689d0585ff075ull}};
  Fq c[4];
  for (int i = 0; i < 4; i++) { memcpy(c[i].v, k[i], 32); c[i] = to_mont(c[i]); }
  G2 g; g.inf = false; g.x = {c[0], c[1]}; g.y = {c[2], c[3]};
  return g;
}
// g2 and [tau] g2 as 128 canonical bytes each; false for a tau that is zero or not canonical (>= r)
static inline bool g2_from_tau(const uint8_t tau[32], uint8_t out_g2_xy[128], uint8_t out_tau_g2_xy[128]) {
  uint64_t k[4]; memcpy(k, tau, 32);
  if (fr::geq(k) || (k[0] | k[1] | k[2] | k[3]) == 0) return false;
  const G2 g = g2_generator();
  g2_to_bytes(g, out_g2_xy);
  g2_to_bytes(g2_mul(g, k), out_tau_g2_xy);
  return true;
}

}  // namespace srs
}  // namespace sbn_host
