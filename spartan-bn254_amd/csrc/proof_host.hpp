// proof_host.hpp — what the one-call provers say to their Merlin transcript, host only: no HIP, no context, no launches.  The reference's
// ProofTranscript / AppendToTranscript (src/transcript.rs) in one place: every line a prover writes is one member of Script, so the byte stream of
// a proof is read off its calls.  tests/proof_host_check.cpp builds this header alone, under ASan + UBSan.
#pragma once
#include "host_field.hpp"
#include "host_strobe.hpp"

namespace sbn_host {

namespace fr {
static inline El fmul(const El& a, const El& b) { return mmul(to_m(a), b); }     // a * b, canonical in and out
}  // namespace fr

// 64 little-endian bytes mod r (Fr::from_le_bytes_mod_order, transcript.rs:56-67): lo + hi * 2^256, canonical
static inline void transcript_wide_reduce(const uint8_t b[64], uint8_t out[32]) {
  using namespace sbn_host::fr;
  El lo, hi; memcpy(lo.v, b, 32); memcpy(hi.v, b + 32, 32);
  const El zero = {{0, 0, 0, 0}};
  auto fold = [&](El x) { while (geq(x.v)) { uint64_t br = 0; for (int i = 0; i < 4; i++) { sbn_host::u128 d = (sbn_host::u128)x.v[i] - P[i] - br; x.v[i] = (uint64_t)d; br = (uint64_t)(d >> 127); } } return x; };   // < 2^256 < 6 r
  El r2; memcpy(r2.v, R2, 32);
  const El res = add(add(fold(lo), zero), mmul(fold(hi), r2));                  // hi * 2^512 / 2^256
  memcpy(out, res.v, 32);
}

// serialize_compressed of one affine point (canonical x ‖ y, all-zero for the identity): x with the flags in the top two bits
static inline void g1_compress(const uint8_t xy[64], uint8_t out32[32]) {
  bool inf = true; for (int k = 0; k < 64; k++) if (xy[k]) { inf = false; break; }
  if (inf) { memset(out32, 0, 32); out32[31] = 0x40; return; }
  memcpy(out32, xy, 32);
  // y > p - y  <=>  2y > p
  uint64_t y[4], t[4]; memcpy(y, xy + 32, 32);
  uint64_t cy = 0; for (int k = 0; k < 4; k++) { t[k] = (y[k] << 1) | cy; cy = y[k] >> 63; }
  bool gt = cy != 0;
  if (!gt) for (int k = 3; k >= 0; k--) { if (t[k] > QP[k]) { gt = true; break; } if (t[k] < QP[k]) break; }
  if (gt) out32[31] |= 0x80;
}

// a label as the transcript takes it: a C string of the prover's own, or the bytes and length a caller of the C ABI passed
struct Label {
  const uint8_t* p; size_t n;
  Label(const char* s) : p((const uint8_t*)s), n(strlen(s)) {}
  Label(const uint8_t* p_, size_t n_) : p(p_), n(n_) {}
};

struct Script {
  MerlinTranscript& t;
  void message(Label l, const void* msg, size_t len) { t.append_message(l.p, l.n, (const uint8_t*)msg, len); }
  void protocol(const char* name) { message("protocol-name", name, strlen(name)); }                      // append_protocol_name, transcript.rs:38-40
  void scalar(Label l, const uint8_t* p32) { message(l, p32, 32); }                                       // append_scalar, :42-44
  void scalars(Label l, const void* p, size_t n) { for (size_t i = 0; i < n; i++) scalar(l, (const uint8_t*)p + 32 * i); }     // a slice is one message per scalar, :46-50
  void point(Label l, const uint8_t* comp32) { message(l, comp32, 32); }                                  // append_point, :52-54
  void point_xy(Label l, const uint8_t xy64[64], uint8_t out32[32]) { g1_compress(xy64, out32); point(l, out32); }     // a GroupElement, :102-108
  void challenge(Label l, uint8_t out32[32]) { uint8_t b[64]; t.challenge_bytes(l.p, l.n, b, 64); transcript_wide_reduce(b, out32); }     // challenge_scalar, :56-67
  void challenges(Label l, uint8_t* out, size_t n) { for (size_t i = 0; i < n; i++) challenge(l, out + 32 * i); }                         // challenge_vector, :69-75
};

}  // namespace sbn_host
