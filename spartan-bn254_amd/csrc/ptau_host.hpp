// ptau_host.hpp — the host half of a powers-of-tau ceremony file (.ptau) as the KZG SRS (abi_kzg_srs.inc: sbn_ptau_scan, sbn_kzg_srs_load_ptau):
// the section table, the header section and the two G2 points.  Host only: no HIP, no context, no launches; built on pairing_host.hpp and includable
// alone.  tests/ptau_host_check.cpp builds this header alone, under ASan + UBSan, and tests/test_ptau_host_cpu.py compares it line by line with the
// literal model of tests/ptau_model.py.
// The format (all integers little-endian; written from a description, NOT compared with a file snarkjs wrote: DESIGN 4.26):
//     "ptau" | u32 version = 1 | u32 nSections | nSections x ( u32 id | u64 size | size bytes )
//     section 1   u32 n8 = 32 | n8 bytes q | u32 power | u32 ceremonyPower            (44 bytes)
//     section 2   2^(power+1) - 1 points of G1, 64 B each: x | y;  point i = [tau^i] G1
//     section 3   2^power points of G2, 128 B each: x.c0 | x.c1 | y.c0 | y.c1;  point i = [tau^i] G2 (only 0 and 1 are read)
// A coordinate is 32 bytes of v 2^256 mod q: ark-ff's Montgomery limbs, this file's own form (host_field.hpp).  All-zero bytes are the identity.
// Sections come in any order; ids other than 1, 2, 3 are skipped; a second section 1, 2 or 3 is refused.
//   scan          walks the table: every offset and size against len, without overflow.  Never touches a point.
//   g2_convert    128 B Montgomery -> 128 canonical bytes, through g2_parse_checked: every refusal of sbn_g2_prepare, the identity and the r-torsion included
#pragma once
#include "pairing_host.hpp"

namespace sbn_host {
namespace ptau {

using namespace pairing;

enum Err { PTAU_OK = 0, PTAU_SHORT, PTAU_MAGIC, PTAU_VERSION, PTAU_SECTION_PAST_END, PTAU_DUPLICATE, PTAU_MISSING, PTAU_HEADER_SIZE, PTAU_N8, PTAU_PRIME,
           PTAU_POWER, PTAU_G1_SIZE, PTAU_G2_SIZE, PTAU_G2_NOT_CANONICAL, PTAU_G2_IDENTITY, PTAU_G2_OFF_CURVE, PTAU_G2_NOT_IN_SUBGROUP };
static inline const char* err_text(int e) {
  static const char* const t[] = {"", "the file ends inside its header or its section table", "the file does not begin with 'ptau'", "the version is not 1",
                                  "a section runs past the end of the file", "section 1, 2 or 3 comes twice", "section 1, 2 or 3 is missing",
                                  "section 1 does not hold 44 bytes", "n8 is not 32", "the prime is not BN254's q", "power is outside 1 .. 28",
                                  "section 2 does not hold 2^(power+1) - 1 points of 64 bytes", "section 3 does not hold 2^power points of 128 bytes",
                                  "a G2 coordinate is not canonical (>= q)", "a G2 point is the identity", "a G2 point is not on the twist E'",
                                  "a G2 point is on E' but outside the r-torsion"};
  return t[e];
}

static const size_t HEAD_BYTES = 12, SECTION_HEAD_BYTES = 12, HEADER_SECTION_BYTES = 44, G1_BYTES = 64, G2_BYTES = 128;
static const uint32_t MAX_POWER = 28;
struct Scan { uint32_t power, ceremony_power; uint64_t n_g1, n_g2; size_t off_g1, off_g2; };

static inline uint32_t rd32(const uint8_t* p) { return (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24; }
static inline uint64_t rd64(const uint8_t* p) { return (uint64_t)rd32(p) | (uint64_t)rd32(p + 4) << 32; }

static inline int scan(const uint8_t* b, size_t len, Scan* s) {
  if (len < HEAD_BYTES) return PTAU_SHORT;
  if (memcmp(b, "ptau", 4)) return PTAU_MAGIC;
  if (rd32(b + 4) != 1) return PTAU_VERSION;
  const uint32_t nsec = rd32(b + 8);
  size_t off[4] = {0, 0, 0, 0}; uint64_t size[4] = {0, 0, 0, 0}; bool have[4] = {false, false, false, false};
  size_t pos = HEAD_BYTES;                                   // pos <= len throughout
  for (uint32_t k = 0; k < nsec; k++) {
    if (len - pos < SECTION_HEAD_BYTES) return PTAU_SHORT;
    const uint32_t id = rd32(b + pos);
    const uint64_t sz = rd64(b + pos + 4);
    pos += SECTION_HEAD_BYTES;
    if (sz > (uint64_t)(len - pos)) return PTAU_SECTION_PAST_END;
    if (id >= 1 && id <= 3) {
      if (have[id]) return PTAU_DUPLICATE;
      have[id] = true; off[id] = pos; size[id] = sz;
    }
    pos += (size_t)sz;
  }
  if (!have[1] || !have[2] || !have[3]) return PTAU_MISSING;
  if (size[1] < 4) return PTAU_HEADER_SIZE;
  const uint8_t* h = b + off[1];
  if (rd32(h) != 32) return PTAU_N8;
  if (size[1] != HEADER_SECTION_BYTES) return PTAU_HEADER_SIZE;
  uint64_t q[4];
  for (int i = 0; i < 4; i++) q[i] = rd64(h + 4 + 8 * i);
  for (int i = 0; i < 4; i++) if (q[i] != QP[i]) return PTAU_PRIME;
  const uint32_t power = rd32(h + 36);
  if (power < 1 || power > MAX_POWER) return PTAU_POWER;      // so 64 (2^(power+1) - 1) < 2^35: no product below can overflow
  const uint64_t n_g1 = ((uint64_t)2 << power) - 1, n_g2 = (uint64_t)1 << power;
  if (size[2] != G1_BYTES * n_g1) return PTAU_G1_SIZE;
  if (size[3] != G2_BYTES * n_g2) return PTAU_G2_SIZE;
  s->power = power; s->ceremony_power = rd32(h + 40); s->n_g1 = n_g1; s->n_g2 = n_g2; s->off_g1 = off[2]; s->off_g2 = off[3];
  return PTAU_OK;
}

// 128 Montgomery bytes x.c0 | x.c1 | y.c0 | y.c1 -> 128 canonical bytes of a point of G2
static inline int g2_convert(const uint8_t in[128], uint8_t out_xy[128], G2* out_pt = nullptr) {
  for (int i = 0; i < 4; i++) {
    Fq c;
    memcpy(c.v, in + 32 * i, 32);
    if (geq_p(c.v)) return PTAU_G2_NOT_CANONICAL;
    c = from_mont(c);
    memcpy(out_xy + 32 * i, c.v, 32);
  }
  G2 q;
  switch (g2_parse_checked(out_xy, false, &q)) {
    case G2_OK: break;
    case G2_NOT_CANONICAL: return PTAU_G2_NOT_CANONICAL;
    case G2_IDENTITY: return PTAU_G2_IDENTITY;
    case G2_OFF_CURVE: return PTAU_G2_OFF_CURVE;
    default: return PTAU_G2_NOT_IN_SUBGROUP;
  }
  if (out_pt) *out_pt = q;
  return PTAU_OK;
}

}  // namespace ptau
}  // namespace sbn_host
