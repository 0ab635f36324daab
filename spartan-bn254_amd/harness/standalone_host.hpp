// standalone_host.hpp — the file formats of harness/sbn_spartan.cpp, host only: no HIP, no context, nothing of the library.  tests/standalone_host_check.cpp
// builds this header alone, under ASan + UBSan.
//
// The proof file, all little-endian:
//     "SBNP" 4 B | version = 1 u32 | mode u8 (0 snark, 1 nizk) | kzg u8 (0, 1; 1 in snark mode only) | 0 u16
//     | num_cons, num_vars, num_inputs, num_nz_entries u64 each, RAW as the circuit has them (what sbn_snark_gens_new / sbn_nizk_gens_new take)
//     | digest_len u32, then the digest (NIZK mode: the circuit digest the prover absorbed; informational — the verifier computes its own)
//     | inputs 32 B each, canonical | proof_len u64, then the proof bytes (what sbn_snark_prove[_kzg] / sbn_nizk_prove wrote)
// The reader takes nothing on trust: every read is checked against the buffer's length first, every length against what is left WITHOUT forming a sum
// that can wrap, and it refuses every short file, every length that overflows or passes the end, a non-canonical input, trailing bytes, an unknown version,
// mode, kzg or reserved field, and a mode or kzg byte that contradicts what the command line asked for.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>
#include <vector>

namespace sbn_standalone {

enum { MODE_SNARK = 0, MODE_NIZK = 1 };
enum { OK = 0, E_SHORT, E_MAGIC, E_VERSION, E_MODE, E_KZG, E_RESERVED, E_LENGTH, E_INPUT, E_TRAILING, E_MODE_MISMATCH, E_KZG_MISMATCH };
static inline const char* why(int e) {
  static const char* const W[] = {"", "the file is shorter than its fields say", "the magic is not SBNP", "the version is not 1", "the mode byte is neither 0 (snark) nor 1 (nizk)",
                                  "the kzg byte is neither 0 nor 1, or 1 in nizk mode", "the reserved field is not 0", "a length field overflows or passes the end of the file",
                                  "an input is not canonical (>= r)", "bytes behind the proof", "the file's mode is not the one asked for", "the file's build (Hyrax / KZG) is not the one asked for"};
  return (e >= 0 && e < (int)(sizeof W / sizeof W[0])) ? W[e] : "?";
}

struct ProofFile {
  uint8_t mode = 0, kzg = 0;
  uint64_t num_cons = 0, num_vars = 0, num_inputs = 0, num_nz_entries = 0;
  std::vector<uint8_t> digest, inputs, proof;      // inputs: 32 num_inputs bytes
};

static inline void put_le(std::vector<uint8_t>& o, uint64_t x, int n) { for (int k = 0; k < n; k++) o.push_back((uint8_t)(x >> (8 * k))); }
static inline uint64_t get_le(const uint8_t* p, int n) { uint64_t x = 0; for (int k = 0; k < n; k++) x |= (uint64_t)p[k] << (8 * k); return x; }

// 32 little-endian bytes below BN254's r
static inline bool fr_canonical(const uint8_t b[32]) {
  static const uint8_t R[32] = {0x01, 0x00, 0x00, 0xf0, 0x93, 0xf5, 0xe1, 0x43, 0x91, 0x70, 0xb9, 0x79, 0x48, 0xe8, 0x33, 0x28,
                                0x5d, 0x58, 0x81, 0x81, 0xb6, 0x45, 0x50, 0xb8, 0x29, 0xa0, 0x31, 0xe1, 0x72, 0x4e, 0x64, 0x30};
  for (int i = 31; i >= 0; i--) { if (b[i] < R[i]) return true; if (b[i] > R[i]) return false; }
  return false;
}

static inline std::vector<uint8_t> write_proof_file(const ProofFile& f) {
  std::vector<uint8_t> o;
  o.insert(o.end(), {'S', 'B', 'N', 'P'});
  put_le(o, 1, 4); o.push_back(f.mode); o.push_back(f.kzg); put_le(o, 0, 2);
  put_le(o, f.num_cons, 8); put_le(o, f.num_vars, 8); put_le(o, f.num_inputs, 8); put_le(o, f.num_nz_entries, 8);
  put_le(o, f.digest.size(), 4); o.insert(o.end(), f.digest.begin(), f.digest.end());
  o.insert(o.end(), f.inputs.begin(), f.inputs.end());
  put_le(o, f.proof.size(), 8); o.insert(o.end(), f.proof.begin(), f.proof.end());
  return o;
}

// want_mode / want_kzg: what the command line asked for, or -1 for "whatever the file says"
static inline int read_proof_file(const uint8_t* p, size_t len, int want_mode, int want_kzg, ProofFile* f) {
  size_t off = 0;
  auto left = [&]() { return len - off; };                            // off <= len always
  if (left() < 4) return E_SHORT;
  if (memcmp(p, "SBNP", 4)) return E_MAGIC;
  off = 4;
  if (left() < 8) return E_SHORT;
  if (get_le(p + off, 4) != 1) return E_VERSION;
  f->mode = p[off + 4]; f->kzg = p[off + 5];
  if (f->mode > 1) return E_MODE;
  if (f->kzg > 1 || (f->kzg && f->mode == MODE_NIZK)) return E_KZG;
  if (get_le(p + off + 6, 2) != 0) return E_RESERVED;
  off += 8;
  if (want_mode >= 0 && want_mode != f->mode) return E_MODE_MISMATCH;
  if (want_kzg >= 0 && want_kzg != f->kzg) return E_KZG_MISMATCH;
  if (left() < 32) return E_SHORT;
  f->num_cons = get_le(p + off, 8); f->num_vars = get_le(p + off + 8, 8); f->num_inputs = get_le(p + off + 16, 8); f->num_nz_entries = get_le(p + off + 24, 8);
  off += 32;
  if (left() < 4) return E_SHORT;
  const uint64_t dl = get_le(p + off, 4);
  off += 4;
  if (dl > left()) return E_LENGTH;
  f->digest.assign(p + off, p + off + (size_t)dl);
  off += (size_t)dl;
  if (f->num_inputs > left() / 32) return E_LENGTH;                   // (no 32 * num_inputs is formed before this)
  const size_t ib = 32 * (size_t)f->num_inputs;
  for (size_t i = 0; i < ib; i += 32) if (!fr_canonical(p + off + i)) return E_INPUT;
  f->inputs.assign(p + off, p + off + ib);
  off += ib;
  if (left() < 8) return E_SHORT;
  const uint64_t pl = get_le(p + off, 8);
  off += 8;
  if (pl > left()) return E_LENGTH;
  f->proof.assign(p + off, p + off + (size_t)pl);
  off += (size_t)pl;
  if (off != len) return E_TRAILING;
  return OK;
}

// ---- the proof's fields as byte spans, from the layouts of include/sbn254.h (what tests/snark_model.proof_spans and nizk_model.r_span give):
//      snark: r1cs_sat_proof | inst_evals [96] | r1cs_eval_proof;   nizk: r1cs_sat_proof | rx [32 nx] | ry [32 ny].
//      sat_bytes: sbn_r1cs_proof_sizes' proof length at the padded shape ----
struct Span { const char* name; size_t first, end; };
static inline std::vector<Span> proof_spans(int mode, size_t sat_bytes, size_t nx, size_t ny, size_t proof_bytes) {
  std::vector<Span> s;
  s.push_back({"r1cs_sat_proof", 0, sat_bytes});
  if (mode == MODE_SNARK) { s.push_back({"inst_evals", sat_bytes, sat_bytes + 96}); s.push_back({"r1cs_eval_proof", sat_bytes + 96, proof_bytes}); }
  else { s.push_back({"rx", sat_bytes, sat_bytes + 32 * nx}); s.push_back({"ry", sat_bytes + 32 * nx, sat_bytes + 32 * (nx + ny)}); }
  return s;
}

}  // namespace sbn_standalone
