// circom_host.hpp — the host half of reading circom's .r1cs and .wtns files (reference src/r1cs_reader.rs:55-129, examples/keyless_benchmark.rs:38-72),
// host only: no HIP, no context, no launches.  The files are byte buffers the caller holds; nothing here copies an entry.
//   r1cs_scan    magic, version, the section walk, the header section's fields, where the constraints section's payload lies
//   r1cs_walk    the ONE sequential dependency of the format: the 3 * nConstraints entry counts, as two prefix arrays.  Run k = 3 i + m is matrix m
//                (A, B, C) of constraint i; run_first[k] = entries in all earlier runs (3 n + 1 values), mat_first[k] = entries of matrix m in earlier
//                constraints.  Entry e of run k starts at byte 4 (k + 1) + 36 (run_first[k] + e) of the payload: a u32 wire, then 32 value bytes.
//                Everything else about an entry is device work (circom_kernels.cuh)
//   wtns_scan    magic, the section walk, the one section of id 2 as (offset, number of 32-byte values)
//   shape        num_vars = nWires - 1 - num_pub_inputs, num_inputs = num_pub_inputs = nPubOut + nPubIn, num_cons = nConstraints, padded by
//                snark_host.hpp's shape_make.  examples/keyless_benchmark.rs:99 pads num_cons with next_power_of_two() alone where Instance::new
//                (snark.rs:82-88) takes max(num_cons, 2): the two differ for the one-constraint circuit only, which R1CSProof cannot take at 1 x n
//                anyway, so shape_make's rule is the one used
// Every read is checked against the buffer's length first.  What is refused is what the reference refuses (a wrong magic, a version other than 1, a
// field size other than 32, a missing section 1 or 2, a read past the end; nWires < 1 + num_pub_inputs, where its num_private_vars underflows), and
// TWO THINGS MORE, each a file the reference would misread without a word:
//   * a prime that is not BN254's r: the reference skips the prime's bytes and reads another field's values as if they were Fr's;
//   * a constraints walk that passes the end of section 2: the reference ignores section_size there and reads on into whatever section follows.
// The witness reader refuses where the example truncates or concatenates silently: a second section 2, a section that passes the end of the file, a
// size that is no multiple of 32.  (A value >= r, which the example replaces by its low 64 bits, is refused by sbn_circom_wtns_load on the device.)
// tests/circom_host_check.cpp builds this header alone, under ASan + UBSan.
#pragma once
#include "host_keccak.hpp"
#include "snark_host.hpp"
#include <vector>

namespace sbn_host {
namespace circom {

enum { OK = 0, E_SHORT, E_MAGIC, E_VERSION, E_NO_HEADER, E_NO_CONSTRAINTS, E_FIELD_SIZE, E_PRIME, E_WIRES, E_SECTION_END, E_TOO_MANY, E_WTNS_TWICE, E_WTNS_NONE, E_WTNS_SIZE };
static inline const char* why(int e) {
  static const char* const W[] = {"", "a read passes the end of the file", "the magic is wrong", "the version is not 1", "no header section (type 1)", "no constraints section (type 2)",
                                  "field_size is not 32", "the prime is not BN254's r", "nWires < 1 + nPubOut + nPubIn", "the constraints walk passes the end of section 2",
                                  "more than 2^31 entries", "a second witness section (id 2)", "no witness section (id 2)", "the witness section's size is no multiple of 32"};
  return (e >= 0 && e < (int)(sizeof W / sizeof W[0])) ? W[e] : "?";
}

static inline void put_u32(uint8_t* p, uint32_t x) { p[0] = (uint8_t)x; p[1] = (uint8_t)(x >> 8); p[2] = (uint8_t)(x >> 16); p[3] = (uint8_t)(x >> 24); }
static inline uint32_t get_u32(const uint8_t* p) { return (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24; }
// [off, off + n) lies inside a buffer of len bytes
static inline bool fits(size_t off, uint64_t n, size_t len) { return off <= len && n <= (uint64_t)(len - off); }

struct R1csScan {
  uint32_t field_size = 0;
  uint64_t n_wires = 0, n_pub_out = 0, n_pub_in = 0, n_prv_in = 0, n_labels = 0, n_cons = 0;
  uint64_t n_pub = 0;                        // num_pub_inputs = nPubOut + nPubIn (r1cs_reader.rs:120)
  size_t payload_off = 0, payload_len = 0;   // section 2 behind its 12-byte head
};

static const size_t HEADER_FIELDS = 4 + 32 + 4 * 4 + 8 + 4;      // field_size, prime, nWires, nPubOut, nPubIn, nPrvIn, nLabels, nConstraints

static inline int r1cs_scan(const uint8_t* p, size_t len, R1csScan* s) {
  if (!fits(0, 12, len)) return E_SHORT;
  if (memcmp(p, "r1cs", 4)) return E_MAGIC;                                       // r1cs_reader.rs:57-61
  if (get_u32(p + 4) != 1) return E_VERSION;                                      // :64-67
  const uint32_t nsec = get_u32(p + 8);                                           // :70
  size_t off = 12, head = 0, cons = 0; uint64_t cons_size = 0;                    // head / cons: the payload's offset of the first section of each type
  bool have_head = false, have_cons = false;
  for (uint32_t i = 0; i < nsec && !(have_head && have_cons); i++) {              // :101-126, :139-188: each walk stops at its first match
    if (!fits(off, 12, len)) return E_SHORT;
    const uint32_t type = get_u32(p + off); const uint64_t size = snark::get_u64(p + off + 4);
    off += 12;
    if (type == 1 && !have_head) { have_head = true; head = off; }
    if (type == 2 && !have_cons) { have_cons = true; cons = off; cons_size = size; }
    if (!fits(off, size, len)) {                                                  // a seek past the end: the next read fails, if there is one
      if (have_head && have_cons) break;
      return E_SHORT;
    }
    off += (size_t)size;
  }
  if (!have_head) return E_NO_HEADER;                                             // :128
  if (!fits(head, 4, len)) return E_SHORT;
  s->field_size = get_u32(p + head);                                              // :107
  if (s->field_size != 32) return E_FIELD_SIZE;                                   // :76-78
  if (!fits(head, HEADER_FIELDS, len)) return E_SHORT;
  {
    uint8_t r[32]; memcpy(r, fr::P, 32);                                          // (little-endian host, as everywhere in this library)
    if (memcmp(p + head + 4, r, 32)) return E_PRIME;                              // beyond the reference, which skips these bytes (:110)
  }
  const uint8_t* q = p + head + 36;
  s->n_wires = get_u32(q); s->n_pub_out = get_u32(q + 4); s->n_pub_in = get_u32(q + 8); s->n_prv_in = get_u32(q + 12);      // :112-115
  s->n_labels = snark::get_u64(q + 16); s->n_cons = get_u32(q + 24);              // :116-117
  s->n_pub = s->n_pub_out + s->n_pub_in;
  if (s->n_wires < 1 + s->n_pub) return E_WIRES;                                  // num_private_vars (:255-257) underflows
  if (!have_cons) return E_NO_CONSTRAINTS;                                        // :190
  if (!fits(cons, cons_size, len)) return E_SHORT;
  s->payload_off = cons; s->payload_len = (size_t)cons_size;
  return OK;
}

// run_first: 3 n + 1 values, mat_first: 3 n; nnz[m]: the entries of matrix m.  Refused: a count or a record that passes the end of the section (beyond
// the reference), more than 2^31 entries in all or in one matrix (what sbn_r1cs_upload and sbn_dense_build take)
static inline int r1cs_walk(const uint8_t* p, const R1csScan& s, std::vector<uint32_t>& run_first, std::vector<uint32_t>& mat_first, uint64_t nnz[3]) {
  const uint8_t* sec = p + s.payload_off;
  const size_t L = s.payload_len;
  const uint64_t nruns = 3 * s.n_cons;
  if (nruns * 4 > L) return E_SECTION_END;                                        // every run has its count: nothing is allocated for a file that cannot hold them
  run_first.assign((size_t)nruns + 1, 0); mat_first.assign((size_t)nruns, 0);
  uint64_t total = 0; nnz[0] = nnz[1] = nnz[2] = 0;
  size_t pos = 0;
  for (uint64_t k = 0; k < nruns; k++) {
    if (!fits(pos, 4, L)) return E_SECTION_END;
    const uint64_t cnt = get_u32(sec + pos);                                      // r1cs_reader.rs:151, :162, :173
    pos += 4;
    if (!fits(pos, 36 * cnt, L)) return E_SECTION_END;
    pos += (size_t)(36 * cnt);
    run_first[(size_t)k] = (uint32_t)total; mat_first[(size_t)k] = (uint32_t)nnz[k % 3];
    total += cnt; nnz[k % 3] += cnt;
    if (total > ((uint64_t)1 << 31)) return E_TOO_MANY;
  }
  run_first[(size_t)nruns] = (uint32_t)total;
  return OK;
}

struct WtnsSpan { size_t off = 0, count = 0; };      // the values of section 2: `count` records of 32 bytes from byte `off` of the file

static inline int wtns_scan(const uint8_t* p, size_t len, WtnsSpan* w) {
  if (!fits(0, 4, len)) return E_SHORT;
  if (memcmp(p, "wtns", 4)) return E_MAGIC;                                       // keyless_benchmark.rs:43-45
  if (!fits(0, 12, len)) return E_SHORT;
  const uint32_t nsec = get_u32(p + 8);                                           // :47
  size_t off = 12; bool have = false;
  for (uint32_t i = 0; i < nsec; i++) {                                           // :51-70
    if (!fits(off, 12, len)) return E_SHORT;                                      // the example stops here without a word
    const uint32_t id = get_u32(p + off); const uint64_t size = snark::get_u64(p + off + 4);
    off += 12;
    if (!fits(off, size, len)) return E_SHORT;                                    // the example keeps the values that are there
    if (id == 2) {
      if (have) return E_WTNS_TWICE;                                              // the example appends the second section's values to the first's
      if (size % 32) return E_WTNS_SIZE;                                          // the example drops the tail
      have = true; w->off = off; w->count = (size_t)(size / 32);
    }
    off += (size_t)size;
  }
  return have ? OK : E_WTNS_NONE;
}

// the raw shape a circuit file gives Instance::new (r1cs_reader.rs:255-257, keyless_benchmark.rs:96-100 with snark.rs:74-90's padding)
static inline bool shape_of(const R1csScan& s, snark::Shape* sh) {
  return snark::shape_make((size_t)s.n_cons, (size_t)(s.n_wires - 1 - s.n_pub), (size_t)s.n_pub, sh);
}

// ---- the circuit digest: THE LIBRARY'S OWN.  It is not the reference's R1CSShape::get_digest (zlib over bincode, r1cs.rs:97-101), which is not
//      reproduced here: a proof made under one digest does not verify under the other.  It binds a NIZK proof to its circuit for a caller who has no
//      Rust side to ask.  Defined over what sbn_circom_r1cs_download returns — kept entries in file order, remapped columns, canonical values — and
//      not over file bytes, so section order and dropped (>= r) entries do not change it:
//        leaf(m, j) = SHAKE256("sbn254/r1cs-digest/leaf/v1" | u8 m | u64le j | u32le k | k x (u32le row | u32le col | val[32]))[0..32]
//                     entries 128 j .. 128 j + k - 1 of matrix m, k = min(128, nnz[m] - 128 j); no leaf for nnz[m] = 0
//        root       = SHAKE256("sbn254/r1cs-digest/root/v1" | u64le num_constraints | num_variables | num_pub_inputs | num_cons_padded | num_vars_padded
//                              | for m = 0, 1, 2: u64le nnz[m] | the leaves of m in order)[0..32]
//      The leaves are device work (circom_kernels.cuh: k_circom_digest_leaves); digest_leaf below is the same function on the host, for the checks
//      (tests/circuit_digest_check.cpp builds the three functions alone, under ASan + UBSan) ----
static const char DIGEST_LEAF_DOMAIN[] = "sbn254/r1cs-digest/leaf/v1";      // 26 bytes: with u8 m, u64 j and u32 k a header of 39
static const char DIGEST_ROOT_DOMAIN[] = "sbn254/r1cs-digest/root/v1";
static const size_t DIGEST_LEAF_ENTRIES = 128;
static inline size_t digest_leaves(uint64_t nnz) { return (size_t)((nnz + DIGEST_LEAF_ENTRIES - 1) / DIGEST_LEAF_ENTRIES); }

// rows, cols, vals: the k entries of the leaf
static inline void digest_leaf(uint8_t m, uint64_t j, uint32_t k, const uint32_t* rows, const uint32_t* cols, const uint8_t* vals, uint8_t out[32]) {
  Keccak h(136, 0x1f);
  uint8_t b[8];
  h.absorb((const uint8_t*)DIGEST_LEAF_DOMAIN, sizeof DIGEST_LEAF_DOMAIN - 1);
  h.absorb(&m, 1);
  snark::put_u64(b, j); h.absorb(b, 8);
  put_u32(b, k); h.absorb(b, 4);
  for (uint32_t e = 0; e < k; e++) {
    put_u32(b, rows[e]); put_u32(b + 4, cols[e]);
    h.absorb(b, 8);
    h.absorb(vals + 32 * (size_t)e, 32);
  }
  h.squeeze(out, 32);
}

// shape: num_constraints, num_variables, num_pub_inputs, num_cons_padded, num_vars_padded; leaves[m]: digest_leaves(nnz[m]) x 32 bytes
static inline void digest_root(const uint64_t shape[5], const uint64_t nnz[3], const uint8_t* const leaves[3], uint8_t out[32]) {
  Keccak h(136, 0x1f);
  uint8_t b[8];
  h.absorb((const uint8_t*)DIGEST_ROOT_DOMAIN, sizeof DIGEST_ROOT_DOMAIN - 1);
  for (int i = 0; i < 5; i++) { snark::put_u64(b, shape[i]); h.absorb(b, 8); }
  for (int m = 0; m < 3; m++) {
    snark::put_u64(b, nnz[m]); h.absorb(b, 8);
    h.absorb(leaves[m], 32 * digest_leaves(nnz[m]));
  }
  h.squeeze(out, 32);
}

}  // namespace circom
}  // namespace sbn_host
