// snark_host.hpp — what SNARK::encode / prove / verify (snark.rs:59-158, :290-529) add around the two halves that already run in one call each, host
// only: no HIP, no context, no launches.
//   shape_make          Instance::new's and SNARKGens::new's padding of a raw shape (snark.rs:74-90, :306-319)
//   convert_cols        Instance::new's triplet conversion (:92-110): the three errors and the column shift; entry order is kept
//   comm_build / _parse R1CSCommitment as bytes: six u64, then the compressed row commitments of comb_ops and comb_mem
//   prefix              the transcript lines in front of R1CSProof: the protocol name and R1CSCommitment::append_to_transcript (r1cs.rs:355-362,
//                       sparse_mlpoly_full.rs:710-717, hyrax.rs:44-51), through proof_host.hpp's Script
//   sizes               rnd = r1cs rnd | sparse rnd (ONE RandomTape, draws in call order); proof = r1cs_sat_proof | inst_evals [96] | r1cs_eval_proof
//   nizk_prefix / nizk_sizes   NIZK mode (snark.rs:162-287): the protocol name and the caller's digest bytes; proof = r1cs_sat_proof | rx | ry
// tests/snark_host_check.cpp and tests/nizk_host_check.cpp build this header alone, under ASan + UBSan.
#pragma once
#include "proof_host.hpp"
#include <vector>

namespace sbn_host {
namespace snark {

static const uint64_t BATCH = 3;                       // A, B, C
static const size_t SHAPE_MAX = (size_t)1 << 29;       // what sbn_r1cs_upload takes
static const size_t HEADER_BYTES = 48;

static inline size_t npo2(size_t n) { size_t p = 1; while (p < n) p <<= 1; return p; }      // next_power_of_two, with next_power_of_two(0) = 1
static inline size_t log2u(size_t n) { size_t l = 0; while (((size_t)1 << l) < n) l++; return l; }
static inline bool is_pow2(uint64_t n) { return n && !(n & (n - 1)); }

// the raw shape a circuit comes with, and what Instance::new makes of it
struct Shape { size_t num_cons, num_vars, num_inputs, nc, nv, nx, ny; };      // nc, nv: padded; nx = log2 nc, ny = log2(2 nv)
static inline bool shape_make(size_t num_cons, size_t num_vars, size_t num_inputs, Shape* s) {
  if (num_cons > SHAPE_MAX || num_vars > SHAPE_MAX || num_inputs >= SHAPE_MAX) return false;
  s->num_cons = num_cons; s->num_vars = num_vars; s->num_inputs = num_inputs;
  s->nv = npo2(num_vars > num_inputs + 1 ? num_vars : num_inputs + 1);          // snark.rs:75-81
  s->nc = npo2(num_cons > 2 ? num_cons : 2);                                    // :82-88
  s->nx = log2u(s->nc); s->ny = log2u(2 * s->nv);
  return true;
}

// Instance::new's convert (snark.rs:92-110) on one matrix: out_cols[e] = the column entry e has in the padded instance.  Rows and values stay
// where they are and entry order is kept (sbn_dense_build's timestamps depend on it).  *bad: the first entry that is refused
enum { CONV_OK = 0, CONV_ROW = 1, CONV_COL = 2, CONV_VAL = 3 };
static inline int convert_cols(const Shape& s, const uint32_t* rows, const uint32_t* cols, const uint8_t* vals, size_t nnz, uint32_t* out_cols, size_t* bad) {
  for (size_t e = 0; e < nnz; e++) {
    if (bad) *bad = e;
    if (rows[e] >= s.num_cons) return CONV_ROW;                                 // :95-97
    if (cols[e] >= s.num_vars + 1 + s.num_inputs) return CONV_COL;              // :98-100
    uint64_t v[4]; memcpy(v, vals + 32 * e, 32);
    if (fr::geq(v)) return CONV_VAL;                                            // Scalar::from_bytes, :101
    out_cols[e] = cols[e] >= s.num_vars ? (uint32_t)(cols[e] + (s.nv - s.num_vars)) : cols[e];      // :102-106
  }
  return CONV_OK;
}

// ---- R1CSCommitment as bytes: num_cons_padded | num_vars_padded | num_inputs | batch (3) | num_ops N | num_mem_cells as little-endian u64, then
//      comm_comb_ops [L_ops x 32] and comm_comb_mem [L_mem x 32], compressed points ----
struct Comm { uint64_t nc, nv, ni, batch, N, cells; size_t nx, ny, L_ops, L_mem; };
static inline size_t ell_ops(size_t N) { return log2u(N) + log2u(npo2(5 * BATCH)); }      // sparse_mlpoly_full.rs:619-620
static inline size_t ell_mem(size_t cells) { return log2u(cells) + 1; }                   // :621
static inline void comm_lens(Comm* c) {
  c->nx = log2u(c->nc); c->ny = log2u(2 * c->nv);
  c->L_ops = (size_t)1 << (ell_ops(c->N) / 2); c->L_mem = (size_t)1 << (ell_mem(c->cells) / 2);      // 2^left of compute_factored_lens
}
static inline Comm comm_of(const Shape& s, size_t N) {
  Comm c; c.nc = s.nc; c.nv = s.nv; c.ni = s.num_inputs; c.batch = BATCH; c.N = N; c.cells = (uint64_t)1 << (s.nx > s.ny ? s.nx : s.ny);
  comm_lens(&c);
  return c;
}
static inline size_t comm_bytes(const Comm& c) { return HEADER_BYTES + 32 * (c.L_ops + c.L_mem); }
static inline void put_u64(uint8_t* p, uint64_t x) { for (int k = 0; k < 8; k++) p[k] = (uint8_t)(x >> (8 * k)); }
static inline uint64_t get_u64(const uint8_t* p) { uint64_t x = 0; for (int k = 0; k < 8; k++) x |= (uint64_t)p[k] << (8 * k); return x; }
// a compressed point as the reference's deserialisation and serialisation leave it: the identity is the flag alone
static inline void normalise(const uint8_t in[32], uint8_t out[32]) {
  memcpy(out, in, 32);
  if (out[31] & 0x40) { memset(out, 0, 32); out[31] = 0x40; }
}
static inline std::vector<uint8_t> comm_build(const Comm& c, const uint8_t* ops32, const uint8_t* mem32) {
  std::vector<uint8_t> out(comm_bytes(c));
  const uint64_t h[6] = {c.nc, c.nv, c.ni, c.batch, c.N, c.cells};
  for (int k = 0; k < 6; k++) put_u64(out.data() + 8 * k, h[k]);
  for (size_t i = 0; i < c.L_ops; i++) normalise(ops32 + 32 * i, out.data() + HEADER_BYTES + 32 * i);
  for (size_t i = 0; i < c.L_mem; i++) normalise(mem32 + 32 * i, out.data() + HEADER_BYTES + 32 * (c.L_ops + i));
  return out;
}
// every field is checked before anything is derived from it; the points are not decompressed here
enum { COMM_OK = 0, COMM_SHORT, COMM_CONS, COMM_VARS, COMM_INPUTS, COMM_BATCH, COMM_OPS, COMM_CELLS, COMM_LENGTH };
static inline int comm_parse(const uint8_t* p, size_t len, Comm* c) {
  if (len < HEADER_BYTES) return COMM_SHORT;
  c->nc = get_u64(p); c->nv = get_u64(p + 8); c->ni = get_u64(p + 16); c->batch = get_u64(p + 24); c->N = get_u64(p + 32); c->cells = get_u64(p + 40);
  if (!is_pow2(c->nc) || c->nc < 2 || c->nc > SHAPE_MAX) return COMM_CONS;
  if (!is_pow2(c->nv) || c->nv > SHAPE_MAX) return COMM_VARS;
  if (c->ni >= c->nv) return COMM_INPUTS;                                       // num_vars_padded >= num_inputs + 1
  if (c->batch != BATCH) return COMM_BATCH;
  if (!is_pow2(c->N) || c->N < 2 || c->N > ((uint64_t)1 << 31)) return COMM_OPS;      // product_tree.rs:89: the dot-product circuits are split
  const size_t nx = log2u((size_t)c->nc), ny = log2u(2 * (size_t)c->nv);
  if (c->cells != (uint64_t)1 << (nx > ny ? nx : ny)) return COMM_CELLS;        // sparse_mlpoly_full.rs:145-149
  comm_lens(c);
  if (len != comm_bytes(*c)) return COMM_LENGTH;
  return COMM_OK;
}
static inline const uint8_t* comm_ops(const Comm&, const uint8_t* p) { return p + HEADER_BYTES; }
static inline const uint8_t* comm_mem(const Comm& c, const uint8_t* p) { return p + HEADER_BYTES + 32 * c.L_ops; }

// ---- the transcript in front of R1CSProof::prove / ::verify (snark.rs:440-442, :496-498).  `after` is called behind every line ----
struct NoHook { void operator()() const {} };
template <class Hook = NoHook>
static inline void prefix(Script& ts, const Comm& c, const uint8_t* comm, Hook after = Hook()) {
  auto u64 = [&](const char* label, uint64_t x) { uint8_t b[8]; put_u64(b, x); ts.message(label, b, 8); after(); };      // Merlin's append_u64
  ts.protocol("Spartan SNARK proof"); after();
  u64("num_cons", c.nc); u64("num_vars", c.nv); u64("num_inputs", c.ni);        // r1cs.rs:358-360
  u64("batch_size", c.batch); u64("num_ops", c.N); u64("num_mem_cells", c.cells);      // sparse_mlpoly_full.rs:712-714
  auto poly = [&](const char* label, const uint8_t* pts, size_t n) {            // PolyCommitment::append_to_transcript, hyrax.rs:44-51
    ts.message(label, "poly_commitment_begin", 21); after();
    for (size_t i = 0; i < n; i++) { uint8_t b[32]; normalise(pts + 32 * i, b); ts.point("poly_commitment_share", b); after(); }
    ts.message(label, "poly_commitment_end", 19); after();
  };
  poly("comm_comb_ops", comm_ops(c, comm), c.L_ops);
  poly("comm_comb_mem", comm_mem(c, comm), c.L_mem);
}

// ---- NIZK mode (snark.rs:162-287): the two lines in front of R1CSProof::prove / ::verify (:212-213, :252-253).  The digest is the caller's
//      inst.digest as bytes, of any length: it is absorbed, never computed or read ----
template <class Hook = NoHook>
static inline void nizk_prefix(Script& ts, const uint8_t* digest, size_t digest_len, Hook after = Hook()) {
  ts.protocol("Spartan NIZK proof"); after();
  ts.message("R1CSShapeDigest", digest, digest_len); after();
}

// ---- sizes: the layouts the two halves' calls write (include/sbn254.h), laid end to end ----
// R1CSProof alone at a padded shape: sbn_r1cs_proof_sizes' two numbers
static inline void sat_sizes(size_t nv, size_t nx, size_t ny, size_t* rnd, size_t* proof) {
  const size_t ell = log2u(nv), ml = ell / 2, lg = ell - ml, L = (size_t)1 << ml;
  *rnd = L + 8 * nx + 7 * ny + 2 * lg + 17;
  *proof = 32 * (L + 10 * nx + 9 * ny + 20) + 64 * lg + 128;
}
// NIZK: rnd = R1CSProof::prove's draws; proof = r1cs_sat_proof | rx [nx x 32] | ry [ny x 32], the declaration order of snark.rs:191-194
struct NizkSizes { size_t r1cs_proof, rnd_scalars, proof_bytes; };
static inline NizkSizes nizk_sizes(const Shape& s) {
  NizkSizes z;
  sat_sizes(s.nv, s.nx, s.ny, &z.rnd_scalars, &z.r1cs_proof);
  z.proof_bytes = z.r1cs_proof + 32 * (s.nx + s.ny);
  return z;
}
struct Sizes { size_t r1cs_rnd, r1cs_proof, eval_rnd, eval_proof, rnd_scalars, proof_bytes; };
static inline Sizes sizes(const Comm& c, bool kzg) {
  Sizes z;
  sat_sizes((size_t)c.nv, c.nx, c.ny, &z.r1cs_rnd, &z.r1cs_proof);
  const size_t b = (size_t)BATCH, n = log2u((size_t)c.N), m = log2u((size_t)c.cells);
  const size_t e_o = ell_ops((size_t)c.N), e_m = m + 1, e_d = n + log2u(npo2(2 * b));
  const size_t lg_o = e_o - e_o / 2, lg_m = e_m - e_m / 2, lg_d = e_d - e_d / 2, Ld = (size_t)1 << (e_d / 2);
  const size_t common = 32 * (4 + 6 * b) + 64 * (m * (m - 1) + n * (n - 1)) + 256 * (m + b * n) + 192 * b + 32 * (7 * b + 2);
  if (kzg) { z.eval_rnd = 6 + 2 * (lg_o + lg_m); z.eval_proof = 32 + common + 64 * (lg_o + lg_m) + 2 * 128 + 64; }
  else { z.eval_rnd = 9 + 2 * (lg_d + lg_o + lg_m); z.eval_proof = 32 * Ld + common + 64 * (lg_d + lg_o + lg_m) + 3 * 128; }
  z.rnd_scalars = z.r1cs_rnd + z.eval_rnd;
  z.proof_bytes = z.r1cs_proof + 96 + z.eval_proof;
  return z;
}

}  // namespace snark
}  // namespace sbn_host
