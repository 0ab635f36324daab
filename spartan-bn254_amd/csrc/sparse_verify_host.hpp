// sparse_verify_host.hpp — the field and transcript half of SparseMatPolyEvalProof::verify (sparse_mlpoly_full.rs:1815-1845), host only: no HIP, no
// context, no launches; built on proof_host.hpp (Script, fr::) and includable alone, like it.  tests/sparse_verify_host_check.cpp builds this header
// alone, under ASan + UBSan, and tests/test_sparse_verify_host_cpu.py compares it with the literal verifier of tests/sparse_eval_model.py.  abi_sparse_verify.inc (sbn_sparse_eval_verify) is its caller in the library.
//   layout                  the thirteen fields of the proof (include/sbn254.h, sbn_sparse_eval_prove) and the canonical check of every scalar
//   pcepb_verify            ProductCircuitEvalProofBatched::verify (product_tree.rs:394-537) with SumcheckInstanceProof::verify of degree 3 inside
//                           (sumcheck.rs:35-85)
//   product_layer_verify    ProductLayerProof::verify (:1436-1520)
//   hash_layer_field        the field part of HashLayerProof::verify (:1048-1112, :1114-1265): the four hash checks per side, claims_dotp, and the
//                           padded evaluation vectors of the three joint openings (the openings themselves are group work)
// Every function refuses (returns false) where the reference's verifier fails: an assert on a length, a sumcheck round, a layer check, a hash
// check, Scalar::from_bytes on a value >= r.  A refusal leaves the transcript wherever the check stopped: the caller works on a copy.
// Field work is O(b (n^2 + m^2)) products and the hashing about 2 * 10^3 permutations at the keyless shape: host work, all of it.
#pragma once
#include "proof_host.hpp"
#include <vector>

namespace sbn_host {
namespace spv {

using fr::El;

struct Span { const uint8_t* p; size_t n; };      // bytes

static inline size_t log2z(size_t x) { size_t l = 0; while (((size_t)1 << (l + 1)) <= x) l++; return l; }
// Scalar::from_bytes (scalar.rs:87-95): false on a value >= r
static inline bool el_load(const uint8_t* b, El* o) { memcpy(o->v, b, 32); return !fr::geq(o->v); }
static inline bool els_load(const uint8_t* b, size_t n, std::vector<El>* o) {
  o->resize(n);
  for (size_t i = 0; i < n; i++) if (!el_load(b + 32 * i, &(*o)[i])) return false;
  return true;
}
static inline bool el_eq(const El& a, const El& b) { return memcmp(a.v, b.v, 32) == 0; }
static inline El lerp(const El& a, const El& b, const El& r) { return fr::add(a, fr::fmul(r, fr::sub(b, a))); }      // a + r (b - a)

// ---- the layout of the proof (include/sbn254.h): comm_derefs, the ProductLayerProof's five fields, the HashLayerProof's seven ----
enum Field { COMM_DEREFS, PROD_EVAL_ROW, PROD_EVAL_COL, PROD_EVAL_VAL, PROD_PROOF_MEM, PROD_PROOF_OPS,
             HASH_EVAL_ROW, HASH_EVAL_COL, HASH_EVAL_VAL, HASH_EVAL_DEREFS, HASH_PROOF_OPS, HASH_PROOF_MEM, HASH_PROOF_DEREFS, NFIELDS };
struct Layout {
  size_t b, n, m;                                  // batch, log2 N (the layers of an ops circuit), max(nx, ny) (the layers of a mem circuit)
  size_t cnt_d, cnt_o;                             // evals of the derefs / ops joint openings, padded to a power of two
  size_t lg_d, lg_o, lg_m, Ld;                     // rounds of the three openings; row commitments in comm_derefs
  size_t off[NFIELDS + 1];                         // field f lies at [off[f], off[f + 1])
  bool kzg;                                        // the KZG build's layout: comm_derefs one point, proof_derefs [proof 32 | eval 32]
};
static inline size_t pcepb_bytes(size_t circuits, size_t layers, size_t dotp) { return 128 * (layers * (layers - 1) / 2) + 32 * (2 * circuits * layers + 3 * dotp); }
// false where SparseMatPolyCommitmentGens::new or the verifier's first assert would fail: N below 2 or no power of two, no batch, no variable
static inline bool layout_make(size_t nx, size_t ny, size_t N, size_t batch, Layout* L, bool kzg = false) {
  if (batch < 1 || N < 2 || (N & (N - 1)) || nx > 63 || ny > 63 || (nx < 1 && ny < 1)) return false;
  L->kzg = kzg; L->b = batch; L->n = log2z(N); L->m = nx > ny ? nx : ny;
  L->cnt_d = 1; while (L->cnt_d < 2 * batch) L->cnt_d <<= 1;
  L->cnt_o = 1; while (L->cnt_o < 5 * batch) L->cnt_o <<= 1;
  const size_t ell_d = L->n + log2z(L->cnt_d), ell_o = L->n + log2z(L->cnt_o), ell_m = L->m + 1;      // sparse_mlpoly_full.rs:619-623
  L->lg_d = ell_d - ell_d / 2; L->lg_o = ell_o - ell_o / 2; L->lg_m = ell_m - ell_m / 2; L->Ld = (size_t)1 << (ell_d / 2);
  const size_t b = batch;
  const size_t len[NFIELDS] = {kzg ? 32 : 32 * L->Ld, 32 * (2 + 2 * b), 32 * (2 + 2 * b), 64 * b, pcepb_bytes(4, L->m, 0), pcepb_bytes(4 * b, L->n, 2 * b),
                               32 * (2 * b + 1), 32 * (2 * b + 1), 32 * b, 64 * b, 64 * L->lg_o + 128, 64 * L->lg_m + 128, kzg ? 64 : 64 * L->lg_d + 128};
  L->off[0] = 0;
  for (int f = 0; f < NFIELDS; f++) L->off[f + 1] = L->off[f] + len[f];
  return true;
}
static inline Span field(const Layout& L, const uint8_t* proof, Field f) { return Span{proof + L.off[f], L.off[f + 1] - L.off[f]}; }
// every scalar of the proof is below r: the nine scalar fields, and z1, z2 at the end of each opening (the KZG build: of the two Hyrax openings, and
// the eval behind the derefs proof point)
static inline bool proof_scalars_canonical(const Layout& L, const uint8_t* proof) {
  El x;
  for (int f = PROD_EVAL_ROW; f <= HASH_EVAL_DEREFS; f++)
    for (size_t o = L.off[f]; o < L.off[f + 1]; o += 32) if (!el_load(proof + o, &x)) return false;
  if (L.kzg && !el_load(proof + L.off[HASH_PROOF_DEREFS] + 32, &x)) return false;
  for (int f = HASH_PROOF_OPS; f <= (L.kzg ? HASH_PROOF_MEM : HASH_PROOF_DEREFS); f++)
    for (size_t o = L.off[f + 1] - 64; o < L.off[f + 1]; o += 32) if (!el_load(proof + o, &x)) return false;
  return true;
}

// ---- ProductCircuitEvalProofBatched::verify (product_tree.rs:394-537) ----
// proof: the polynomials (layer k: k of 4 coefficients), then per layer claims_prod_left[circuits] ‖ claims_prod_right[circuits], then
// claims_dotp left ‖ right ‖ weight.  `length`: the entries of a circuit's input layer, a power of two.  Out: claims_to_verify, the folded
// dot-product claims (3 per pair), rand.  False: a length the reference asserts, a sumcheck round, a layer check, a scalar >= r.
static inline bool pcepb_verify(Script& ts, Span proof, const std::vector<El>& claims_prod, const std::vector<El>& claims_dotp, size_t length,
                                std::vector<El>* claims_out, std::vector<El>* dotp_out, std::vector<El>* rand_out) {
  using namespace fr;
  if (length == 0 || (length & (length - 1))) return false;
  const size_t layers = log2z(length), n = claims_prod.size(), d = claims_dotp.size();
  if (proof.n != pcepb_bytes(n, layers, d) || (d & 1)) return false;
  const uint8_t* polys = proof.p; const uint8_t* claims = polys + 128 * (layers * (layers - 1) / 2); const uint8_t* dotp = claims + 64 * n * layers;
  const El one = from_u64(1), zero = from_u64(0);
  std::vector<El> cur = claims_prod, rand, dl, dr, dw;
  if (!els_load(dotp, d, &dl) || !els_load(dotp + 32 * d, d, &dr) || !els_load(dotp + 64 * d, d, &dw)) return false;
  dotp_out->clear();
  size_t po = 0;
  for (size_t i = 0; i < layers; i++) {
    const bool last = i + 1 == layers;
    if (last) cur.insert(cur.end(), claims_dotp.begin(), claims_dotp.end());                   // product_tree.rs:410
    std::vector<uint8_t> cb(32 * cur.size());
    ts.challenges("rand_coeffs_next_layer", cb.data(), cur.size());                            // :415
    std::vector<El> coeffs;
    if (!els_load(cb.data(), cur.size(), &coeffs)) return false;
    El e = zero;
    for (size_t k = 0; k < cur.size(); k++) e = add(e, fmul(cur[k], coeffs[k]));
    std::vector<El> rand_prod;
    for (size_t j = 0; j < i; j++) {                                                           // SumcheckInstanceProof::verify, sumcheck.rs:35-85
      const uint8_t* cp = polys + 128 * (po + j);
      El co[4];
      for (int k = 0; k < 4; k++) if (!el_load(cp + 32 * k, &co[k])) return false;
      if (!el_eq(add(add(add(co[0], co[0]), co[1]), add(co[2], co[3])), e)) return false;      // poly(0) + poly(1) == e  (:62-66)
      ts.message("poly", "UniPoly_begin", 13);                                                 // unipoly.rs:118-122
      ts.scalars("coeff", cp, 4);
      ts.message("poly", "UniPoly_end", 11);
      uint8_t rb[32]; El r;
      ts.challenge("challenge_nextround", rb);
      if (!el_load(rb, &r)) return false;
      rand_prod.push_back(r);
      e = add(co[0], fmul(r, add(co[1], fmul(r, add(co[2], fmul(r, co[3]))))));
    }
    po += i;
    std::vector<El> lefts, rights;
    if (!els_load(claims + 64 * n * i, n, &lefts) || !els_load(claims + 64 * n * i + 32 * n, n, &rights)) return false;
    for (size_t k = 0; k < n; k++) { ts.scalar("claim_prod_left", claims + 64 * n * i + 32 * k); ts.scalar("claim_prod_right", claims + 64 * n * i + 32 * (n + k)); }
    El eq = one;                                                                               // :435
    for (size_t k = 0; k < rand.size(); k++) eq = fmul(eq, add(fmul(rand[k], rand_prod[k]), fmul(sub(one, rand[k]), sub(one, rand_prod[k]))));
    El expected = zero;
    for (size_t k = 0; k < n; k++) expected = add(expected, fmul(fmul(coeffs[k], eq), fmul(lefts[k], rights[k])));
    if (last)                                                                                  // :447-453
      for (size_t k = 0; k < d; k++) {
        ts.scalar("claim_dotp_left", dotp + 32 * k); ts.scalar("claim_dotp_right", dotp + 32 * (d + k)); ts.scalar("claim_dotp_weight", dotp + 32 * (2 * d + k));
        expected = add(expected, fmul(fmul(coeffs[n + k], dl[k]), fmul(dr[k], dw[k])));
      }
    if (!el_eq(expected, e)) return false;                                                     // :506
    uint8_t lb[32]; El r_layer;
    ts.challenge("challenge_r_layer", lb);
    if (!el_load(lb, &r_layer)) return false;
    cur.resize(n);
    for (size_t k = 0; k < n; k++) cur[k] = lerp(lefts[k], rights[k], r_layer);
    if (last)                                                                                  // :516-530
      for (size_t k = 0; k < d / 2; k++) { dotp_out->push_back(lerp(dl[2 * k], dl[2 * k + 1], r_layer)); dotp_out->push_back(lerp(dr[2 * k], dr[2 * k + 1], r_layer)); dotp_out->push_back(lerp(dw[2 * k], dw[2 * k + 1], r_layer)); }
    rand.assign(1, r_layer); rand.insert(rand.end(), rand_prod.begin(), rand_prod.end());                      // :532-533
  }
  *claims_out = cur; *rand_out = rand;
  return true;
}

// ---- ProductLayerProof::verify (:1436-1520) ----
struct ProductFields { Span eval_row, eval_col, eval_val, proof_mem, proof_ops; };
struct ProductClaims { std::vector<El> claims_mem, rand_mem, claims_ops, claims_dotp, rand_ops; };
// evals: b canonical scalars (the caller's).  False: a field of the wrong length, init * prod write != prod read * audit on a side,
// eval_dotp_left + eval_dotp_right != evals[i], either batched product proof
static inline bool product_layer_verify(Script& ts, const ProductFields& f, size_t num_ops, size_t num_cells, const uint8_t* evals, size_t b, ProductClaims* out) {
  using namespace fr;
  ts.protocol("Sparse polynomial product layer proof");
  if (b < 1 || f.eval_row.n != 32 * (2 + 2 * b) || f.eval_col.n != 32 * (2 + 2 * b) || f.eval_val.n != 64 * b) return false;
  std::vector<El> side[2], ev, want;
  static const char* const lab[2][4] = {{"claim_row_eval_init", "claim_row_eval_read", "claim_row_eval_write", "claim_row_eval_audit"},
                                        {"claim_col_eval_init", "claim_col_eval_read", "claim_col_eval_write", "claim_col_eval_audit"}};
  for (int s = 0; s < 2; s++) {
    const uint8_t* p = s ? f.eval_col.p : f.eval_row.p;                                        // init, read[b], write[b], audit
    if (!els_load(p, 2 + 2 * b, &side[s])) return false;
    El w = side[s][0], r = side[s][1 + 2 * b];
    for (size_t k = 0; k < b; k++) { r = fmul(r, side[s][1 + k]); w = fmul(w, side[s][1 + b + k]); }
    if (!el_eq(w, r)) return false;                                                            // :1454-1460, :1468-1474
    ts.scalar(lab[s][0], p); ts.scalars(lab[s][1], p + 32, b); ts.scalars(lab[s][2], p + 32 * (1 + b), b); ts.scalar(lab[s][3], p + 32 * (1 + 2 * b));
  }
  if (!els_load(f.eval_val.p, 2 * b, &ev) || !els_load(evals, b, &want)) return false;        // lefts[b], rights[b]
  std::vector<El> dotp_circuit, ops_in, mem_in, none;
  for (size_t i = 0; i < b; i++) {
    if (!el_eq(add(ev[i], ev[b + i]), want[i])) return false;                                  // :1482-1487
    ts.scalar("claim_eval_dotp_left", f.eval_val.p + 32 * i); ts.scalar("claim_eval_dotp_right", f.eval_val.p + 32 * (b + i));
    dotp_circuit.push_back(ev[i]); dotp_circuit.push_back(ev[b + i]);
  }
  for (int s = 0; s < 2; s++) ops_in.insert(ops_in.end(), side[s].begin() + 1, side[s].begin() + 1 + 2 * b);      // row read, row write, col read, col write
  for (int s = 0; s < 2; s++) { mem_in.push_back(side[s][0]); mem_in.push_back(side[s][1 + 2 * b]); }            // row init, row audit, col init, col audit
  if (!pcepb_verify(ts, f.proof_ops, ops_in, dotp_circuit, num_ops, &out->claims_ops, &out->claims_dotp, &out->rand_ops)) return false;
  std::vector<El> no_dotp;
  return pcepb_verify(ts, f.proof_mem, mem_in, none, num_cells, &out->claims_mem, &no_dotp, &out->rand_mem);
}

// ---- the field part of HashLayerProof::verify (:1048-1112, :1114-1265) ----
struct HashFields { Span eval_row, eval_col, eval_val, eval_derefs; };
struct JointEvals { std::vector<uint8_t> derefs, ops, mem; };      // the evaluation vectors the three openings reduce, padded with zeros to a power of two
static inline El hash_func(const El& addr, const El& val, const El& ts_, const El& r_hash) { return fr::add(fr::add(fr::fmul(ts_, fr::fmul(r_hash, r_hash)), fr::fmul(val, r_hash)), addr); }
// rx, ry: the equalized points, m = rand_mem.size() scalars each.  False: a field or a claims vector of the wrong length, any of the four hash
// checks of a side, claims_dotp against eval_derefs / eval_val
static inline bool hash_layer_field(const HashFields& f, size_t b, const ProductClaims& pc, const El* rx, const El* ry, const El& r_hash, const El& r_multiset, JointEvals* out) {
  using namespace fr;
  const size_t m = pc.rand_mem.size();
  if (b < 1 || f.eval_row.n != 32 * (2 * b + 1) || f.eval_col.n != 32 * (2 * b + 1) || f.eval_val.n != 32 * b || f.eval_derefs.n != 64 * b) return false;
  if (pc.claims_mem.size() != 4 || pc.claims_ops.size() != 4 * b || pc.claims_dotp.size() != 3 * b) return false;      // :1612-1613, :1188
  std::vector<El> dv, val, sv[2];
  if (!els_load(f.eval_derefs.p, 2 * b, &dv) || !els_load(f.eval_val.p, b, &val)) return false;                         // eval_row_ops_val[b], eval_col_ops_val[b]
  if (!els_load(f.eval_row.p, 2 * b + 1, &sv[0]) || !els_load(f.eval_col.p, 2 * b + 1, &sv[1])) return false;           // addr[b], read_ts[b], audit_ts
  const El one = from_u64(1), zero = from_u64(0);
  El id = zero;                                                                                 // IdentityPolynomial::evaluate (:1278-1285)
  for (size_t j = 0; j < m; j++) id = add(add(id, id), pc.rand_mem[j]);
  for (int s = 0; s < 2; s++) {                                                                 // verify_helper (:1048-1112)
    const El* r = s ? ry : rx;
    El eqv = one;                                                                               // EqPolynomial::new(r).evaluate(rand_mem)
    for (size_t j = 0; j < m; j++) eqv = fmul(eqv, add(fmul(r[j], pc.rand_mem[j]), fmul(sub(one, r[j]), sub(one, pc.rand_mem[j]))));
    const El& c_init = pc.claims_mem[2 * s]; const El& c_audit = pc.claims_mem[2 * s + 1];
    if (!el_eq(c_init, sub(hash_func(id, eqv, zero, r_hash), r_multiset))) return false;
    if (!el_eq(c_audit, sub(hash_func(id, eqv, sv[s][2 * b], r_hash), r_multiset))) return false;
    for (size_t i = 0; i < b; i++) {
      const El& addr = sv[s][i]; const El& rts = sv[s][b + i]; const El& v = dv[b * s + i];
      if (!el_eq(pc.claims_ops[2 * b * s + i], sub(hash_func(addr, v, rts, r_hash), r_multiset))) return false;
      if (!el_eq(pc.claims_ops[2 * b * s + b + i], sub(hash_func(addr, v, add(rts, one), r_hash), r_multiset))) return false;
    }
  }
  for (size_t i = 0; i < b; i++)                                                                // :1188-1194
    if (!el_eq(pc.claims_dotp[3 * i], dv[i]) || !el_eq(pc.claims_dotp[3 * i + 1], dv[b + i]) || !el_eq(pc.claims_dotp[3 * i + 2], val[i])) return false;
  size_t cnt_d = 1, cnt_o = 1;
  while (cnt_d < 2 * b) cnt_d <<= 1;
  while (cnt_o < 5 * b) cnt_o <<= 1;
  out->derefs.assign(32 * cnt_d, 0); memcpy(out->derefs.data(), f.eval_derefs.p, 64 * b);       // :471
  out->ops.assign(32 * cnt_o, 0);                                                               // row addr, row read_ts, col addr, col read_ts, val  (:1215-1222)
  memcpy(out->ops.data(), f.eval_row.p, 64 * b); memcpy(out->ops.data() + 64 * b, f.eval_col.p, 64 * b); memcpy(out->ops.data() + 128 * b, f.eval_val.p, 32 * b);
  out->mem.assign(64, 0);                                                                       // row audit_ts, col audit_ts  (:1244-1245)
  memcpy(out->mem.data(), f.eval_row.p + 64 * b, 32); memcpy(out->mem.data() + 32, f.eval_col.p + 64 * b, 32);
  return true;
}

}  // namespace spv
}  // namespace sbn_host
