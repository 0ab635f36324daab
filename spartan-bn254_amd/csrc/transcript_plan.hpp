// transcript_plan.hpp — the host's plans of the device transcript steps (transcript_kernels.cuh) and the layout of what they hand over.
// Host code only: the host's own Strobe code (host_strobe.hpp) run with StrobePlan as its permutation, and the C ABI's error codes.
//
// The contract between a plan and the step that executes it.  A step's STROBE bookkeeping (operation headers, lengths, labels, run_f's
// padding, where the blocks end) depends on the phase (pos, pos_begin) alone, never on a value, so it is planned here, per block:
//   k_tr_sumcheck_step   one 200-byte XOR mask per block (transcript_plan_round).  The four coefficients' bytes are placed by the step itself
//                        from the constants below: coefficient k's byte o sits TR_COEFF_FIRST + TR_COEFF_STRIDE k + o bytes behind pos0 in the
//                        round's stream, block = that offset / TR_RATE.  The 64 challenge bytes are read and cleared behind the last block.
//   k_tr_layer_step      one record of TR_REC_BYTES per block (transcript_plan_boundary): the 200-byte XOR mask; at TR_REC_FLAGS a 64-bit word,
//                        1 when a 64-byte challenge is read and cleared behind this block's permutation, else 0; at TR_REC_SRC 168 16-bit
//                        indices, one per rate byte (the last two unused): the data byte XORed there, or 0xffff.
// tests/transcript_plan_check.cpp executes both plans in plain C++ against the literal operation sequence, at every phase and shape.
#pragma once
#include "../../include/sbn254.h"
#include "host_strobe.hpp"

namespace sbn {

constexpr int TR_RATE = 166;                 // STROBE-128
constexpr int TR_ROUND_STREAM = 255;         // bytes one sumcheck round absorbs ahead of the PRF's permutation
constexpr int TR_COEFF_FIRST = 38;           // offset of the first coefficient's 32 bytes in that stream: 25 ("poly" / "UniPoly_begin") + 13
constexpr int TR_COEFF_STRIDE = 45;          // 2 + 5 + 4 + 2 + 32 per "coeff" message

constexpr int TR_REC_BYTES = 544;            // 200 mask, 8 flags, 168 x 2 byte sources
constexpr int TR_REC_FLAGS = 200, TR_REC_SRC = 208;

}  // namespace sbn

// One sumcheck round's seven transcript operations (unipoly.rs:117-122 + challenge_scalar("challenge_nextround")) from the phase
// (pos, pos_begin): the XOR mask of every block the round completes (200 bytes each; labels, lengths, operation headers, padding),
// coefficient bytes left zero.  The round ends behind the PRF's 64 bytes: pos = 64, pos_begin = 0, cur_flags = I|A|C.
static void transcript_plan_round(uint8_t pos, uint8_t pos_begin, uint8_t cur_flags, std::vector<uint8_t>& masks, uint8_t end[3]) {
  sbn_host::MerlinTranscriptT<sbn_host::StrobePlan> p;
  memset(p.s.st, 0, sizeof p.s.st);
  p.s.pos = pos; p.s.pos_begin = pos_begin; p.s.cur_flags = cur_flags;
  masks.clear(); p.s.perm.blocks = &masks;
  const uint8_t zero[32] = {0};
  uint8_t out[64];
  p.append_message((const uint8_t*)"poly", 4, (const uint8_t*)"UniPoly_begin", 13);
  for (int k = 0; k < 4; k++) p.append_message((const uint8_t*)"coeff", 5, zero, 32);
  p.append_message((const uint8_t*)"poly", 4, (const uint8_t*)"UniPoly_end", 11);
  p.challenge_bytes((const uint8_t*)"challenge_nextround", 19, out, 64);
  end[0] = p.s.pos; end[1] = p.s.pos_begin; end[2] = p.s.cur_flags;
}

// One boundary's transcript work from the phase (pos, pos_begin, cur_flags): the records k_tr_layer_step executes.
//   close (n_close > 0): append_scalar("claim_prod_left" / "claim_prod_right") per circuit, ("claim_dotp_left" / "_right" / "_weight") per
//   dot-product circuit (product_tree.rs:352-365; append_scalar = append_message of the 32 canonical bytes, transcript.rs:28-32), then
//   challenge_scalar("challenge_r_layer"); open: n_open x challenge_scalar("rand_coeffs_next_layer") (challenge_vector, transcript.rs:69-73).
// The appended values are the closing layer's final claims in the order of sbn_sumcheck_finish: data index = table index.
static int transcript_plan_boundary(uint8_t pos, uint8_t pos_begin, uint8_t cur_flags, size_t n_close, size_t n_dotp_close, size_t n_open, std::vector<uint8_t>& recs, uint8_t end[3]) {
  using namespace sbn;
  using S = sbn_host::StrobeT<sbn_host::StrobePlan>;
  sbn_host::MerlinTranscriptT<sbn_host::StrobePlan> p;
  memset(p.s.st, 0, sizeof p.s.st);
  p.s.pos = pos; p.s.pos_begin = pos_begin; p.s.cur_flags = cur_flags;
  std::vector<uint8_t> masks; p.s.perm.blocks = &masks;
  struct Put { size_t lin; size_t table; };
  std::vector<Put> puts; std::vector<size_t> chal;
  const uint8_t zero[32] = {0}; const uint8_t n32[4] = {32, 0, 0, 0};
  auto append = [&](const char* label, size_t table) {
    p.s.meta_ad((const uint8_t*)label, strlen(label), false); p.s.meta_ad(n32, 4, true);
    p.s.begin_op(S::FLAG_A, false);                                   // ad's header; the 32 bytes follow from here
    puts.push_back({masks.size() / 200 * (size_t)S::RATE + p.s.pos, table});
    p.s.absorb(zero, 32);
  };
  auto challenge = [&](const char* label) {
    uint8_t out[64];
    p.challenge_bytes((const uint8_t*)label, strlen(label), out, 64);
    chal.push_back(masks.size() / 200);                               // blocks completed when the 64 bytes are read
    return p.s.pos == 64 && masks.size() >= 200;
  };
  bool ok = true;
  if (n_close) {
    for (size_t i = 0; i < n_close; i++) { append("claim_prod_left", i); append("claim_prod_right", n_close + i); }
    const size_t o = 2 * n_close + 1;
    for (size_t k = 0; k < n_dotp_close; k++) { append("claim_dotp_left", o + k); append("claim_dotp_right", o + n_dotp_close + k); append("claim_dotp_weight", o + 2 * n_dotp_close + k); }
    ok = challenge("challenge_r_layer") && ok;
  }
  for (size_t i = 0; i < n_open; i++) ok = challenge("rand_coeffs_next_layer") && ok;
  const size_t nblk = masks.size() / 200;
  for (size_t k = 0; k < chal.size(); k++) if (chal[k] == 0 || chal[k] > nblk || (k && chal[k] <= chal[k - 1])) ok = false;   // one challenge per block at most, each behind a permutation of this step
  if (!ok || chal.empty() || chal.back() != nblk) return SBN_EINVAL;
  recs.assign(nblk * (size_t)TR_REC_BYTES, 0);
  for (size_t b = 0; b < nblk; b++) {
    uint8_t* rec = recs.data() + b * TR_REC_BYTES;
    memcpy(rec, masks.data() + 200 * b, 200);
    memset(rec + TR_REC_SRC, 0xff, 336);
  }
  for (size_t b : chal) recs[(b - 1) * TR_REC_BYTES + TR_REC_FLAGS] = 1;
  for (const Put& q : puts)
    for (size_t o = 0; o < 32; o++) {
      const size_t lin = q.lin + o, b = lin / S::RATE, at = lin % S::RATE;
      if (b >= nblk) return SBN_EINVAL;
      const uint16_t idx = (uint16_t)(32 * q.table + o);
      memcpy(recs.data() + b * TR_REC_BYTES + TR_REC_SRC + 2 * at, &idx, 2);
    }
  end[0] = p.s.pos; end[1] = p.s.pos_begin; end[2] = p.s.cur_flags;
  return SBN_OK;
}
