// The plans of the device transcript steps (csrc/transcript_plan.hpp) as a stand-alone program: one case per line of stdin, one line of results
// per case.  tests/test_transcript_plan_cpu.py builds it under ASan + UBSan and sweeps every STROBE phase and every boundary shape.
// Each case plans a step, executes the plan in plain C++ the way the kernels of csrc/transcript_kernels.cuh consume it, and compares with
// MerlinTranscript (csrc/host_strobe.hpp) running the literal operation sequence on the same starting state and the same random bytes: every
// challenge's 64 bytes, the 200 sponge bytes at the end, and end[3].  All arguments are decimal.
//   round POS POS_BEGIN FLAGS SEED                         -> OK nblk end0 end1 end2            (k_tr_sumcheck_step's transcript part)
//   bound POS POS_BEGIN FLAGS N_CLOSE N_DOTP N_OPEN SEED   -> OK nblk end0 end1 end2 nchal nsrc (k_tr_layer_step's sponge; nsrc = source bytes placed)
// A case that does not hold prints FAIL and the reason, and the program's exit status is 1.
#include "../spartan-bn254_amd/csrc/transcript_plan.hpp"
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

using namespace sbn_host;
using sbn::TR_COEFF_FIRST; using sbn::TR_COEFF_STRIDE; using sbn::TR_RATE; using sbn::TR_REC_BYTES; using sbn::TR_REC_FLAGS; using sbn::TR_REC_SRC; using sbn::TR_ROUND_STREAM;

static_assert(TR_RATE == Strobe128::RATE, "the device's rate is STROBE-128's");
static_assert(TR_REC_FLAGS == 200 && TR_REC_SRC == TR_REC_FLAGS + 8 && TR_REC_BYTES == TR_REC_SRC + 2 * 168, "mask, flag word, 168 sources");
static_assert(TR_REC_BYTES % 16 == 0 && TR_REC_SRC % 16 == 0 && TR_REC_FLAGS % 8 == 0, "the step loads the sources 16 bytes and the flags 8 bytes at a time");

struct Rng {                                            // splitmix64: the cases' random bytes
  uint64_t s;
  uint64_t next() { uint64_t z = (s += 0x9e3779b97f4a7c15ull); z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull; z = (z ^ (z >> 27)) * 0x94d049bb133111ebull; return z ^ (z >> 31); }
  void fill(uint8_t* p, size_t n) { for (size_t i = 0; i < n; i++) p[i] = (uint8_t)(next() >> 32); }
};

static MerlinTranscript start(Rng& rng, size_t pos, size_t pos_begin, size_t flags) {
  MerlinTranscript t;
  rng.fill(t.s.st, 200);
  t.s.pos = (uint8_t)pos; t.s.pos_begin = (uint8_t)pos_begin; t.s.cur_flags = (uint8_t)flags;
  return t;
}
static void read_and_clear(uint8_t* st, uint8_t out[64]) { memcpy(out, st, 64); memset(st, 0, 64); }
static bool same_end(const MerlinTranscript& t, const uint8_t* st, const uint8_t end[3], std::string& why) {
  if (memcmp(t.s.st, st, 200)) { why = "the 200 sponge bytes differ at the end"; return false; }
  if (t.s.pos != end[0] || t.s.pos_begin != end[1] || t.s.cur_flags != end[2]) { why = "end[3] is not the transcript's pos, pos_begin, cur_flags"; return false; }
  return true;
}

// k_tr_sumcheck_step, part 3: per block mask ^ coefficient bytes placed from pos0 by the constants, Keccak-f; the challenge behind the last block
static bool round_case(size_t pos, size_t pos_begin, size_t flags, uint64_t seed, std::string& out) {
  Rng rng{seed};
  MerlinTranscript t = start(rng, pos, pos_begin, flags);
  uint8_t st[200]; memcpy(st, t.s.st, 200);
  uint8_t cb[128]; rng.fill(cb, 128);
  std::vector<uint8_t> masks; uint8_t end[3];
  transcript_plan_round((uint8_t)pos, (uint8_t)pos_begin, (uint8_t)flags, masks, end);
  const size_t nblk = masks.size() / 200;
  if (masks.size() % 200 || nblk < 1) { out = "no whole block"; return false; }
  if (nblk > 3) { out = "a round of more than 3 blocks"; return false; }
  size_t placed = 0;
  for (size_t b = 0; b < nblk; b++) {
    for (int i = 0; i < 200; i++) st[i] ^= masks[200 * b + i];
    for (int p = 0; p < TR_RATE; p++) {
      const int tt = TR_RATE * (int)b + p - (int)pos - TR_COEFF_FIRST;
      const int k = tt / TR_COEFF_STRIDE, o = tt - k * TR_COEFF_STRIDE;
      if (tt >= 0 && k < 4 && o < 32) { st[p] ^= cb[32 * k + o]; placed++; }
    }
    KeccakPerm::keccak_f(st);
  }
  if (placed != 128) { out = "not every coefficient byte falls into the round's blocks"; return false; }
  if ((pos + TR_ROUND_STREAM + TR_RATE - 1) / TR_RATE != nblk) { out = "TR_ROUND_STREAM bytes from pos do not end in the last block"; return false; }
  uint8_t got[64]; read_and_clear(st, got);

  t.append_message((const uint8_t*)"poly", 4, (const uint8_t*)"UniPoly_begin", 13);
  for (int k = 0; k < 4; k++) t.append_message((const uint8_t*)"coeff", 5, cb + 32 * k, 32);
  t.append_message((const uint8_t*)"poly", 4, (const uint8_t*)"UniPoly_end", 11);
  uint8_t want[64]; t.challenge_bytes((const uint8_t*)"challenge_nextround", 19, want, 64);
  if (memcmp(got, want, 64)) { out = "the challenge's 64 bytes differ"; return false; }
  if (!same_end(t, st, end, out)) return false;
  std::ostringstream o; o << "OK " << nblk << " " << (int)end[0] << " " << (int)end[1] << " " << (int)end[2];
  out = o.str();
  return true;
}

// k_tr_layer_step, part 1: per block mask ^ data[idx] at every rate byte with a source, Keccak-f, and where the flag is set a challenge
static bool bound_case(size_t pos, size_t pos_begin, size_t flags, size_t n_close, size_t n_dotp, size_t n_open, uint64_t seed, std::string& out) {
  Rng rng{seed};
  MerlinTranscript t = start(rng, pos, pos_begin, flags);
  uint8_t st[200]; memcpy(st, t.s.st, 200);
  const size_t ndata = n_close ? 2 * n_close + 1 + 3 * n_dotp : 0;         // the closing layer's final claims, the shared eq table's among them
  std::vector<uint8_t> data(32 * ndata); rng.fill(data.data(), data.size());
  std::vector<uint8_t> recs; uint8_t end[3];
  if (transcript_plan_boundary((uint8_t)pos, (uint8_t)pos_begin, (uint8_t)flags, n_close, n_dotp, n_open, recs, end) != SBN_OK) { out = "the planner refused"; return false; }
  const size_t nblk = recs.size() / TR_REC_BYTES;
  if (recs.size() % TR_REC_BYTES || nblk < 1) { out = "no whole record"; return false; }
  std::vector<std::vector<uint8_t>> got;
  std::vector<uint8_t> used(data.size(), 0);
  size_t nsrc = 0;
  for (size_t b = 0; b < nblk; b++) {
    const uint8_t* rec = recs.data() + b * TR_REC_BYTES;
    for (int i = 0; i < 200; i++) st[i] ^= rec[i];
    for (int at = 0; at < 168; at++) {
      uint16_t idx; memcpy(&idx, rec + TR_REC_SRC + 2 * at, 2);
      if (idx == 0xffff) continue;
      if (at >= TR_RATE) { out = "a source behind the rate"; return false; }
      if (idx >= 32 * ndata) { out = "a source index reaches 32 * ndata"; return false; }
      if (used[idx]++) { out = "a data byte placed twice"; return false; }
      st[at] ^= data[idx]; nsrc++;
    }
    KeccakPerm::keccak_f(st);
    uint64_t fl; memcpy(&fl, rec + TR_REC_FLAGS, 8);
    if (fl > 1) { out = "a flag word that is neither 0 nor 1 (two flags in one block)"; return false; }
    if (fl) { got.emplace_back(64); read_and_clear(st, got.back().data()); }
  }
  { uint64_t fl; memcpy(&fl, recs.data() + (nblk - 1) * TR_REC_BYTES + TR_REC_FLAGS, 8); if (!fl) { out = "the last block reads no challenge"; return false; } }

  std::vector<std::vector<uint8_t>> want;
  auto app = [&](const char* label, size_t table) { t.append_message((const uint8_t*)label, strlen(label), data.data() + 32 * table, 32); };
  auto chal = [&](const char* label) { want.emplace_back(64); t.challenge_bytes((const uint8_t*)label, strlen(label), want.back().data(), 64); };
  if (n_close) {
    for (size_t i = 0; i < n_close; i++) { app("claim_prod_left", i); app("claim_prod_right", n_close + i); }
    const size_t o = 2 * n_close + 1;
    for (size_t k = 0; k < n_dotp; k++) { app("claim_dotp_left", o + k); app("claim_dotp_right", o + n_dotp + k); app("claim_dotp_weight", o + 2 * n_dotp + k); }
    chal("challenge_r_layer");
  }
  for (size_t i = 0; i < n_open; i++) chal("rand_coeffs_next_layer");
  if (got.size() != want.size()) { out = "flags: " + std::to_string(got.size()) + " challenges read, " + std::to_string(want.size()) + " drawn"; return false; }
  for (size_t k = 0; k < want.size(); k++) if (got[k] != want[k]) { out = "challenge " + std::to_string(k) + ": the 64 bytes differ"; return false; }
  if (nsrc != 32 * (ndata ? ndata - 1 : 0)) { out = "not every appended byte has a source"; return false; }
  if (!same_end(t, st, end, out)) return false;
  std::ostringstream o; o << "OK " << nblk << " " << (int)end[0] << " " << (int)end[1] << " " << (int)end[2] << " " << got.size() << " " << nsrc;
  out = o.str();
  return true;
}

int main() {
  std::string line;
  bool all = true;
  while (std::getline(std::cin, line)) {
    std::istringstream in(line);
    std::string cmd; in >> cmd;
    auto count = [&]() { uint64_t n = 0; if (!(in >> n)) { fprintf(stderr, "bad case: %s\n", line.c_str()); exit(2); } return n; };
    std::string out; bool ok;
    if (cmd == "round") {
      const size_t pos = count(), pb = count(), fl = count(); const uint64_t seed = count();
      if (pos >= (size_t)TR_RATE || pb > pos) { fprintf(stderr, "bad phase: %s\n", line.c_str()); return 2; }
      ok = round_case(pos, pb, fl, seed, out);
    } else if (cmd == "bound") {
      const size_t pos = count(), pb = count(), fl = count(), nc = count(), nd = count(), no = count(); const uint64_t seed = count();
      if (pos >= (size_t)TR_RATE || pb > pos || (!nc && (nd || !no))) { fprintf(stderr, "bad case: %s\n", line.c_str()); return 2; }
      ok = bound_case(pos, pb, fl, nc, nd, no, seed, out);
    } else { fprintf(stderr, "unknown case: %s\n", line.c_str()); return 2; }
    if (!ok) { all = false; out = "FAIL " + out; }
    puts(out.c_str());
  }
  puts("TRANSCRIPT PLAN CHECK DONE");
  return all ? 0 : 1;
}
