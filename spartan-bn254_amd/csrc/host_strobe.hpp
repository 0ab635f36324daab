// host_strobe.hpp — STROBE-128 over Keccak-f[1600] and the Merlin v1.0 transcript built on it (merlin::Transcript as the
// reference uses it: src/transcript.rs, unipoly.rs:117-122).  Host-only, no device needed.  Written from the public Merlin and
// STROBE specifications; the device mirror is transcript_kernels.cuh, the checker tests/transcript_model.py.
// The whole state is 203 bytes: the 200 sponge bytes, then pos, pos_begin, cur_flags — the record both sides exchange.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>
#include <vector>

namespace sbn_host {

// Perm: what run_f does with the 200 bytes.  KeccakPerm is the transcript; StrobePlan (below) records the block instead.
struct KeccakPerm;
template <class Perm>
struct StrobeT {
  static constexpr int RATE = 166;                         // 200 - 128 / 4 - 2
  enum : uint8_t { FLAG_I = 1, FLAG_A = 2, FLAG_C = 4, FLAG_T = 8, FLAG_M = 16, FLAG_K = 32 };
  uint8_t st[200];
  uint8_t pos, pos_begin, cur_flags;
  Perm perm;

  void init(const uint8_t* protocol, size_t len) {
    memset(st, 0, sizeof st);
    const uint8_t head[6] = {1, RATE + 2, 1, 0, 1, 96};
    memcpy(st, head, 6); memcpy(st + 6, "STROBEv1.0.2", 12);
    perm(st);
    pos = pos_begin = cur_flags = 0;
    meta_ad(protocol, len, false);
  }
  void run_f() { st[pos] ^= pos_begin; st[pos + 1] ^= 0x04; st[RATE + 1] ^= 0x80; perm(st); pos = pos_begin = 0; }
  void absorb(const uint8_t* d, size_t n) { for (size_t i = 0; i < n; i++) { st[pos++] ^= d[i]; if (pos == RATE) run_f(); } }
  void squeeze(uint8_t* d, size_t n) { for (size_t i = 0; i < n; i++) { d[i] = st[pos]; st[pos++] = 0; if (pos == RATE) run_f(); } }
  void begin_op(uint8_t flags, bool more) {
    if (more) return;                                     // continues the running operation (callers pass the same flags)
    const uint8_t hdr[2] = {pos_begin, flags};
    pos_begin = (uint8_t)(pos + 1); cur_flags = flags;
    absorb(hdr, 2);
    if ((flags & (FLAG_C | FLAG_K)) && pos != 0) run_f();
  }
  void meta_ad(const uint8_t* d, size_t n, bool more) { begin_op(FLAG_M | FLAG_A, more); absorb(d, n); }
  void ad(const uint8_t* d, size_t n, bool more) { begin_op(FLAG_A, more); absorb(d, n); }
  void prf(uint8_t* d, size_t n, bool more) { begin_op(FLAG_I | FLAG_A | FLAG_C, more); squeeze(d, n); }
};

struct KeccakPerm {
  void operator()(uint8_t* s) const { keccak_f(s); }
  static uint64_t rol(uint64_t x, int n) { n &= 63; return n ? (x << n) | (x >> (64 - n)) : x; }
  static void keccak_f(uint8_t s[200]) {
    // rho offsets, the pi walk and the round constants from their defining recurrences (FIPS 202 3.2), once
    struct Tab { int rho[25]; int pi[25]; uint64_t rc[24]; };
    static const Tab T = [] {
      Tab t;
      for (int i = 0; i < 25; i++) { t.rho[i] = 0; t.pi[i] = i; }
      int x = 1, y = 0;
      for (int k = 0; k < 24; k++) { t.rho[x + 5 * y] = ((k + 1) * (k + 2) / 2) % 64; const int nx = y, ny = (2 * x + 3 * y) % 5; x = nx; y = ny; }
      for (int xx = 0; xx < 5; xx++) for (int yy = 0; yy < 5; yy++) t.pi[yy + 5 * ((2 * xx + 3 * yy) % 5)] = xx + 5 * yy;    // dest <- src
      uint8_t lfsr = 1;
      for (int r = 0; r < 24; r++) {
        uint64_t c = 0;
        for (int j = 0; j < 7; j++) { if (lfsr & 1) c |= (uint64_t)1 << ((1 << j) - 1); lfsr = (uint8_t)((lfsr << 1) ^ ((lfsr & 0x80) ? 0x71 : 0)); }
        t.rc[r] = c;
      }
      return t;
    }();
    uint64_t a[25];
    for (int i = 0; i < 25; i++) { a[i] = 0; for (int b = 0; b < 8; b++) a[i] |= (uint64_t)s[8 * i + b] << (8 * b); }
    for (int r = 0; r < 24; r++) {
      uint64_t C[5], D[5], B[25];
      for (int x = 0; x < 5; x++) C[x] = a[x] ^ a[x + 5] ^ a[x + 10] ^ a[x + 15] ^ a[x + 20];
      for (int x = 0; x < 5; x++) D[x] = C[(x + 4) % 5] ^ rol(C[(x + 1) % 5], 1);
      for (int i = 0; i < 25; i++) a[i] ^= D[i % 5];
      for (int i = 0; i < 25; i++) B[i] = rol(a[T.pi[i]], T.rho[T.pi[i]]);
      for (int y = 0; y < 5; y++) for (int x = 0; x < 5; x++) a[x + 5 * y] = B[x + 5 * y] ^ (~B[(x + 1) % 5 + 5 * y] & B[(x + 2) % 5 + 5 * y]);
      a[0] ^= T.rc[r];
    }
    for (int i = 0; i < 25; i++) for (int b = 0; b < 8; b++) s[8 * i + b] = (uint8_t)(a[i] >> (8 * b));
  }
};
// the planner's permutation: hands the finished block (everything XORed in since the last one, run_f's padding included) to the
// list and starts the next from zero.  Run on a zeroed state with zero bytes for the values, the transcript code above then
// yields exactly the XOR masks a device step applies (transcript_kernels.cuh): its bookkeeping never reads the state.
struct StrobePlan {
  std::vector<uint8_t>* blocks = nullptr;
  void operator()(uint8_t* s) const { blocks->insert(blocks->end(), s, s + 200); memset(s, 0, 200); }
};
using Strobe128 = StrobeT<KeccakPerm>;

template <class Perm>
struct MerlinTranscriptT {
  StrobeT<Perm> s;
  void init(const uint8_t* label, size_t len) {
    s.init((const uint8_t*)"Merlin v1.0", 11);
    append_message((const uint8_t*)"dom-sep", 7, label, len);
  }
  static void le32(uint32_t n, uint8_t b[4]) { b[0] = (uint8_t)n; b[1] = (uint8_t)(n >> 8); b[2] = (uint8_t)(n >> 16); b[3] = (uint8_t)(n >> 24); }
  void append_message(const uint8_t* label, size_t label_len, const uint8_t* msg, size_t msg_len) {
    uint8_t n[4]; le32((uint32_t)msg_len, n);
    s.meta_ad(label, label_len, false); s.meta_ad(n, 4, true); s.ad(msg, msg_len, false);
  }
  void challenge_bytes(const uint8_t* label, size_t label_len, uint8_t* out, size_t out_len) {
    uint8_t n[4]; le32((uint32_t)out_len, n);
    s.meta_ad(label, label_len, false); s.meta_ad(n, 4, true); s.prf(out, out_len, false);
  }
};

using MerlinTranscript = MerlinTranscriptT<KeccakPerm>;

}  // namespace sbn_host
