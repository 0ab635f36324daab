// abi_transcript.inc — C ABI: a Merlin v1.0 transcript (merlin::Transcript as src/transcript.rs uses it) on the host.  The plan of a
// sumcheck round's transcript work that the device step executes (transcript_kernels.cuh) is transcript_plan.hpp's.  No context, no device.
#include "transcript_plan.hpp"      // transcript_plan_round

struct sbn_transcript { sbn_host::MerlinTranscript t; };

extern "C" {

int sbn_transcript_new(const uint8_t* label, size_t label_len, sbn_transcript** out) {
  if (!out || (!label && label_len) || label_len > 0xffffffffu) return SBN_EINVAL;
  sbn_transcript* t = new (std::nothrow) sbn_transcript();
  if (!t) return SBN_ENOMEM;
  t->t.init(label, label_len);
  *out = t;
  return SBN_OK;
}
int sbn_transcript_clone(const sbn_transcript* t, sbn_transcript** out) {
  if (!t || !out) return SBN_EINVAL;
  sbn_transcript* n = new (std::nothrow) sbn_transcript(*t);
  if (!n) return SBN_ENOMEM;
  *out = n;
  return SBN_OK;
}
void sbn_transcript_free(sbn_transcript* t) { delete t; }
int sbn_transcript_append_message(sbn_transcript* t, const uint8_t* label, size_t label_len, const uint8_t* msg, size_t msg_len) {
  if (!t || (!label && label_len) || (!msg && msg_len) || msg_len > 0xffffffffu) return SBN_EINVAL;
  t->t.append_message(label, label_len, msg, msg_len);
  return SBN_OK;
}
int sbn_transcript_challenge_bytes(sbn_transcript* t, const uint8_t* label, size_t label_len, uint8_t* out, size_t out_len) {
  if (!t || (!label && label_len) || (!out && out_len) || out_len > 0xffffffffu) return SBN_EINVAL;
  t->t.challenge_bytes(label, label_len, out, out_len);
  return SBN_OK;
}
int sbn_transcript_challenge_scalar(sbn_transcript* t, const uint8_t* label, size_t label_len, uint8_t out[32]) {
  if (!t || (!label && label_len) || !out) return SBN_EINVAL;
  sbn_host::Script{t->t}.challenge(sbn_host::Label(label, label_len), out);
  return SBN_OK;
}
int sbn_fr_from_wide(const uint8_t in[64], uint8_t out[32]) {
  if (!in || !out) return SBN_EINVAL;
  sbn_host::transcript_wide_reduce(in, out);
  return SBN_OK;
}
int sbn_transcript_state(const sbn_transcript* t, uint8_t out[203]) {
  if (!t || !out) return SBN_EINVAL;
  memcpy(out, t->t.s.st, 200); out[200] = t->t.s.pos; out[201] = t->t.s.pos_begin; out[202] = t->t.s.cur_flags;
  return SBN_OK;
}
int sbn_transcript_from_state(const uint8_t in[203], sbn_transcript** out) {
  if (!in || !out) return SBN_EINVAL;
  // what a STROBE-128 state can hold: pos inside the rate, pos_begin at most one past it, flags within the six defined bits
  if (in[200] >= sbn_host::Strobe128::RATE || in[201] > sbn_host::Strobe128::RATE || (in[202] & 0xc0)) return SBN_EINVAL;
  sbn_transcript* t = new (std::nothrow) sbn_transcript();
  if (!t) return SBN_ENOMEM;
  memcpy(t->t.s.st, in, 200); t->t.s.pos = in[200]; t->t.s.pos_begin = in[201]; t->t.s.cur_flags = in[202];
  *out = t;
  return SBN_OK;
}

}  // extern "C"
