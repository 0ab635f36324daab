// abi_random_tape.inc — C ABI: the prover's RandomTape (reference src/random.rs) and the draw plans that fill the `rnd` of every one-call prover
// (include/sbn254.h).  Host only: no context, no device, no launch; random_tape_host.hpp holds the tape and the plans, this file the handle, the
// shapes (the same helpers the *_sizes calls use, so a plan's count is theirs) and the refusals.  A refusal draws nothing: the tape is unchanged.
// The reason of a refusal is kept in the handle (sbn_random_tape_last_error), or per thread where there is no handle yet.  Neither `init` nor a draw
// is ever part of such a text.  Included by sbn254.hip behind abi_kzg_srs.inc.
#include <sys/random.h>
#include <cerrno>

struct sbn_random_tape {
  sbn_host::tape::RandomTape t;
  std::string err;
};

static thread_local std::string g_tape_err;      // sbn_random_tape_new's own refusals: there is no handle to keep them in

static int tape_fail(sbn_random_tape* tp, int code, const char* fmt, ...) {
  char buf[512];
  va_list ap; va_start(ap, fmt); vsnprintf(buf, sizeof buf, fmt, ap); va_end(ap);
  if (tp) tp->err = buf; else g_tape_err = buf;
  return code;
}

// a plan's common front: the handle, the buffer, and the caller's count against the plan's
static int tape_plan_check(sbn_random_tape* tp, const char* pfx, const uint8_t* out, size_t out_scalars, size_t want) {
  if (!tp) return SBN_EINVAL;
  if (!out && want) return tape_fail(tp, SBN_EINVAL, "%s: a NULL buffer for %zu scalars", pfx, want);
  if (out_scalars != want) return tape_fail(tp, SBN_EINVAL, "%s: the buffer holds %zu scalars, the shape draws %zu", pfx, out_scalars, want);
  return SBN_OK;
}

extern "C" {

const char* sbn_random_tape_last_error(const sbn_random_tape* tp) { return tp ? tp->err.c_str() : g_tape_err.c_str(); }

int sbn_random_tape_new(const uint8_t* name, size_t name_len, const uint8_t* init, sbn_random_tape** out) {
  if (!out || (!name && name_len)) return SBN_EINVAL;
  *out = nullptr;
  if (name_len > UINT32_MAX) return tape_fail(nullptr, SBN_EINVAL, "random tape: a name of %zu bytes: a transcript message has a 32-bit length", name_len);
  uint8_t seed[32];
  if (init) {
    if (!fr_canonical(init)) return tape_fail(nullptr, SBN_EINVAL, "random tape: init is not canonical (>= r)  [scalar.rs:87-95]");
    memcpy(seed, init, 32);
  } else {                                                                        // Scalar::random(&mut OsRng), random.rs:18-20
    uint8_t wide[64]; size_t got = 0;
    while (got < sizeof wide) {
      const ssize_t k = getrandom(wide + got, sizeof wide - got, 0);
      if (k < 0 && errno == EINTR) continue;
      if (k <= 0) {
        const int e = errno;
        sbn_host::tape::secure_zero(wide, sizeof wide);
        return tape_fail(nullptr, SBN_EOS, "random tape: getrandom: %s", k < 0 ? strerror(e) : "no bytes");
      }
      got += (size_t)k;
    }
    sbn_host::transcript_wide_reduce(wide, seed);
    sbn_host::tape::secure_zero(wide, sizeof wide);
  }
  sbn_random_tape* tp = new sbn_random_tape();
  static const uint8_t NONE[1] = {0};
  tp->t.init(name ? name : NONE, name_len, seed);
  sbn_host::tape::secure_zero(seed, sizeof seed);
  *out = tp;
  return SBN_OK;
}

void sbn_random_tape_free(sbn_random_tape* tp) {
  if (!tp) return;
  tp->t.wipe();
  delete tp;
}

int sbn_random_tape_scalars(sbn_random_tape* tp, const uint8_t* label, size_t label_len, size_t n, uint8_t* out) {
  if (!tp) return SBN_EINVAL;
  if ((!label && label_len) || (!out && n)) return tape_fail(tp, SBN_EINVAL, "random tape: a NULL label or buffer");
  if (label_len > UINT32_MAX) return tape_fail(tp, SBN_EINVAL, "random tape: a label of %zu bytes: a transcript message has a 32-bit length", label_len);
  static const uint8_t NONE[1] = {0};
  tp->t.draw(sbn_host::Label(label ? label : NONE, label_len), out, n);
  return SBN_OK;
}

int sbn_zk_sumcheck_draw_rnd(size_t num_rounds, size_t n, sbn_random_tape* tp, uint8_t* out, size_t out_scalars) {
  if (!tp) return SBN_EINVAL;
  if (num_rounds < 1 || num_rounds > 64 || (n != 3 && n != 4)) return tape_fail(tp, SBN_EINVAL, "zk sumcheck draws: %zu rounds of %zu coefficients (1 .. 64 rounds; 4: r1cs, 3: quad)", num_rounds, n);
  int rc;
  if ((rc = tape_plan_check(tp, "zk sumcheck draws", out, out_scalars, sbn_host::tape::count_zk_sumcheck(num_rounds, n)))) return rc;
  sbn_host::tape::plan_zk_sumcheck(tp->t, num_rounds, n, out);
  return SBN_OK;
}

int sbn_polyeval_draw_rnd(size_t ell, sbn_random_tape* tp, uint8_t* out, size_t out_scalars) {
  if (!tp) return SBN_EINVAL;
  if (ell < 1 || ell > 40) return tape_fail(tp, SBN_EINVAL, "polyeval draws: ell = %zu (1 .. 40, as sbn_polyeval_prove)", ell);
  const size_t lg = ell - ell / 2;
  int rc;
  if ((rc = tape_plan_check(tp, "polyeval draws", out, out_scalars, sbn_host::tape::count_polyeval(lg)))) return rc;
  sbn_host::tape::plan_polyeval(tp->t, lg, out);
  return SBN_OK;
}

int sbn_r1cs_proof_draw_rnd(size_t num_cons, size_t num_vars, sbn_random_tape* tp, uint8_t* out, size_t out_scalars) {
  if (!tp) return SBN_EINVAL;
  R1csProofShape s;
  if (!r1cs_proof_shape(num_cons, num_vars, &s)) return tape_fail(tp, SBN_EINVAL, "r1cs proof draws: shape %zu x %zu is one sbn_r1cs_proof_sizes refuses", num_cons, num_vars);
  int rc;
  if ((rc = tape_plan_check(tp, "r1cs proof draws", out, out_scalars, s.rnd_scalars))) return rc;
  sbn_host::tape::plan_r1cs_proof(tp->t, s.L, s.nx, s.ny, s.lg, out);
  return SBN_OK;
}

int sbn_sparse_eval_draw_rnd(size_t num_vars_x, size_t num_vars_y, size_t num_ops, size_t batch, int kzg, sbn_random_tape* tp, uint8_t* out, size_t out_scalars) {
  if (!tp) return SBN_EINVAL;
  SparseEvalShape s;
  if (!sparse_eval_shape(num_vars_x, num_vars_y, num_ops, batch, &s)) return tape_fail(tp, SBN_EINVAL, "sparse eval draws: the shape is one sbn_sparse_eval_sizes refuses");
  const size_t want = kzg ? s.rnd_scalars_kzg : s.rnd_scalars;
  int rc;
  if ((rc = tape_plan_check(tp, "sparse eval draws", out, out_scalars, want))) return rc;
  sbn_host::tape::plan_sparse_eval(tp->t, s.lg_d, s.lg_o, s.lg_m, kzg != 0, out);
  return SBN_OK;
}

int sbn_snark_draw_rnd(const sbn_snark_key* key, int kzg, sbn_random_tape* tp, uint8_t* out, size_t out_scalars) {
  if (!tp || !key) return SBN_EINVAL;
  SnarkShapes s;
  if (!snark_shapes(key, kzg != 0, &s)) return tape_fail(tp, SBN_EINVAL, "snark draws: the key's shape is one sbn_snark_sizes refuses");
  int rc;
  if ((rc = tape_plan_check(tp, "snark draws", out, out_scalars, s.z.rnd_scalars))) return rc;
  uint8_t* mid = sbn_host::tape::plan_r1cs_proof(tp->t, s.r.L, s.r.nx, s.r.ny, s.r.lg, out);      // ONE tape over both halves, draws in call order (snark.rs:438)
  sbn_host::tape::plan_sparse_eval(tp->t, s.e.lg_d, s.e.lg_o, s.e.lg_m, kzg != 0, mid);
  return SBN_OK;
}

int sbn_nizk_draw_rnd(const sbn_nizk_inst* inst, sbn_random_tape* tp, uint8_t* out, size_t out_scalars) {
  if (!tp || !inst) return SBN_EINVAL;
  NizkShapes s;
  if (!nizk_shapes(inst, &s)) return tape_fail(tp, SBN_EINVAL, "nizk draws: the instance's shape is one sbn_nizk_sizes refuses");
  int rc;
  if ((rc = tape_plan_check(tp, "nizk draws", out, out_scalars, s.z.rnd_scalars))) return rc;
  sbn_host::tape::plan_r1cs_proof(tp->t, s.r.L, s.r.nx, s.r.ny, s.r.lg, out);
  return SBN_OK;
}

}  // extern "C"
