// fe_probe.hip — a test-only device probe of the shipped field, G1 and Fq12 layer (csrc/fp.cuh, csrc/g1.cuh, csrc/pairing_kernels.cuh,
// included unmodified).
//
// One host entry point runs one primitive over n cases, one thread per case (4 lanes per case for the quad-cooperative addition,
// one 64-lane wave per case for the wave sum).  Elements cross the boundary as 9 raw signed 32-bit limbs, so a test can feed any
// lazy representation and read back the exact limbs a primitive returned.  Layout of `in` / `out`: [case][lane][element][9 limbs].
// Memory-format ops (is_canonical, unpack, pack, store_tab) carry 8 little-endian 32-bit words in limbs 0..7 of an element.
// The Fq12 ops (f12_*) run one 64-lane block per case over an LDS image of k_pairing_products' own size; a case is ONE row of elements
// (lanes = 1): the operands' 12 coefficients each, then one element whose limb 0 selects where the operands and the result lie:
//   f12_mul  a, b, selector -> result, S[a] and S[b] read back after the call.  Selector: 0 dst, a, b distinct slots; 1 dst == a, b in the
//            line slot PAIR_LINE_OFF (the Miller step); 2 dst == a == b (the squaring; the case's b is not used); 3 dst == b != a;
//            4 a == b != dst (the final exponentiation's powers by u; the case's b is not used)
//   f12_frob, f12_conj, f12_inv_fq  a, selector -> result, S[a] read back.  Selector: 0 dst != a; 1 dst == a
//   f12_final_exp  a -> f12_final_exp of a in slot 0 (no selector)
// Not linked with the product library and not part of include/sbn254.h: tests/test_gpu_fe_bounds.py,
// tests/test_gpu_column_products.py (ops mulu2, squ2, mac2u) and tests/test_gpu_f12_bounds.py (nine, negb_11, f12_*) are its only users.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <type_traits>

#include "../csrc/g1.cuh"
#include "../csrc/pairing_kernels.cuh"

using namespace sbn;

namespace {

enum Group { GF, GG, GQ, GW, GP };   // field op (per field), G1 op (Fq), quad addition (4 lanes), wave sum (64 lanes), Fq12 op (one block a case)
enum Fields { FQ = 1, FR = 2, BOTH = 3 };
struct OpInfo { const char* name; int nin, nout, lanes, group, fields; };

// the op code is the index into this table
const OpInfo OPS[] = {
    {"norm", 1, 1, 1, GF, BOTH},        {"normu", 1, 1, 1, GF, BOTH},       {"add", 2, 1, 1, GF, BOTH},
    {"sub", 2, 1, 1, GF, BOTH},         {"dbl", 1, 1, 1, GF, BOTH},         {"neg", 1, 1, 1, GF, BOTH},
    {"mul", 2, 1, 1, GF, BOTH},         {"sqr", 1, 1, 1, GF, BOTH},         {"mulu", 2, 1, 1, GF, BOTH},
    {"squ", 1, 1, 1, GF, BOTH},         {"reduce", 1, 1, 1, GF, BOTH},      {"canon_small", 1, 1, 1, GF, BOTH},
    {"canon", 1, 1, 1, GF, BOTH},       {"is_zero", 1, 1, 1, GF, BOTH},     {"eq", 2, 1, 1, GF, BOTH},
    {"maybe_zero", 1, 1, 1, GF, BOTH},  {"subb_3_1", 2, 1, 1, GF, FR},      {"subb_4_2", 2, 1, 1, GF, FR},
    {"subb_9_1", 2, 1, 1, GF, FR},      {"subb_14_1", 2, 1, 1, GF, FR},     {"subb_2_1", 2, 1, 1, GF, FQ},
    {"subb_4_1", 2, 1, 1, GF, FQ},      {"subb_4_3", 2, 1, 1, GF, FQ},      {"subb_6_1", 2, 1, 1, GF, FQ},
    {"negb_2", 1, 1, 1, GF, BOTH},      {"negb_4", 1, 1, 1, GF, FQ},        {"fix_nonneg_1", 1, 1, 1, GF, FQ},
    {"fix_nonneg_2", 1, 1, 1, GF, FQ},  {"fix_nonneg_4", 1, 1, 1, GF, FQ},  {"fix_tab", 1, 1, 1, GF, BOTH},
    {"cols_mac12", 24, 1, 1, GF, BOTH}, {"cols_lazy2", 4, 1, 1, GF, BOTH},  {"to_mont", 1, 1, 1, GF, BOTH},
    {"from_mont", 1, 1, 1, GF, BOTH},   {"from_ark_mont", 1, 1, 1, GF, BOTH}, {"ark_mont_to_plain", 1, 1, 1, GF, BOTH},
    {"from_u64", 1, 1, 1, GF, BOTH},    {"inv", 1, 1, 1, GF, BOTH},         {"is_canonical", 1, 1, 1, GF, BOTH},
    {"unpack", 1, 1, 1, GF, BOTH},      {"pack", 1, 1, 1, GF, BOTH},        {"store_tab", 1, 1, 1, GF, BOTH},
    {"madd", 6, 4, 1, GG, FQ},          {"madd_neg", 6, 4, 1, GG, FQ},      {"add_inl", 8, 4, 1, GG, FQ},
    {"dbl_xyzz", 4, 4, 1, GG, FQ},      {"dbl_affine", 2, 4, 1, GG, FQ},    {"to_affine", 4, 2, 1, GG, FQ},
    {"store_load", 4, 4, 1, GG, FQ},    {"add_quad", 8, 4, 4, GQ, FQ},      {"wave_sum", 4, 4, 64, GW, FQ},
    {"mulu2", 4, 2, 1, GF, BOTH},       {"squ2", 2, 2, 1, GF, BOTH},        {"mac2u", 4, 1, 1, GF, BOTH},
    {"nine", 1, 1, 1, GF, FQ},          {"negb_11", 1, 1, 1, GF, FQ},       {"f12_mul", 25, 36, 1, GP, FQ},
    {"f12_frob", 13, 24, 1, GP, FQ},    {"f12_conj", 13, 24, 1, GP, FQ},    {"f12_inv_fq", 13, 24, 1, GP, FQ},
    {"f12_final_exp", 12, 12, 1, GP, FQ},
};
constexpr int NOPS = (int)(sizeof(OPS) / sizeof(OPS[0]));

template <class M> __device__ __forceinline__ Fe<M> ld(const int32_t* s, int i) { Fe<M> r;
  for (int k = 0; k < NL; k++) r.v[k] = (uint32_t)s[i * NL + k];
  return r; }
template <class M> __device__ __forceinline__ void st(int32_t* d, int i, const Fe<M>& x) { for (int k = 0; k < NL; k++) d[i * NL + k] = (int32_t)x.v[k]; }
__device__ __forceinline__ void st_word(int32_t* d, int i, uint32_t w) { for (int k = 0; k < NL; k++) d[i * NL + k] = k == 0 ? (int32_t)w : 0; }
__device__ __forceinline__ void words(const int32_t* s, uint32_t w[8]) { for (int k = 0; k < 8; k++) w[k] = (uint32_t)s[k]; }
__device__ __forceinline__ void st_words(int32_t* d, const uint32_t w[8]) { for (int k = 0; k < NL; k++) d[k] = k < 8 ? (int32_t)w[k] : 0; }
__device__ __forceinline__ XYZZ ld_xyzz(const int32_t* s, int i) { XYZZ p; p.X = ld<FqP>(s, i); p.Y = ld<FqP>(s, i + 1); p.ZZ = ld<FqP>(s, i + 2); p.ZZZ = ld<FqP>(s, i + 3); return p; }
__device__ __forceinline__ void st_xyzz(int32_t* d, const XYZZ& p) { st(d, 0, p.X); st(d, 1, p.Y); st(d, 2, p.ZZ); st(d, 3, p.ZZZ); }

// the op codes a kernel switches on (the table above fixes them; a static_assert keeps the two in step)
enum : int {
  O_NORM, O_NORMU, O_ADD, O_SUB, O_DBL, O_NEG, O_MUL, O_SQR, O_MULU, O_SQU, O_REDUCE, O_CANON_SMALL, O_CANON, O_IS_ZERO, O_EQ,
  O_MAYBE_ZERO, O_SUBB_3_1, O_SUBB_4_2, O_SUBB_9_1, O_SUBB_14_1, O_SUBB_2_1, O_SUBB_4_1, O_SUBB_4_3, O_SUBB_6_1, O_NEGB_2, O_NEGB_4,
  O_FIX1, O_FIX2, O_FIX4, O_FIX_TAB, O_COLS12, O_COLS_LAZY2, O_TO_MONT, O_FROM_MONT, O_FROM_ARK, O_ARK_TO_PLAIN, O_FROM_U64, O_INV,
  O_IS_CANON, O_UNPACK, O_PACK, O_STORE_TAB, O_MADD, O_MADD_NEG, O_ADD_INL, O_DBL_XYZZ, O_DBL_AFF, O_TO_AFF, O_STORE_LOAD, O_ADD_QUAD,
  O_WAVE_SUM, O_MULU2, O_SQU2, O_MAC2U, O_NINE, O_NEGB_11, O_F12_MUL, O_F12_FROB, O_F12_CONJ, O_F12_INV_FQ, O_F12_FINAL_EXP, O_COUNT
};
static_assert(O_COUNT == NOPS, "op enum and table differ");

template <class M>
__global__ void field_kernel(int op, const int32_t* __restrict__ in, int32_t* __restrict__ out, size_t n, int nin, int nout) {
  const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n) return;
  const int32_t* s = in + t * (size_t)nin * NL;
  int32_t* d = out + t * (size_t)nout * NL;
  const Fe<M> a = ld<M>(s, 0);
  switch (op) {
    case O_NORM: st(d, 0, fe_norm(a)); break;
    case O_NORMU: st(d, 0, fe_normu(a)); break;
    case O_ADD: st(d, 0, fe_add(a, ld<M>(s, 1))); break;
    case O_SUB: st(d, 0, fe_sub(a, ld<M>(s, 1))); break;
    case O_DBL: st(d, 0, fe_dbl(a)); break;
    case O_NEG: st(d, 0, fe_neg(a)); break;
    case O_MUL: st(d, 0, fe_mul(a, ld<M>(s, 1))); break;
    case O_SQR: st(d, 0, fe_sqr(a)); break;
    case O_MULU: st(d, 0, fe_mulu(a, ld<M>(s, 1))); break;
    case O_SQU: st(d, 0, fe_squ(a)); break;
    case O_REDUCE: st(d, 0, fe_reduce(a)); break;
    case O_CANON_SMALL: st(d, 0, fe_canon_small(a)); break;
    case O_CANON: st(d, 0, fe_canon(a)); break;
    case O_IS_ZERO: st_word(d, 0, fe_is_zero(a) ? 1u : 0u); break;
    case O_EQ: st_word(d, 0, fe_eq(a, ld<M>(s, 1)) ? 1u : 0u); break;
    case O_MAYBE_ZERO: st_word(d, 0, fe_maybe_zero(a) ? 1u : 0u); break;
    case O_SUBB_3_1: st(d, 0, fe_subb<M, 3, 1>(a, ld<M>(s, 1))); break;
    case O_SUBB_4_2: st(d, 0, fe_subb<M, 4, 2>(a, ld<M>(s, 1))); break;
    case O_SUBB_9_1: st(d, 0, fe_subb<M, 9, 1>(a, ld<M>(s, 1))); break;
    case O_SUBB_14_1: st(d, 0, fe_subb<M, 14, 1>(a, ld<M>(s, 1))); break;
    case O_SUBB_2_1: st(d, 0, fe_subb<M, 2, 1>(a, ld<M>(s, 1))); break;
    case O_SUBB_4_1: st(d, 0, fe_subb<M, 4, 1>(a, ld<M>(s, 1))); break;
    case O_SUBB_4_3: st(d, 0, fe_subb<M, 4, 3>(a, ld<M>(s, 1))); break;
    case O_SUBB_6_1: st(d, 0, fe_subb<M, 6, 1>(a, ld<M>(s, 1))); break;
    case O_NEGB_2: st(d, 0, fe_negb<M, 2>(a)); break;
    case O_NEGB_4: st(d, 0, fe_negb<M, 4>(a)); break;
    case O_FIX1: st(d, 0, fe_fix_nonneg<M, 1>(a)); break;
    case O_FIX2: st(d, 0, fe_fix_nonneg<M, 2>(a)); break;
    case O_FIX4: st(d, 0, fe_fix_nonneg<M, 4>(a)); break;
    case O_FIX_TAB: st(d, 0, fe_fix_tab(a)); break;
    case O_COLS12: {                    // 6 products, a carry pass, 6 more products, one reduction (the sumcheck rounds' pattern)
      Cols c; cols_zero(c);
      for (int i = 0; i < 6; i++) cols_mac<M>(c, ld<M>(s, 2 * i), ld<M>(s, 2 * i + 1));
      cols_carry(c);
      for (int i = 6; i < 12; i++) cols_mac<M>(c, ld<M>(s, 2 * i), ld<M>(s, 2 * i + 1));
      st(d, 0, cols_reduce<M>(c));
    } break;
    case O_COLS_LAZY2: {                // g1.cuh's Y3: two products with one lazy operand each, one reduction
      Cols c; cols_zero(c);
      cols_mac_lazy<M>(c, a, ld<M>(s, 1)); cols_mac_lazy<M>(c, ld<M>(s, 2), ld<M>(s, 3));
      st(d, 0, cols_reduce<M>(c));
    } break;
    case O_TO_MONT: st(d, 0, fe_to_mont(a)); break;
    case O_FROM_MONT: st(d, 0, fe_from_mont(a)); break;
    case O_FROM_ARK: st(d, 0, fe_from_ark_mont(a)); break;
    case O_ARK_TO_PLAIN: st(d, 0, fe_ark_mont_to_plain(a)); break;
    case O_FROM_U64: st(d, 0, fe_from_u64<M>((unsigned long long)(uint32_t)s[0] | (unsigned long long)(uint32_t)s[1] << 32)); break;
    case O_INV: st(d, 0, fe_inv(a)); break;
    case O_IS_CANON: { uint32_t w[8]; words(s, w); st_word(d, 0, fe_is_canonical<M>(w) ? 1u : 0u); } break;
    case O_UNPACK: { uint32_t w[8]; words(s, w); st(d, 0, fe_unpack<M>(w)); } break;
    case O_PACK: { uint32_t w[8]; fe_pack(a, w); st_words(d, w); } break;
    case O_STORE_TAB: {                 // the shipped store of intermediate tables, into an aligned private buffer
      uint4 buf[2]; fe_store_tab<M>(buf, a);
      const uint32_t w[8] = {buf[0].x, buf[0].y, buf[0].z, buf[0].w, buf[1].x, buf[1].y, buf[1].z, buf[1].w};
      st_words(d, w);
    } break;
    case O_MULU2: { Fe<M> r0, r1; fe_mulu2(a, ld<M>(s, 1), ld<M>(s, 2), ld<M>(s, 3), r0, r1); st(d, 0, r0); st(d, 1, r1); } break;      // (a0, b0, a1, b1)
    case O_SQU2: { Fe<M> r0, r1; fe_squ2(a, ld<M>(s, 1), r0, r1); st(d, 0, r0); st(d, 1, r1); } break;
    case O_MAC2U: st(d, 0, fe_mac2u(a, ld<M>(s, 1), ld<M>(s, 2), ld<M>(s, 3))); break;                                                   // a0 b0 + a1 b1, one reduction
    case O_NINE: if constexpr (std::is_same<M, FqP>::value) st(d, 0, fe_nine(a)); break;                                                 // pairing_kernels.cuh, Fq only
    case O_NEGB_11: st(d, 0, fe_negb<M, 11>(a)); break;
    default: break;
  }
}

__global__ void g1_kernel(int op, const int32_t* __restrict__ in, int32_t* __restrict__ out, size_t n, int nin, int nout) {
  const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n) return;
  const int32_t* s = in + t * (size_t)nin * NL;
  int32_t* d = out + t * (size_t)nout * NL;
  switch (op) {
    case O_MADD: case O_MADD_NEG: {
      XYZZ acc = ld_xyzz(s, 0); Affine q; q.x = ld<FqP>(s, 4); q.y = ld<FqP>(s, 5);
      xyzz_madd(acc, q, op == O_MADD_NEG);
      st_xyzz(d, acc);
    } break;
    case O_ADD_INL: st_xyzz(d, xyzz_add_inl(ld_xyzz(s, 0), ld_xyzz(s, 4))); break;
    case O_DBL_XYZZ: st_xyzz(d, xyzz_dbl(ld_xyzz(s, 0))); break;
    case O_DBL_AFF: { Affine q; q.x = ld<FqP>(s, 0); q.y = ld<FqP>(s, 1); st_xyzz(d, xyzz_dbl_affine(q)); } break;
    case O_TO_AFF: { const Affine r = xyzz_to_affine(ld_xyzz(s, 0)); st(d, 0, r.x); st(d, 1, r.y); } break;
    case O_STORE_LOAD: {
      uint4 buf[8]; xyzz_store(buf, ld_xyzz(s, 0));
      st_xyzz(d, xyzz_load(buf));
    } break;
    default: break;
  }
}

// 4 lanes per case (all four hold the same operands, as in the reduction kernels); every lane writes its own result
__global__ void quad_kernel(const int32_t* __restrict__ in, int32_t* __restrict__ out, size_t n) {
  const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t / 4 >= n) return;             // whole quads only: blockDim is a multiple of 4
  const XYZZ r = xyzz_add_quad(ld_xyzz(in + t * 8 * NL, 0), ld_xyzz(in + t * 8 * NL, 4), (int)(threadIdx.x & 3));
  st_xyzz(out + t * 4 * NL, r);
}
// one 64-lane block per case: the sum of the 64 lanes' points, returned in every lane
__global__ void wave_kernel(const int32_t* __restrict__ in, int32_t* __restrict__ out) {
  const size_t t = (size_t)blockIdx.x * 64 + threadIdx.x;
  st_xyzz(out + t * 4 * NL, wave_sum_all(ld_xyzz(in + t * 4 * NL, 0)));
}

// the slots (word offsets into S) of the Fq12 ops' selectors: {dst, a, b}
constexpr int F12_MUL_SELS = 5, F12_UNARY_SELS = 2;
__device__ const int F12_MUL_SLOTS[F12_MUL_SELS][3] = {{2 * F12_WORDS, 0, F12_WORDS}, {0, 0, PAIR_LINE_OFF}, {0, 0, 0}, {F12_WORDS, 0, F12_WORDS}, {2 * F12_WORDS, 0, 0}};
int f12_selectors(int op) { return op == O_F12_MUL ? F12_MUL_SELS : op == O_F12_FINAL_EXP ? 0 : F12_UNARY_SELS; }
// one 64-lane block per case, S as k_pairing_products declares and clears it; the host has checked every selector
__global__ void __launch_bounds__(64) f12_kernel(int op, const int32_t* __restrict__ in, int32_t* __restrict__ out, int nin, int nout) {
  __shared__ uint32_t S[PAIR_LDS_WORDS];
  const int lane = threadIdx.x;
  const int32_t* s = in + (size_t)blockIdx.x * nin * NL;
  int32_t* d = out + (size_t)blockIdx.x * nout * NL;
  for (int i = lane; i < PAIR_LDS_WORDS; i += 64) S[i] = 0;
  __syncthreads();
  int dst = 0, a = 0, b = 0;
  if (op == O_F12_MUL) {
    const int sel = min(max(s[24 * NL], 0), F12_MUL_SELS - 1);
    dst = F12_MUL_SLOTS[sel][0]; a = F12_MUL_SLOTS[sel][1]; b = F12_MUL_SLOTS[sel][2];
  } else if (op != O_F12_FINAL_EXP) {
    dst = s[12 * NL] == 1 ? 0 : F12_WORDS;
  }
  for (int i = lane; i < F12_WORDS; i += 64) {
    S[a + i] = (uint32_t)s[i];
    if (op == O_F12_MUL && b != a) S[b + i] = (uint32_t)s[F12_WORDS + i];
  }
  __syncthreads();
  if (op == O_F12_MUL) f12_mul(S, dst, a, b, lane);
  else if (op == O_F12_FROB) f12_frob(S, dst, a, lane);
  else if (op == O_F12_CONJ) f12_conj(S, dst, a, lane);
  else if (op == O_F12_INV_FQ) f12_inv_fq(S, dst, a, lane);
  else f12_final_exp(S, lane);
  for (int i = lane; i < F12_WORDS; i += 64) {
    d[i] = (int32_t)S[dst + i];
    if (op != O_F12_FINAL_EXP) d[F12_WORDS + i] = (int32_t)S[a + i];
    if (op == O_F12_MUL) d[2 * F12_WORDS + i] = (int32_t)S[b + i];
  }
}

int fail(char* err, size_t errlen, const char* what, hipError_t e) {
  if (err && errlen) snprintf(err, errlen, "%s: %s", what, hipGetErrorString(e));
  return (int)e;
}

}  // namespace

extern "C" {

int fe_probe_num_ops() { return NOPS; }
const char* fe_probe_op_name(int op) { return op >= 0 && op < NOPS ? OPS[op].name : nullptr; }
// 0 and the per-lane element counts if `op` exists for `field` (0 = Fq, 1 = Fr), -1 otherwise
int fe_probe_shape(int op, int field, int* nin, int* nout, int* lanes) {
  if (op < 0 || op >= NOPS || field < 0 || field > 1 || !(OPS[op].fields & (1 << field))) return -1;
  *nin = OPS[op].nin; *nout = OPS[op].nout; *lanes = OPS[op].lanes;
  return 0;
}
// runs `op` on n cases: allocates, copies, launches, synchronises, copies back, frees; returns the HIP status (0 on success)
int fe_probe_run(int op, int field, const int32_t* in, int32_t* out, size_t n, char* err, size_t errlen) {
  int nin, nout, lanes;
  if (err && errlen) err[0] = 0;
  if (fe_probe_shape(op, field, &nin, &nout, &lanes) != 0) return fail(err, errlen, "no such op for this field", hipErrorInvalidValue);
  if (n == 0) return 0;
  if (OPS[op].group == GP && f12_selectors(op)) {          // a selector picks LDS offsets: refuse one the kernel does not know
    for (size_t c = 0; c < n; c++) {
      const int32_t sel = in[(c * nin + (nin - 1)) * NL];
      if (sel < 0 || sel >= f12_selectors(op)) return fail(err, errlen, "no such placement selector", hipErrorInvalidValue);
    }
  }
  const size_t bin = n * lanes * nin * NL * sizeof(int32_t), bout = n * lanes * nout * NL * sizeof(int32_t);
  int32_t *din = nullptr, *dout = nullptr;
  hipError_t e = hipMalloc((void**)&din, bin);
  if (e != hipSuccess) return fail(err, errlen, "hipMalloc", e);
  e = hipMalloc((void**)&dout, bout);
  if (e != hipSuccess) { hipFree(din); return fail(err, errlen, "hipMalloc", e); }
  const char* what = "hipMemcpy H2D";
  e = hipMemcpy(din, in, bin, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemset(dout, 0, bout), what = "hipMemset";
  if (e == hipSuccess) {
    const unsigned blocks = (unsigned)((n * lanes + 63) / 64);
    const int g = OPS[op].group;
    if (g == GF && field == 0) field_kernel<FqP><<<blocks, 64>>>(op, din, dout, n, nin, nout);
    else if (g == GF) field_kernel<FrP><<<blocks, 64>>>(op, din, dout, n, nin, nout);
    else if (g == GG) g1_kernel<<<blocks, 64>>>(op, din, dout, n, nin, nout);
    else if (g == GQ) quad_kernel<<<blocks, 64>>>(din, dout, n);
    else if (g == GP) f12_kernel<<<(unsigned)n, 64>>>(op, din, dout, nin, nout);
    else wave_kernel<<<(unsigned)n, 64>>>(din, dout);
    what = "launch";
    e = hipGetLastError();
    if (e == hipSuccess) e = hipDeviceSynchronize(), what = "kernel";
  }
  if (e == hipSuccess) e = hipMemcpy(out, dout, bout, hipMemcpyDeviceToHost), what = "hipMemcpy D2H";
  hipFree(din); hipFree(dout);
  return e == hipSuccess ? 0 : fail(err, errlen, what, e);
}

}  // extern "C"
