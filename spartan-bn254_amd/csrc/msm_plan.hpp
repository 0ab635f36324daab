// msm_plan.hpp — the integer rules of a bucket job, host-only: window choice, the SBN_* overrides of the MSM / commit path, the geometry of the
// accumulate, the reduction and the two sorts.  No HIP, no context, no launches: msm_host.hpp turns a plan into ensure() calls and launches, and
// tests/msm_plan_check.cpp holds it against tests/acc_model.py in a plain g++ build.  Included by msm_kernels.cuh: the kernels share its constants.
#pragma once
#include <algorithm>
#include <climits>
#include <cstddef>
#include <cstdint>
#include <cstdlib>

namespace sbn {

struct MsmShape {
  int c;        // window bits
  int W;        // number of windows
  int nb;       // buckets per window = 2^(c-1)
};
enum { MODE_SINGLE = 0, MODE_ROWS = 1 };   // msm_kernels.cuh: the two front-ends of a bucket job

constexpr int MSM_C_MAX = 16;             // widest window of the one-level sort: a digit fits 16 bits (dig_t), a window's counters fit LDS
constexpr uint32_t ACC_SEG_MAX = 8192;   // longest chain one lane runs before a bucket is cut into segments
constexpr uint32_t MERGE_LANE_MAX = 12;  // most partial sums of a bucket that k_acc_merge folds with one lane; beyond, one wave per bucket
constexpr int S2_LO_LOG_MAX = 11, S2_LO_MAX = 1 << S2_LO_LOG_MAX;      // most buckets per partition (LDS counters of level 2)
constexpr int S2_P_MAX = 1024;                                        // most partitions per window (one scan lane each in level 1)
constexpr int S2_SPT = 8;                                 // scalars per thread in level 1: 8192 per block (large inputs)
constexpr int S2_SPT_SMALL = 2;                           // ... up to 2^21 scalars: 8192 per block would be 128 - 256 blocks, half the chip or less (k_s2_scatter at 2^20: 95 us)
constexpr int S2_C_MIN = 13, S2_C_MAX = 22;               // window bits this path is built for (P = 2^(c-12) partitions: 2 .. 1024)
constexpr uint32_t S2_SUB = 16384;                        // entries of a level-2 sub-chunk (k_s2_prefix_hi)
constexpr int COMB_C_MAX = 17;   // widest lookup window (c = 17: 15 windows; 177 GB for the 2814 unique points of the 8193-generator set)

// Numeric overrides of the automatic choices (tools/README.md), for experiments.  Read ONCE per job, at its entry (msm_device,
// commit_rows_launch), and passed down: the tests change these variables between calls on one context.  0 = unset or out of range.
struct MsmOverrides {
  bool c_set = false; int c = 0;   // SBN_MSM_C: present, whatever it holds (glv_applies keeps the plain windows then); its value: choose_shape takes 7 .. chard, glv_shape 13 .. 17
  int seg = 0, red_l = 0;          // SBN_MSM_SEG 8 .. ACC_SEG_MAX, SBN_RED_L 1 .. 64, any value
  int s2_lo = 0, s2_spt = 0;       // SBN_SORT2_LO 4 .. S2_LO_LOG_MAX, SBN_SORT2_SPT S2_SPT_SMALL or S2_SPT
  int comb_s = 0;                  // SBN_COMB_S 1 .. 128
};
static MsmOverrides msm_overrides_read() {
  MsmOverrides o;
  auto num = [](const char* n, int lo, int hi, int* out) { const char* e = getenv(n); if (!e) return false; const int v = atoi(e); if (v >= lo && v <= hi) *out = v; return true; };
  o.c_set = num("SBN_MSM_C", INT_MIN, INT_MAX, &o.c);
  num("SBN_MSM_SEG", 8, (int)ACC_SEG_MAX, &o.seg); num("SBN_RED_L", 1, 64, &o.red_l); num("SBN_SORT2_LO", 4, S2_LO_LOG_MAX, &o.s2_lo);
  num("SBN_SORT2_SPT", S2_SPT_SMALL, S2_SPT, &o.s2_spt); if (o.s2_spt != S2_SPT && o.s2_spt != S2_SPT_SMALL) o.s2_spt = 0;
  num("SBN_COMB_S", 1, 128, &o.comb_s);
  return o;
}

// Signed radix-2^c digits: W windows cover `bits` bits (254: canonical scalars; 127: GLV half-scalars), the top digit (+ carry)
// must stay <= 2^(c-1).
static MsmShape make_shape(int c, int bits = 254) {
  MsmShape s; s.c = c; s.nb = 1 << (c - 1);
  int W = (bits + c - 1) / c;
  int tb = bits - (W - 1) * c;         // bits in the top window
  if (tb > c - 1) W += 1;
  s.W = W;
  return s;
}
// The window model, in modular products: `terms`*W mixed adds (10 each) into `sets` bucket sets of 2^(c-1) buckets (W sets, or one shared by
// the windows of a row), each bucket costing `per_bucket` products in the running-sum reduction.
static double window_cost(size_t terms, const MsmShape& s, int bits, bool shared_bucket_set, double per_bucket) {
  const double sets = shared_bucket_set ? 1.0 : (double)s.W;
  double cost = (double)terms * s.W * 10.0 + sets * s.nb * per_bucket;
  // a top window narrower than c - 1 bits fills only 2^tb of its buckets, each 2^(c-1-tb) times over: those go through the
  // segment work list (k_acc_extra / k_acc_merge), measured at about half a window's worth of additions on top
  if (!shared_bucket_set && bits - (s.W - 1) * s.c < s.c - 1) cost += (double)terms * 5.0;
  return cost;
}
// Window size from the cost model above: each bucket costing ~2 full adds (14 each) in the running-sum reduction (x2 for the wave-level part).
// SBN_MSM_C overrides for experiments.
// Small jobs (`problems` x `terms` far below the chip's lane count) are latency-bound: what counts is the length of the longest
// bucket chain, not the number of products, so they take the smallest window with a mean bucket load <= 4.
// `chard`: the widest window the caller's sort can take (MSM_C_MAX for the one-level LDS sort, S2_C_MAX for the two-level one).
static MsmShape choose_shape(const MsmOverrides& o, size_t terms, bool shared_bucket_set, int cmax, size_t problems = 0, int chard = MSM_C_MAX) {
  if (o.c >= 7 && o.c <= chard) return make_shape(o.c);
  if (cmax > chard) cmax = chard;
  if (problems && problems * terms <= 32768) {
    // one MSM of 512 .. 4096 terms: the narrowest windows, their overloaded buckets (16 - 64 points, the top window's two with n / 2 each) cut into
    // segments of 8 (acc_plan) — 64 buckets per window keep the two reduction levels short: 353 / 371 / 407 us at 2^10 / 2^11 / 2^12 against
    // 479 / 474 / 478 with the rule below (c = 15, segments of 32); profiles/r04_small_msm_window_sweep.txt
    if (!shared_bucket_set && problems == 1 && terms >= 512 && terms <= 4096 && cmax >= 8) return make_shape(terms <= 512 ? 8 : 7);
    // expected longest chain ~ mean load + the load of the top window's few buckets (it holds only 254 - (W-1)c bits)
    double bl = 1e300; int bcl = 7;
    for (int c = 7; c <= cmax; c++) {
      MsmShape s = make_shape(c);
      const int tb = 254 - (s.W - 1) * c;
      const double top = (double)terms / (double)(1u << (tb > 0 ? (tb < 20 ? tb : 20) : 0));
      const double load = (shared_bucket_set ? (double)terms * s.W / s.nb : (double)terms / s.nb) + top;
      if (load <= 6.0) return s;
      if (load < bl) { bl = load; bcl = c; }
    }
    return make_shape(bcl);
  }
  // One MSM between the latency regime and 2^20 terms: c = 15 (254 = 16 x 15 + 14: the top window is as wide as the others).  The product count below
  // would pick windows whose top digit has 2 - 7 bits (c = 8, 12, 13): their handful of top buckets take n / 2^tb points each, a chain of segments and
  // merges that runs AFTER the main pass — measured (tools/sweep_small_msm_c.py, profiles/r04_small_msm_window_sweep.txt) at 2^16 / 2^17 / 2^18:
  // 880 / 1055 / 1209 us with c = 12 / 13 / 13 against 610 / 769 / 1129 with c = 15; 15 is also the measured optimum at 2^15 and 2^19.
  if (!shared_bucket_set && terms < ((size_t)1 << 20) && cmax >= 15) return make_shape(15);
  double best = 1e300; int bc = 7;
  // cmax: one sort block keeps all 2^(c-1) counters of a problem in LDS; beyond that every block re-reads its digits once
  // per counter range (measured at 2^26, c = 20: sort 82 ms vs accumulate 74 ms), which costs more than the 13 -> 16 windows;
  // the two-level sort (sort2_kernels.cuh) has no such cap and lets large single MSMs take c up to 22.
  for (int c = 7; c <= cmax; c++) {
    // per bucket: ~56 products in the one-level regime (measured at 2^20), ~40 once the reduction runs on millions of buckets
    // (many rows over one bucket set each are the same throughput regime: the derefs matrix, 4096 rows x 2814 merged columns, c = 11 / 12 / 13 ->
    //  19.6 / 18.2 / 19.0 ms — with 56 the model ties 11 and 12 and takes 11; tools/sweep_hyrax_bucket.sh)
    const double per_bucket = (chard > MSM_C_MAX || (shared_bucket_set && problems >= 256)) ? 40.0 : 56.0;
    const double cost = window_cost(terms, make_shape(c), 254, shared_bucket_set, per_bucket);
    if (cost < best) { best = cost; bc = c; }
  }
  return make_shape(bc);
}

// ---- GLV (glv_kernels.cuh): one MSM of n full-width scalars as an MSM of 2n half-width ones over P_i and phi(P_i) ----
// Products of the window model above for one MSM in the two-level sort regime (40 per bucket)
static double single_msm_cost(size_t terms, const MsmShape& s, int bits) { return window_cost(terms, s, bits, false, 40.0); }
// GLV shape for n bases (2n half-scalars of 127 bits): SBN_MSM_C when it is one of the instantiated widths, else the model's best of 13..17
// (c = 16: 8 windows of 16 bits fill all 2^15 buckets of the top window, 127 = 7 x 16 + 15)
static MsmShape glv_shape(const MsmOverrides& o, size_t n) {
  if (o.c >= 13 && o.c <= 17) return make_shape(o.c, 127);
  MsmShape best = make_shape(16, 127);
  for (int cc = 13; cc <= 17; cc++) { const MsmShape s = make_shape(cc, 127); if (single_msm_cost(2 * n, s, 127) < single_msm_cost(2 * n, best, 127)) best = s; }
  return best;
}
// The automatic rule of glv_applies (msm_host.hpp): the window model's products at least 4 % below the plain shape's (a margin for the
// split pass and for gathering from a table twice the size) — 2^19 .. 2^20 bases (c = 16 against c = 15: 8 x 2n against 17 x n mixed
// additions, -5.9 %); at 2^21 the model gains 2 %, at 2^22 and above the plain windows (c = 17, 15 x n) win.
static bool glv_pays(const MsmOverrides& o, size_t n, const MsmShape& plain) {
  return single_msm_cost(2 * n, glv_shape(o, n), 127) * 1.04 < single_msm_cost(n, plain, 254);
}

// ---- accumulate and reduction of P problems (windows or rows) of nb buckets and `estride` sorted entries each ----
struct AccPlan {
  uint32_t SEG; int LPB;                   // segment length a bucket's entry list is cut into; lanes per bucket of k_acc_first
  int L, chunks, levels; bool quad;        // buckets per lane of k_reduce_l1; chunks (waves) per problem; k_reduce_combine launches, by the quad-cooperative kernel or not
  size_t max_extra, max_big;               // capacity of the segment work list and of the list of cut buckets
};
// segment length: twice the mean bucket load (power of two, >= 32)
static uint32_t acc_seg(size_t P, size_t estride, size_t nb) {
  const size_t NB = P * nb, mean = estride / nb + 1;
  uint32_t SEG = 32; while (SEG < 2 * mean && SEG < ACC_SEG_MAX) SEG <<= 1;
  // enough segments to fill the chip when a problem has few, heavily loaded buckets (one row, many columns)
  if (NB < 262144) { const size_t total = P * estride; uint32_t cap = 32; while ((size_t)cap * 262144 < total && cap < ACC_SEG_MAX) cap <<= 1; if (SEG > cap) SEG = cap; }
  return SEG;
}
static void acc_set_seg(AccPlan& a, uint32_t SEG, size_t P, size_t estride, size_t nb) { a.SEG = SEG; a.max_extra = P * estride / SEG + 1; a.max_big = std::min(P * nb, a.max_extra); }
// n: the records of a problem as the digit kernel counts them (DigitArgs::n)
static AccPlan acc_plan(int mode, size_t n, size_t P, size_t estride, int nb, const MsmOverrides& o) {
  AccPlan a; const size_t NB = P * (size_t)nb, mean = estride / (size_t)nb + 1;
  uint32_t SEG = acc_seg(P, estride, (size_t)nb);
  if (mode == MODE_SINGLE && n >= 512 && n <= 4096) SEG = 8;       // small single MSMs: short chains, the partials folded by k_acc_merge (choose_shape)
  if (o.seg) SEG = (uint32_t)o.seg;
  acc_set_seg(a, SEG, P, estride, (size_t)nb);
  // lanes per bucket (k_acc_first<G>): chains of ~32 mixed additions when the buckets are loaded enough to be split
  // (only while one lane per bucket would leave the chip short of lanes: at 2^22, c = 17 — 983 k buckets of 64 points — two lanes per bucket accumulate no
  //  faster (4.74 against 4.77 ms) and make the reduction read two slots per bucket: k_reduce_l1 0.53 against 0.37 ms)
  a.LPB = 1; if (mode == MODE_SINGLE && mean >= 48 && NB <= ((size_t)1 << 19)) a.LPB = 2;
  // Buckets per lane (L) of the reduction's first level.  A chunk (one wave, 64 lanes x L buckets) costs a chain of about (2 L - 1) + L (LPB - 1) + 10
  // additions (running sums, the LPB partial sums of a bucket, the wave's scan and tree) and keeps its SIMD's issue slots busy for all of it, so the
  // level takes ceil(waves / SIMDs) such chains: L is chosen to minimise that — NOT a power of two in general (2^20 points: 17 windows x 2^14 buckets
  // with L = 4 are 1 088 waves on 1 024 SIMDs, i.e. 64 SIMDs with two chains, 274 us; L = 5 with a ragged last chunk are 884 waves, one chain each).
  // Many buckets (millions): the chip holds two waves per SIMD and the level is throughput-bound: the power-of-two rule stays.
  int L = 1; while ((size_t)L * 64 * 2048 < NB && L < 16) L <<= 1;
  if (L < 4) L = 4;
  if (L > nb / 64) L = nb / 64;
  if (L < 1) L = 1;
  if (NB <= (size_t)64 * 16 * 1024) {
    double best = 1e300; int bl = L;
    for (int t = 1; t <= 32 && t * 64 <= std::max(nb, 64); t++) {
      const size_t waves = P * (size_t)((nb + 64 * t - 1) / (64 * t));
      const double cost = (double)((waves + 1023) / 1024) * (double)((2 * t - 1) + t * (a.LPB - 1) + 10);
      if (cost < best) { best = cost; bl = t; }
    }
    L = bl;
  }
  a.L = o.red_l ? o.red_l : L;
  a.chunks = (nb + 64 * a.L - 1) / (64 * a.L);      // per problem, >= 1; the last one may be ragged
  a.levels = 1; for (int G = (a.chunks + 63) / 64; G > 1; G = (G + 63) / 64) a.levels++;     // each launch folds 64 partial sums into one
  // The combine level of a job with few chunks (a single MSM of ~2^20 points, small commits) is a latency chain on a nearly empty chip: the
  // quad-cooperative kernel (256 threads per group of 64 chunks, 3.5 instead of 7.6 us per dependent addition) runs it in 0.115 instead of
  // 0.141 ms at 2^20.  Level 1 stays one wave per chunk: measured with quads 0.35 - 0.38 ms against 0.277 at L = 4 / 8 / 16 (level 1 is SIMD-issue
  // bound, not a latency chain: four times the waves at 2.3x the instructions only make the queues longer; profiles/r04_reduce_quad_sweep.txt).
  a.quad = P * (size_t)a.chunks <= 2048;
  return a;
}

// ---- one-level LDS counting sort (msm_kernels.cuh: k_hist_lds / k_scatter_lds): R counter ranges of RS buckets, K entry chunks per problem ----
struct Sort1Plan { int RS, logRS, R, K; size_t chunk; };
static Sort1Plan sort1_plan(int sort_rs_max, size_t P, size_t estride, int nb) {
  Sort1Plan g;
  g.RS = std::min(nb, sort_rs_max); g.logRS = 0; while ((1 << g.logRS) < g.RS) g.logRS++;
  g.R = nb / g.RS;
  { size_t want = (1024 + P * g.R - 1) / (P * g.R); size_t maxk = std::max<size_t>(1, estride / 4096); g.K = (int)std::max<size_t>(1, std::min(want, maxk)); }
  g.chunk = (estride + g.K - 1) / g.K;
  return g;
}

// ---- two-level sort of a large single MSM (sort2_kernels.cuh) ----
enum { S2_PLAN_OK = 0, S2_PLAN_TOO_WIDE, S2_PLAN_COUNTERS };   // TOO_WIDE: no split of the window fits; COUNTERS: W x P level-1 counters exceed k_s2_count's LDS
constexpr size_t S2_COUNT_LDS_BYTES = (size_t)24 * S2_P_MAX * 4;   // k_s2_count keeps W * P counters: up to 24 windows x S2_P_MAX partitions (SBN_SORT2_LO can push P to the maximum with a narrow window)
struct Sort2Plan { int status, lo_log, P, spt, K; size_t max_sc; };
static Sort2Plan sort2_plan(size_t n, const MsmShape& s, const MsmOverrides& o) {
  Sort2Plan g; g.status = S2_PLAN_OK; g.P = g.spt = g.K = 0; g.max_sc = 0;
  // bucket index = hi (level 1, <= 1024 partitions) | lo (level 2, <= 2048 LDS counters): runs of 8192 / P entries leave level 1,
  // runs of tile / 2^lo_log leave level 2
  g.lo_log = std::max(s.c - 1 - 8, 8); if (g.lo_log > S2_LO_LOG_MAX) g.lo_log = S2_LO_LOG_MAX;
  if (o.s2_lo) g.lo_log = o.s2_lo;
  if (s.c - 1 - g.lo_log < 0) g.lo_log = s.c - 1;
  while ((s.nb >> g.lo_log) > S2_P_MAX) g.lo_log++;
  if (g.lo_log > S2_LO_LOG_MAX) { g.status = S2_PLAN_TOO_WIDE; return g; }
  g.P = s.nb >> g.lo_log;
  // scalars per level-1 block: 8192, or 2048 while that still leaves runs of >= 32 entries per partition (P <= 64: windows up to 15 bits) and the
  // input is small enough for 8192 to mean few blocks: a 2^20 MSM (c = 15) starts 512 blocks of 1024 threads instead of 128 (k_s2_count + k_s2_scatter
  // 26 + 96 -> 18 + 68 us); at 2^21 / 2^22 (c = 17, P = 256: runs of 8) the small blocks lose (sort 0.42 / 0.83 against 0.33 / 0.64 ms).  SBN_SORT2_SPT = 2 / 8 overrides
  g.spt = (n <= ((size_t)1 << 21) && g.P <= 64) ? S2_SPT_SMALL : S2_SPT;
  if (o.s2_spt) g.spt = o.s2_spt;
  const size_t ch = (size_t)1024 * g.spt, WP = (size_t)s.W * g.P;
  g.K = (int)((n + ch - 1) / ch);
  g.max_sc = ((size_t)s.W * n) / S2_SUB + WP;          // sum over partitions of ceil(cnt / S2_SUB), cnt summing to <= W n
  if (WP * 4 > S2_COUNT_LDS_BYTES) g.status = S2_PLAN_COUNTERS;
  return g;
}

// ---- lookup-table row commits (comb_kernels.cuh): blocks per row ----
// few rows (latency-bound regime): spread a row over S blocks so that a lane takes at most two table points — the block
// sums are log-depth quad-cooperative additions (3.5 us a level), cheaper than a third chained mixed addition (5.4 us)
static unsigned comb_split(size_t L, size_t ncol, int W, const MsmOverrides& o) {
  unsigned S = 1;
  if ((size_t)L * 64 < 2048 && ncol * (size_t)W > 1024) {
    S = (unsigned)std::min<size_t>(128, (ncol * (size_t)W + 511) / 512);
    while (S > 1 && (size_t)L * S > 4096) S--;
  }
  if (o.comb_s) S = (unsigned)o.comb_s;
  return S;
}

}  // namespace sbn
