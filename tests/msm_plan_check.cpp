// The host's planning rules (csrc/msm_plan.hpp) as a stand-alone program: one case per line of stdin, one line of results per case.
// tests/test_msm_plan_cpu.py builds it under ASan + UBSan and compares every line with tests/acc_model.py / window_model.py.
// A case may end in NAME=VALUE words: the SBN_* overrides it runs under, set in the environment and read through msm_overrides_read.
//   const                                  -> NAME=value ...
//   shape c bits                           -> c W nb
//   choose terms shared cmax problems chard -> c
//   glv n                                  -> c W
//   acc mode n P estride nb                -> SEG LPB L chunks levels quad max_extra max_big
//   sort1 sort_rs_max P estride nb         -> RS logRS R K chunk
//   sort2 n c bits                         -> status lo_log P spt K max_sc W
#include "../spartan-bn254_amd/csrc/msm_plan.hpp"
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

using namespace sbn;

static const char* const NAMES[] = {"SBN_MSM_C", "SBN_MSM_SEG", "SBN_RED_L", "SBN_SORT2_LO", "SBN_SORT2_SPT", "SBN_COMB_S"};

int main() {
  std::string line;
  while (std::getline(std::cin, line)) {
    std::istringstream in(line);
    std::string cmd, word; in >> cmd;
    std::vector<unsigned long long> a;
    for (const char* n : NAMES) unsetenv(n);
    while (in >> word) {
      const size_t eq = word.find('=');
      if (eq == std::string::npos) a.push_back(std::stoull(word));
      else setenv(word.substr(0, eq).c_str(), word.substr(eq + 1).c_str(), 1);
    }
    const MsmOverrides o = msm_overrides_read();
    auto need = [&](size_t k) { if (a.size() != k) { fprintf(stderr, "bad case: %s\n", line.c_str()); exit(2); } };
    if (cmd == "const") {
      printf("MSM_C_MAX=%d ACC_SEG_MAX=%u MERGE_LANE_MAX=%u S2_C_MIN=%d S2_C_MAX=%d S2_P_MAX=%d S2_LO_LOG_MAX=%d S2_SPT=%d S2_SPT_SMALL=%d S2_SUB=%u COMB_C_MAX=%d MODE_SINGLE=%d MODE_ROWS=%d\n",
             MSM_C_MAX, ACC_SEG_MAX, MERGE_LANE_MAX, S2_C_MIN, S2_C_MAX, S2_P_MAX, S2_LO_LOG_MAX, S2_SPT, S2_SPT_SMALL, S2_SUB, COMB_C_MAX, (int)MODE_SINGLE, (int)MODE_ROWS);
    } else if (cmd == "shape") {
      need(2); const MsmShape s = make_shape((int)a[0], (int)a[1]);
      printf("%d %d %d\n", s.c, s.W, s.nb);
    } else if (cmd == "choose") {
      need(5); printf("%d\n", choose_shape(o, a[0], a[1] != 0, (int)a[2], a[3], (int)a[4]).c);
    } else if (cmd == "glv") {
      need(1); const MsmShape s = glv_shape(o, a[0]);
      printf("%d %d\n", s.c, s.W);
    } else if (cmd == "acc") {
      need(5); const AccPlan p = acc_plan((int)a[0], a[1], a[2], a[3], (int)a[4], o);
      printf("%u %d %d %d %d %d %zu %zu\n", p.SEG, p.LPB, p.L, p.chunks, p.levels, p.quad ? 1 : 0, p.max_extra, p.max_big);
    } else if (cmd == "sort1") {
      need(4); const Sort1Plan p = sort1_plan((int)a[0], a[1], a[2], (int)a[3]);
      printf("%d %d %d %d %zu\n", p.RS, p.logRS, p.R, p.K, p.chunk);
    } else if (cmd == "sort2") {
      need(3); const MsmShape s = make_shape((int)a[1], (int)a[2]); const Sort2Plan p = sort2_plan(a[0], s, o);
      printf("%d %d %d %d %d %zu %d\n", p.status, p.lo_log, p.P, p.spt, p.K, p.max_sc, s.W);
    } else { fprintf(stderr, "unknown case: %s\n", line.c_str()); return 2; }
  }
  puts("MSM PLAN CHECK DONE");
  return 0;
}
