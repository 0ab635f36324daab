// The field and transcript half of the sparse evaluation check (csrc/sparse_verify_host.hpp) as a stand-alone program: one case per line of
// stdin, one line of results per case.  tests/test_sparse_verify_host_cpu.py builds it under ASan + UBSan and compares every line with
// tests/sparse_eval_model.py.  Every argument is hex ("-" for no bytes) or a decimal count; a refusal prints "0".
//   layout NX NY N B             -> "1" and the 14 field offsets, or "0"
//   canon NX NY N B PROOF        -> "1" when the proof has the layout's length and every scalar of it is below r
//   product STATE203 NUM_OPS NUM_CELLS EVALS EVAL_ROW EVAL_COL EVAL_VAL PROOF_MEM PROOF_OPS
//                                -> "1" claims_mem rand_mem claims_ops claims_dotp rand_ops STATE203
//   hash B EVAL_ROW EVAL_COL EVAL_VAL EVAL_DEREFS CLAIMS_MEM RAND_MEM CLAIMS_OPS CLAIMS_DOTP RX RY R_HASH R_MULTISET
//                                -> "1" evals_derefs evals_ops evals_mem
#include "../spartan-bn254_amd/csrc/sparse_verify_host.hpp"
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

using namespace sbn_host;
using spv::El;

static std::vector<uint8_t> unhex(const std::string& s) {
  std::vector<uint8_t> v;
  if (s == "-") return v;
  if (s.size() % 2) { fprintf(stderr, "odd hex: %s\n", s.c_str()); exit(2); }
  for (size_t i = 0; i < s.size(); i += 2) v.push_back((uint8_t)std::stoul(s.substr(i, 2), nullptr, 16));
  return v;
}
static std::string hex(const uint8_t* p, size_t n) {
  static const char* d = "0123456789abcdef";
  if (!n) return "-";
  std::string s;
  for (size_t i = 0; i < n; i++) { s += d[p[i] >> 4]; s += d[p[i] & 15]; }
  return s;
}
static std::string hex(const std::vector<El>& v) { return hex(v.empty() ? nullptr : (const uint8_t*)v.data(), 32 * v.size()); }
static std::string hex(const std::vector<uint8_t>& v) { return hex(v.data(), v.size()); }
static std::string state(const MerlinTranscript& t) {
  uint8_t rec[203]; memcpy(rec, t.s.st, 200); rec[200] = t.s.pos; rec[201] = t.s.pos_begin; rec[202] = t.s.cur_flags;
  return hex(rec, 203);
}
// canonical scalars, as the caller of the header has them
static std::vector<El> els(const std::vector<uint8_t>& b) {
  std::vector<El> v;
  if (b.size() % 32 || !spv::els_load(b.data(), b.size() / 32, &v)) { fprintf(stderr, "bad scalars\n"); exit(2); }
  return v;
}

int main() {
  std::string line;
  while (std::getline(std::cin, line)) {
    std::istringstream in(line);
    std::string cmd; in >> cmd;
    auto bytes = [&]() {
      std::string w; if (!(in >> w)) { fprintf(stderr, "bad case: %s\n", line.substr(0, 80).c_str()); exit(2); }
      return unhex(w);
    };
    auto count = [&]() { size_t n = 0; if (!(in >> n)) { fprintf(stderr, "bad case: %s\n", line.substr(0, 80).c_str()); exit(2); } return n; };
    auto span = [](const std::vector<uint8_t>& v) { return spv::Span{v.data(), v.size()}; };
    if (cmd == "layout" || cmd == "canon") {
      const size_t nx = count(), ny = count(), N = count(), b = count();
      spv::Layout L;
      if (!spv::layout_make(nx, ny, N, b, &L)) { puts("0"); continue; }
      if (cmd == "layout") {
        std::string s = "1";
        for (int f = 0; f <= spv::NFIELDS; f++) s += " " + std::to_string(L.off[f]);
        puts(s.c_str());
      } else {
        const std::vector<uint8_t> proof = bytes();
        puts(proof.size() == L.off[spv::NFIELDS] && spv::proof_scalars_canonical(L, proof.data()) ? "1" : "0");
      }
    } else if (cmd == "product") {
      const std::vector<uint8_t> st = bytes();
      if (st.size() != 203) { fprintf(stderr, "bad state\n"); return 2; }
      MerlinTranscript t; memcpy(t.s.st, st.data(), 200); t.s.pos = st[200]; t.s.pos_begin = st[201]; t.s.cur_flags = st[202];
      const size_t num_ops = count(), num_cells = count();
      const std::vector<uint8_t> evals = bytes(), er = bytes(), ec = bytes(), ev = bytes(), pm = bytes(), po = bytes();
      if (evals.size() % 32) { fprintf(stderr, "bad evals\n"); return 2; }
      Script ts{t};
      spv::ProductFields f{span(er), span(ec), span(ev), span(pm), span(po)};
      spv::ProductClaims pc;
      if (!spv::product_layer_verify(ts, f, num_ops, num_cells, evals.data(), evals.size() / 32, &pc)) { puts("0"); continue; }
      puts(("1 " + hex(pc.claims_mem) + " " + hex(pc.rand_mem) + " " + hex(pc.claims_ops) + " " + hex(pc.claims_dotp) + " " + hex(pc.rand_ops) + " " + state(t)).c_str());
    } else if (cmd == "hash") {
      const size_t b = count();
      const std::vector<uint8_t> er = bytes(), ec = bytes(), ev = bytes(), ed = bytes();
      spv::ProductClaims pc;
      pc.claims_mem = els(bytes()); pc.rand_mem = els(bytes()); pc.claims_ops = els(bytes()); pc.claims_dotp = els(bytes());
      const std::vector<El> rx = els(bytes()), ry = els(bytes()), rh = els(bytes()), rm = els(bytes());
      if (rx.size() != pc.rand_mem.size() || ry.size() != pc.rand_mem.size() || rh.size() != 1 || rm.size() != 1) { fprintf(stderr, "bad point\n"); return 2; }
      spv::HashFields f{span(er), span(ec), span(ev), span(ed)};
      spv::JointEvals je;
      if (!spv::hash_layer_field(f, b, pc, rx.data(), ry.data(), rh[0], rm[0], &je)) { puts("0"); continue; }
      puts(("1 " + hex(je.derefs) + " " + hex(je.ops) + " " + hex(je.mem)).c_str());
    } else { fprintf(stderr, "unknown case: %s\n", line.substr(0, 80).c_str()); return 2; }
  }
  puts("SPARSE VERIFY HOST CHECK DONE");
  return 0;
}
