// The verifiers' host arithmetic (csrc/verify_host.hpp) as a stand-alone program: one case per line of stdin, one line of results per case.
// tests/test_verify_host_cpu.py builds it under ASan + UBSan and compares every line with tests/polyeval_verify_model.py, tests/polyeval_model.py,
// tests/transcript_model.py and plain integers.  Every argument is hex ("-" for no bytes) or a decimal count.
//   valid XY64                   -> 1 / 0 of g1_xy_valid
//   norm C32                     -> the 32 bytes of g1_compressed_normalise
//   frneg S32                    -> the 32 bytes of fr_neg_bytes
//   g1neg XY64                   -> the 64 bytes of g1_neg_bytes, then 1 / 0 of g1_is_identity of the input
//   devmont X32                  -> the 32 bytes of fq_to_dev_mont
//   shape ELL                    -> ell ml mr L_size n lg np of opening_shape
//   eq M R                       -> the 2^M scalars of polyeval_host_eq over the M coordinates R
//   joint LABEL EVALS LC L_EVALS L_CHAL L_CLAIM R ELL_R      (a transcript begun with LABEL; 2^LC evals)
//                                -> rj, claim, the 203-byte state
//   opening LABEL CXY128 RV N COMP LG R_RIGHT Z1 Z2         (polyeval_verify_script, then polyeval_verify_scalars on its challenges)
//                                -> 1 / 0, rq, cc, u, u^-1, a_hat, nz1, nz2, tail, the 2 LG + 4 scalars of hs, the 203-byte state
#include "../spartan-bn254_amd/csrc/verify_host.hpp"
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

using namespace sbn_host;

static std::vector<uint8_t> unhex(const std::string& s) {
  std::vector<uint8_t> v;
  if (s == "-") return v;
  if (s.size() % 2) { fprintf(stderr, "odd hex: %s\n", s.c_str()); exit(2); }
  for (size_t i = 0; i < s.size(); i += 2) v.push_back((uint8_t)std::stoul(s.substr(i, 2), nullptr, 16));
  return v;
}
static std::string hex(const void* q, size_t n) {
  static const char* d = "0123456789abcdef";
  const uint8_t* p = (const uint8_t*)q;
  std::string s;
  for (size_t i = 0; i < n; i++) { s += d[p[i] >> 4]; s += d[p[i] & 15]; }
  return n ? s : std::string("-");
}
static std::string state(const MerlinTranscript& t) {
  uint8_t rec[203]; memcpy(rec, t.s.st, 200); rec[200] = t.s.pos; rec[201] = t.s.pos_begin; rec[202] = t.s.cur_flags;
  return hex(rec, 203);
}
static std::string els(const std::vector<fr::El>& v) {
  std::vector<uint8_t> b(32 * v.size());
  for (size_t i = 0; i < v.size(); i++) memcpy(&b[32 * i], v[i].v, 32);
  return hex(b.data(), b.size());
}

int main() {
  std::string line;
  while (std::getline(std::cin, line)) {
    std::istringstream in(line);
    std::string cmd; in >> cmd;
    auto bytes = [&](size_t want) {
      std::string w; if (!(in >> w)) { fprintf(stderr, "bad case: %s\n", line.c_str()); exit(2); }
      std::vector<uint8_t> v = unhex(w);
      if (want != (size_t)-1 && v.size() != want) { fprintf(stderr, "bad length in: %s\n", line.c_str()); exit(2); }
      return v;
    };
    auto count = [&]() { size_t n = 0; if (!(in >> n)) { fprintf(stderr, "bad case: %s\n", line.c_str()); exit(2); } return n; };
    if (cmd == "valid") {
      const std::vector<uint8_t> p = bytes(64);
      puts(g1_xy_valid(p.data()) ? "1" : "0");
    } else if (cmd == "norm") {
      const std::vector<uint8_t> p = bytes(32); uint8_t o[32];
      g1_compressed_normalise(p.data(), o);
      puts(hex(o, 32).c_str());
    } else if (cmd == "frneg") {
      const std::vector<uint8_t> p = bytes(32); uint8_t o[32];
      fr_neg_bytes(p.data(), o);
      puts(hex(o, 32).c_str());
    } else if (cmd == "g1neg") {
      const std::vector<uint8_t> p = bytes(64); uint8_t o[64];
      g1_neg_bytes(p.data(), o);
      printf("%s %d\n", hex(o, 64).c_str(), g1_is_identity(p.data()) ? 1 : 0);
    } else if (cmd == "devmont") {
      const std::vector<uint8_t> p = bytes(32);
      const Fq v = fq_to_dev_mont(p.data());
      puts(hex(v.v, 32).c_str());
    } else if (cmd == "shape") {
      const OpeningShape s = opening_shape(count());
      printf("%zu %zu %zu %zu %zu %zu %zu\n", s.ell, s.ml, s.mr, s.L_size, s.n, s.lg, s.np);
    } else if (cmd == "eq") {
      const size_t m = count();
      const std::vector<uint8_t> r = bytes(32 * m);
      std::vector<uint8_t> out;
      polyeval_host_eq(r.data(), m, out);
      if (out.size() != ((size_t)32 << m)) { fprintf(stderr, "eq: %zu bytes\n", out.size()); return 2; }
      puts(hex(out.data(), out.size()).c_str());
    } else if (cmd == "joint") {
      const std::vector<uint8_t> label = bytes((size_t)-1), evals = bytes((size_t)-1);
      const size_t lc = count();
      if (evals.size() != ((size_t)32 << lc)) { fprintf(stderr, "joint: %zu bytes of evals\n", evals.size()); return 2; }
      const std::vector<uint8_t> le = bytes((size_t)-1), lh = bytes((size_t)-1), ll = bytes((size_t)-1), r = bytes((size_t)-1);
      const size_t ell_r = count();
      if (r.size() != 32 * ell_r) { fprintf(stderr, "joint: %zu bytes of r\n", r.size()); return 2; }
      MerlinTranscript t; t.init(label.data(), label.size());
      std::vector<uint8_t> rj; uint8_t claim[32];
      joint_reduce(evals.data(), (size_t)1 << lc, lc, Label(le.data(), le.size()), Label(lh.data(), lh.size()), Label(ll.data(), ll.size()), ell_r ? r.data() : nullptr, ell_r, t, rj, claim);
      if (rj.size() != 32 * (lc + ell_r)) { fprintf(stderr, "joint: %zu bytes of rj\n", rj.size()); return 2; }
      printf("%s %s %s\n", hex(rj.data(), rj.size()).c_str(), hex(claim, 32).c_str(), state(t).c_str());
    } else if (cmd == "opening") {
      const std::vector<uint8_t> label = bytes((size_t)-1), Cxy = bytes(128), Rv = bytes((size_t)-1);
      const size_t n = count();
      const std::vector<uint8_t> comp = bytes((size_t)-1);
      const size_t lg = count();
      if (Rv.size() != 32 * n || comp.size() != 32 * (2 * lg + 2)) { fprintf(stderr, "opening: bad sizes\n"); return 2; }
      const std::vector<uint8_t> rr = bytes(32 * lg), z1 = bytes(32), z2 = bytes(32);
      MerlinTranscript t; t.init(label.data(), label.size());
      Script ts{t};
      uint8_t rq[32], cc[32];
      std::vector<fr::El> u, ui;
      if (!polyeval_verify_script(ts, Cxy.data(), Rv.data(), n, comp.data(), lg, rq, cc, u, ui)) { printf("0 %s\n", state(t).c_str()); continue; }
      std::vector<uint8_t> hs(32 * (2 * lg + 4));
      const PolyevalFinal f = polyeval_verify_scalars(rr.data(), lg, u, ui, rq, cc, z1.data(), z2.data(), hs.data());
      printf("1 %s %s %s %s %s %s %s %s %s %s\n", hex(rq, 32).c_str(), hex(cc, 32).c_str(), els(u).c_str(), els(ui).c_str(), hex(f.a_hat.v, 32).c_str(), hex(f.nz1.v, 32).c_str(),
             hex(f.nz2.v, 32).c_str(), hex(f.tail.v, 32).c_str(), hex(hs.data(), hs.size()).c_str(), state(t).c_str());
    } else { fprintf(stderr, "unknown case: %s\n", line.c_str()); return 2; }
  }
  puts("VERIFY HOST CHECK DONE");
  return 0;
}
