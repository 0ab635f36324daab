// What NIZK::prove / verify add around R1CSProof on the host (csrc/snark_host.hpp: nizk_prefix, nizk_sizes) as a stand-alone program: one case per line
// of stdin, one line of results per case.  tests/test_nizk_host_cpu.py builds it under ASan + UBSan and compares every line with tests/nizk_model.py
// and tests/transcript_model.py.  Every argument is hex ("-" for no bytes) or a decimal number.
//   prefix LABEL DIGEST     -> the 203-byte transcript state after each of the two lines (a digest of no bytes is passed as NULL, length 0)
//   sizes NC NV NI          -> r1cs_proof rnd_scalars proof_bytes at the padded shape, or "refused"
#include "../spartan-bn254_amd/csrc/snark_host.hpp"
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
static std::string state(const MerlinTranscript& t) {
  static const char* d = "0123456789abcdef";
  uint8_t rec[203]; memcpy(rec, t.s.st, 200); rec[200] = t.s.pos; rec[201] = t.s.pos_begin; rec[202] = t.s.cur_flags;
  std::string s;
  for (uint8_t b : rec) { s += d[b >> 4]; s += d[b & 15]; }
  return s;
}

int main() {
  std::string line;
  while (std::getline(std::cin, line)) {
    std::istringstream in(line);
    std::string cmd; in >> cmd;
    auto bytes = [&]() { std::string w; if (!(in >> w)) { fprintf(stderr, "bad case: %s\n", line.c_str()); exit(2); } return unhex(w); };
    auto num = [&]() { size_t n = 0; if (!(in >> n)) { fprintf(stderr, "bad case: %s\n", line.c_str()); exit(2); } return n; };
    if (cmd == "prefix") {
      const std::vector<uint8_t> label = bytes(), digest = bytes();
      const std::vector<uint8_t> exact(digest.begin(), digest.end());      // a buffer of exactly the digest's length: ASan sees a read past its end
      MerlinTranscript t; t.init(label.data(), label.size());
      Script ts{t};
      std::string res;
      snark::nizk_prefix(ts, exact.empty() ? nullptr : exact.data(), exact.size(), [&]() { res += (res.empty() ? "" : " ") + state(t); });
      puts(res.c_str());
    } else if (cmd == "sizes") {
      const size_t a = num(), b = num(), c = num();
      snark::Shape s;
      if (!snark::shape_make(a, b, c, &s)) { puts("refused"); continue; }
      const snark::NizkSizes z = snark::nizk_sizes(s);
      printf("%zu %zu %zu\n", z.r1cs_proof, z.rnd_scalars, z.proof_bytes);
    } else { fprintf(stderr, "unknown case: %s\n", line.c_str()); return 2; }
  }
  puts("NIZK HOST CHECK DONE");
  return 0;
}
