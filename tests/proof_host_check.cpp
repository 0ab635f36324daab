// The provers' transcript script (csrc/proof_host.hpp) as a stand-alone program: one case per line of stdin, one line of results per case.
// tests/test_proof_host_cpu.py builds it under ASan + UBSan and compares every line with tests/transcript_model.py and plain integers.
// Every argument is hex ("-" for no bytes) or a decimal count.
//   wide B64                     -> the 32 bytes of transcript_wide_reduce
//   fmul A32 B32                 -> the 32 bytes of fr::fmul
//   script LABEL OP ARGS ...     -> per operation on a transcript begun with LABEL: [OUT:]STATE, the 203-byte state after it
//     protocol NAME | scalar LABEL P32 | scalars LABEL DATA N | point LABEL C32 | point_xy LABEL XY64 (OUT: the compressed point)
//     message LABEL MSG (the label as bytes and length) | challenge LABEL (OUT: the scalar) | challenges LABEL N (OUT: the N scalars)
#include "../spartan-bn254_amd/csrc/proof_host.hpp"
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
static std::string hex(const uint8_t* p, size_t n) {
  static const char* d = "0123456789abcdef";
  std::string s;
  for (size_t i = 0; i < n; i++) { s += d[p[i] >> 4]; s += d[p[i] & 15]; }
  return s;
}
static std::string state(const MerlinTranscript& t) {
  uint8_t rec[203]; memcpy(rec, t.s.st, 200); rec[200] = t.s.pos; rec[201] = t.s.pos_begin; rec[202] = t.s.cur_flags;
  return hex(rec, 203);
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
    auto text = [&]() { const std::vector<uint8_t> v = bytes((size_t)-1); return std::string(v.begin(), v.end()); };      // a label or name without NUL bytes
    auto count = [&]() { size_t n = 0; if (!(in >> n)) { fprintf(stderr, "bad case: %s\n", line.c_str()); exit(2); } return n; };
    if (cmd == "wide") {
      const std::vector<uint8_t> b = bytes(64); uint8_t out[32];
      transcript_wide_reduce(b.data(), out);
      puts(hex(out, 32).c_str());
    } else if (cmd == "fmul") {
      const std::vector<uint8_t> a = bytes(32), b = bytes(32);
      fr::El x, y; memcpy(x.v, a.data(), 32); memcpy(y.v, b.data(), 32);
      const fr::El z = fr::fmul(x, y);
      puts(hex((const uint8_t*)z.v, 32).c_str());
    } else if (cmd == "script") {
      const std::vector<uint8_t> label = bytes((size_t)-1);
      MerlinTranscript t; t.init(label.data(), label.size());
      Script s{t};
      std::string op, res;
      while (in >> op) {
        std::string out;
        if (op == "protocol") { const std::string name = text(); s.protocol(name.c_str()); }
        else if (op == "scalar") { const std::string l = text(); const std::vector<uint8_t> p = bytes(32); s.scalar(l.c_str(), p.data()); }
        else if (op == "scalars") { const std::string l = text(); const std::vector<uint8_t> p = bytes((size_t)-1); const size_t n = count(); if (p.size() != 32 * n) exit(2); s.scalars(l.c_str(), p.data(), n); }
        else if (op == "point") { const std::string l = text(); const std::vector<uint8_t> p = bytes(32); s.point(l.c_str(), p.data()); }
        else if (op == "point_xy") { const std::string l = text(); const std::vector<uint8_t> p = bytes(64); uint8_t o[32]; s.point_xy(l.c_str(), p.data(), o); out = hex(o, 32); }
        else if (op == "message") { const std::vector<uint8_t> l = bytes((size_t)-1), m = bytes((size_t)-1); s.message(Label(l.data(), l.size()), m.data(), m.size()); }
        else if (op == "challenge") { const std::string l = text(); uint8_t o[32]; s.challenge(l.c_str(), o); out = hex(o, 32); }
        else if (op == "challenges") { const std::string l = text(); const size_t n = count(); std::vector<uint8_t> o(32 * n); s.challenges(l.c_str(), o.data(), n); out = n ? hex(o.data(), o.size()) : "-"; }
        else { fprintf(stderr, "unknown operation: %s\n", op.c_str()); return 2; }
        res += (res.empty() ? "" : " ") + (out.empty() ? "" : out + ":") + state(t);
      }
      puts(res.c_str());
    } else { fprintf(stderr, "unknown case: %s\n", line.c_str()); return 2; }
  }
  puts("PROOF HOST CHECK DONE");
  return 0;
}
