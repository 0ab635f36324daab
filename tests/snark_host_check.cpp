// What SNARK::encode / prove / verify add around their two halves on the host (csrc/snark_host.hpp) as a stand-alone program: one case per line of
// stdin, one line of results per case.  tests/test_snark_host_cpu.py builds it under ASan + UBSan and compares every line with tests/snark_model.py
// and tests/transcript_model.py.  Every argument is hex ("-" for no bytes) or a decimal number.
//   shape NC NV NI                      -> nc nv nx ny, or "refused"
//   convert NC NV NI ROWS COLS VALS     -> CODE BAD COLS': rows / cols as little-endian u32, vals 32 bytes each; CODE 0 ok, 1 row, 2 col, 3 val
//   build NC NV NI N OPS MEM            -> the commitment's bytes (OPS / MEM: the compressed points; their count is checked against the shape)
//   parse COMM                          -> CODE nc nv ni batch N cells L_ops L_mem (the numbers only with CODE 0)
//   prefix LABEL COMM                   -> the 203-byte transcript state after every line of the prefix
//   sizes COMM KZG                      -> r1cs_rnd r1cs_proof eval_rnd eval_proof rnd_scalars proof_bytes
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
static std::string hex(const uint8_t* p, size_t n) {
  static const char* d = "0123456789abcdef";
  std::string s;
  for (size_t i = 0; i < n; i++) { s += d[p[i] >> 4]; s += d[p[i] & 15]; }
  return n ? s : "-";
}
static std::string state(const MerlinTranscript& t) {
  uint8_t rec[203]; memcpy(rec, t.s.st, 200); rec[200] = t.s.pos; rec[201] = t.s.pos_begin; rec[202] = t.s.cur_flags;
  return hex(rec, 203);
}
static std::vector<uint32_t> words(const std::vector<uint8_t>& b) {
  if (b.size() % 4) { fprintf(stderr, "u32 array of %zu bytes\n", b.size()); exit(2); }
  std::vector<uint32_t> w(b.size() / 4);
  if (!w.empty()) memcpy(w.data(), b.data(), b.size());
  return w;
}

int main() {
  std::string line;
  while (std::getline(std::cin, line)) {
    std::istringstream in(line);
    std::string cmd; in >> cmd;
    auto bytes = [&]() { std::string w; if (!(in >> w)) { fprintf(stderr, "bad case: %s\n", line.c_str()); exit(2); } return unhex(w); };
    auto num = [&]() { size_t n = 0; if (!(in >> n)) { fprintf(stderr, "bad case: %s\n", line.c_str()); exit(2); } return n; };
    auto shape = [&](snark::Shape* s) { const size_t a = num(), b = num(), c = num(); return snark::shape_make(a, b, c, s); };
    if (cmd == "shape") {
      snark::Shape s;
      if (!shape(&s)) puts("refused");
      else printf("%zu %zu %zu %zu\n", s.nc, s.nv, s.nx, s.ny);
    } else if (cmd == "convert") {
      snark::Shape s;
      if (!shape(&s)) { puts("refused"); continue; }
      const std::vector<uint32_t> rows = words(bytes()), cols = words(bytes());
      const std::vector<uint8_t> vals = bytes();
      if (rows.size() != cols.size() || vals.size() != 32 * rows.size()) { fprintf(stderr, "bad lengths in: %s\n", line.c_str()); return 2; }
      std::vector<uint32_t> out(rows.size());                      // exactly nnz entries: ASan sees a write past the end
      size_t bad = 0;
      const int e = snark::convert_cols(s, rows.data(), cols.data(), vals.data(), rows.size(), out.data(), &bad);
      printf("%d %zu %s\n", e, bad, e ? "-" : hex((const uint8_t*)out.data(), 4 * out.size()).c_str());
    } else if (cmd == "build") {
      snark::Shape s;
      if (!shape(&s)) { puts("refused"); continue; }
      const size_t N = num();
      const std::vector<uint8_t> ops = bytes(), mem = bytes();
      const snark::Comm c = snark::comm_of(s, N);
      if (ops.size() != 32 * c.L_ops || mem.size() != 32 * c.L_mem) { printf("lengths %zu %zu\n", c.L_ops, c.L_mem); continue; }
      const std::vector<uint8_t> b = snark::comm_build(c, ops.data(), mem.data());
      puts(hex(b.data(), b.size()).c_str());
    } else if (cmd == "parse") {
      const std::vector<uint8_t> b = bytes();
      const std::vector<uint8_t> exact(b.begin(), b.end());        // a buffer of exactly the given length
      snark::Comm c;
      const int e = snark::comm_parse(exact.data(), exact.size(), &c);
      if (e) printf("%d\n", e);
      else printf("0 %llu %llu %llu %llu %llu %llu %zu %zu\n", (unsigned long long)c.nc, (unsigned long long)c.nv, (unsigned long long)c.ni, (unsigned long long)c.batch,
                  (unsigned long long)c.N, (unsigned long long)c.cells, c.L_ops, c.L_mem);
    } else if (cmd == "prefix") {
      const std::vector<uint8_t> label = bytes(), b = bytes();
      snark::Comm c;
      if (snark::comm_parse(b.data(), b.size(), &c)) { puts("refused"); continue; }
      MerlinTranscript t; t.init(label.data(), label.size());
      Script ts{t};
      std::string res;
      snark::prefix(ts, c, b.data(), [&]() { res += (res.empty() ? "" : " ") + state(t); });
      puts(res.c_str());
    } else if (cmd == "sizes") {
      const std::vector<uint8_t> b = bytes();
      const size_t kzg = num();
      snark::Comm c;
      if (snark::comm_parse(b.data(), b.size(), &c)) { puts("refused"); continue; }
      const snark::Sizes z = snark::sizes(c, kzg != 0);
      printf("%zu %zu %zu %zu %zu %zu\n", z.r1cs_rnd, z.r1cs_proof, z.eval_rnd, z.eval_proof, z.rnd_scalars, z.proof_bytes);
    } else { fprintf(stderr, "unknown case: %s\n", line.c_str()); return 2; }
  }
  puts("SNARK HOST CHECK DONE");
  return 0;
}
