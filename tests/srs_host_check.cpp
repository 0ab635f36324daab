// The host half of the KZG SRS file (csrc/srs_host.hpp: scan, g2_decompress, g2_compress, g2_from_tau) as a stand-alone program: one case per line of
// stdin, one line of results per case.  tests/test_srs_host_cpu.py builds it under ASan + UBSan and compares every line with tests/srs_model.py.  The
// bytes are passed as hex ("-" for none) and copied into a heap buffer of exactly their length, so that ASan sees a read past the end.
//   srs FILE    -> "ok" n tau_g2_off g2_off TAU_G2_XY G2_XY TAU_G2_AGAIN G2_AGAIN   (the two points decompressed, then compressed again)   or "refused" CODE
//   g2 BYTES64  -> "ok" XY AGAIN                                                     or "refused" CODE
//   tau BYTES32 -> "ok" G2_XY TAU_G2_XY                                              or "refused tau"
#include "../spartan-bn254_amd/csrc/srs_host.hpp"
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <memory>
#include <sstream>
#include <string>

using namespace sbn_host;

static const char* const CODE[] = {"ok", "short", "empty", "g2_not_canonical", "g2_flags", "g2_identity", "g2_off_curve", "g2_not_in_subgroup"};

static std::string hex(const uint8_t* b, size_t n) {
  static const char* d = "0123456789abcdef";
  std::string s;
  for (size_t i = 0; i < n; i++) { s += d[b[i] >> 4]; s += d[b[i] & 15]; }
  return s;
}
// decompress, print the canonical point, compress it again: 0 or the refusal
static int g2_round_trip(const uint8_t* in, std::string* out) {
  uint8_t xy[128], again[64];
  int e = srs::g2_decompress(in, xy);
  if (!e) e = srs::g2_compress(xy, false, again);
  if (!e) *out = hex(xy, 128) + " " + hex(again, 64);
  return e;
}

int main() {
  std::string line;
  while (std::getline(std::cin, line)) {
    std::istringstream in(line);
    std::string cmd, hx; in >> cmd >> hx;
    if (hx.empty() || (hx != "-" && hx.size() % 2)) { fprintf(stderr, "bad case: %s\n", line.c_str()); return 2; }
    const size_t len = hx == "-" ? 0 : hx.size() / 2;
    std::unique_ptr<uint8_t[]> buf(new uint8_t[len]);                  // exactly len bytes (new uint8_t[0] is a valid, unreadable pointer)
    for (size_t i = 0; i < len; i++) buf[i] = (uint8_t)std::stoul(hx.substr(2 * i, 2), nullptr, 16);
    if (cmd == "srs") {
      srs::Scan s;
      int e = srs::scan(buf.get(), len, &s);
      std::string a, b;
      if (!e) e = g2_round_trip(buf.get() + s.tau_g2_off, &a);
      if (!e) e = g2_round_trip(buf.get() + s.g2_off, &b);
      if (e) { printf("refused %s\n", CODE[e]); continue; }
      const std::string ta = a.substr(0, 256), tb = a.substr(257), ga = b.substr(0, 256), gb = b.substr(257);
      printf("ok %llu %zu %zu %s %s %s %s\n", (unsigned long long)s.n, s.tau_g2_off, s.g2_off, ta.c_str(), ga.c_str(), tb.c_str(), gb.c_str());
    } else if (cmd == "g2" && len == 64) {
      std::string a;
      const int e = g2_round_trip(buf.get(), &a);
      if (e) printf("refused %s\n", CODE[e]); else printf("ok %s\n", a.c_str());
    } else if (cmd == "tau" && len == 32) {
      uint8_t g[128], t[128];
      if (!srs::g2_from_tau(buf.get(), g, t)) puts("refused tau"); else printf("ok %s %s\n", hex(g, 128).c_str(), hex(t, 128).c_str());
    } else { fprintf(stderr, "unknown case: %s\n", line.c_str()); return 2; }
  }
  puts("SRS HOST CHECK DONE");
  return 0;
}
