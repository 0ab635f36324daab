// The host half of a .ptau file as the KZG SRS (csrc/ptau_host.hpp: scan, g2_convert) as a stand-alone program: one case per line of stdin, one line of
// results per case (`prefixes`: one per prefix).  tests/test_ptau_host_cpu.py builds it under ASan + UBSan and compares every line with tests/ptau_model.py.
// The bytes are passed as hex ("-" for none) and copied into a heap buffer of exactly their length, so that ASan sees a read past the end.
//   ptau FILE      -> "ok" power ceremonyPower n_g1 n_g2 off_g1 off_g2 G2_XY TAU_G2_XY   (tauG2[1] converted first, then tauG2[0], as the load does)   or "refused" CODE
//   prefixes FILE  -> the `ptau` line of FILE[:n] for n = 0 .. len - 1, each prefix in a buffer of its own
//   g2 BYTES128    -> "ok" XY                                                             or "refused" CODE
#include "../spartan-bn254_amd/csrc/ptau_host.hpp"
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <memory>
#include <sstream>
#include <string>

using namespace sbn_host;

static const char* const CODE[] = {"ok", "short", "magic", "version", "section_past_end", "duplicate_section", "missing_section", "header_size", "n8", "prime",
                                   "power", "g1_size", "g2_size", "g2_not_canonical", "g2_identity", "g2_off_curve", "g2_not_in_subgroup"};

static std::string hex(const uint8_t* b, size_t n) {
  static const char* d = "0123456789abcdef";
  std::string s;
  for (size_t i = 0; i < n; i++) { s += d[b[i] >> 4]; s += d[b[i] & 15]; }
  return s;
}

static void ptau_line(const uint8_t* b, size_t len) {
  ptau::Scan s;
  uint8_t g2[128], tau_g2[128];
  int e = ptau::scan(b, len, &s);
  if (!e) e = ptau::g2_convert(b + s.off_g2 + 128, tau_g2);
  if (!e) e = ptau::g2_convert(b + s.off_g2, g2);
  if (e) { printf("refused %s\n", CODE[e]); return; }
  printf("ok %u %u %llu %llu %zu %zu %s %s\n", s.power, s.ceremony_power, (unsigned long long)s.n_g1, (unsigned long long)s.n_g2, s.off_g1, s.off_g2,
         hex(g2, 128).c_str(), hex(tau_g2, 128).c_str());
}

int main() {
  std::string line;
  while (std::getline(std::cin, line)) {
    std::istringstream in(line);
    std::string cmd, hx; in >> cmd >> hx;
    if (hx.empty() || (hx != "-" && hx.size() % 2)) { fprintf(stderr, "bad case: %s\n", line.substr(0, 80).c_str()); return 2; }
    const size_t len = hx == "-" ? 0 : hx.size() / 2;
    std::unique_ptr<uint8_t[]> buf(new uint8_t[len]);                  // exactly len bytes (new uint8_t[0] is a valid, unreadable pointer)
    for (size_t i = 0; i < len; i++) buf[i] = (uint8_t)std::stoul(hx.substr(2 * i, 2), nullptr, 16);
    if (cmd == "ptau") ptau_line(buf.get(), len);
    else if (cmd == "prefixes") {
      for (size_t n = 0; n < len; n++) {
        std::unique_ptr<uint8_t[]> p(new uint8_t[n]);
        memcpy(p.get(), buf.get(), n);
        ptau_line(p.get(), n);
      }
    } else if (cmd == "g2" && len == 128) {
      uint8_t xy[128];
      const int e = ptau::g2_convert(buf.get(), xy);
      if (e) printf("refused %s\n", CODE[e]); else printf("ok %s\n", hex(xy, 128).c_str());
    } else { fprintf(stderr, "unknown case: %s\n", line.substr(0, 80).c_str()); return 2; }
  }
  puts("PTAU HOST CHECK DONE");
  return 0;
}
