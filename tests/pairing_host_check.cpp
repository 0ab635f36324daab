// pairing_host_check.cpp — pairing_host.hpp alone, as a stand-alone program (tests/test_pairing_host_cpu.py builds it under ASan + UBSan).
// One command a line on standard input, one answer a line on standard output:
//   table <256 hex>   ->  the canonical bytes of the point's line table, then one digit a line (square_first)     | "refused <code>"
//   parse <256 hex>   ->  the ParseResult of g2_parse_checked (0 ok, 1 not canonical, 2 identity, 3 off E', 4 outside the r-torsion)
//   mont  <256 hex>   ->  the same with the coordinates read as ark-ff Montgomery limbs
//   naf               ->  the schedule's digits, most significant first, as one string of '+', '-', '0'
#include "../spartan-bn254_amd/csrc/pairing_host.hpp"
#include <cstdio>
#include <iostream>
#include <string>

using namespace sbn_host::pairing;

static bool unhex(const std::string& s, uint8_t* out, size_t n) {
  if (s.size() != 2 * n) return false;
  for (size_t i = 0; i < n; i++) { unsigned v; if (sscanf(s.c_str() + 2 * i, "%2x", &v) != 1) return false; out[i] = (uint8_t)v; }
  return true;
}

int main() {
  std::string cmd;
  while (std::cin >> cmd) {
    if (cmd == "naf") {
      std::string o;
      for (int d : naf_schedule()) o += d > 0 ? '+' : d < 0 ? '-' : '0';
      printf("%s\n", o.c_str());
      continue;
    }
    std::string hex; std::cin >> hex;
    uint8_t b[128];
    if (!unhex(hex, b, 128)) { printf("bad input\n"); return 1; }
    G2 q;
    if (cmd == "parse" || cmd == "mont") { printf("%d\n", (int)g2_parse_checked(b, cmd == "mont", &q)); continue; }
    if (cmd != "table") { printf("bad command\n"); return 1; }
    const ParseResult r = g2_parse_checked(b, false, &q);
    std::vector<Line> t;
    if (r != G2_OK || !line_table(q, &t)) { printf("refused %d\n", (int)r); continue; }
    std::vector<uint8_t> out(LINE_BYTES * t.size()), dev(LINE_BYTES * t.size());
    std::vector<uint32_t> sq(t.size());
    lines_to_canonical(t, out.data());
    lines_to_device(t, dev.data(), sq.data());
    for (uint8_t x : out) printf("%02x", x);
    printf(" ");
    for (uint32_t s : sq) printf("%u", s);
    printf(" ");
    for (uint8_t x : dev) printf("%02x", x);
    printf("\n");
  }
  printf("PAIRING HOST CHECK DONE\n");
  return 0;
}
