// The proof-file reader and writer of harness/sbn_spartan.cpp (harness/standalone_host.hpp) as a stand-alone program: one file per line of stdin, one line
// of results per file.  tests/test_standalone_host_cpu.py builds it under ASan + UBSan.  The file is passed as hex ("-" for no bytes) and copied into a heap
// buffer of exactly its length, so that ASan sees a read past its end.
//   FILE WANT_MODE WANT_KZG   (-1: whatever the file says)
//   -> "ok" mode kzg num_cons num_vars num_inputs num_nz_entries DIGEST INPUTS PROOF rewrite   (hex, "-" for none; rewrite: "same" when write_proof_file of what was
//      read gives the file's bytes back)      or "refused" CODE
#include "../spartan-bn254_amd/harness/standalone_host.hpp"
#include <cstdio>
#include <iostream>
#include <memory>
#include <sstream>
#include <string>

using namespace sbn_standalone;

static const char* const CODE[] = {"ok", "short", "magic", "version", "mode", "kzg", "reserved", "length", "input", "trailing", "mode_mismatch", "kzg_mismatch"};

static std::string hex(const std::vector<uint8_t>& v) {
  if (v.empty()) return "-";
  std::string s; char b[3];
  for (uint8_t x : v) { snprintf(b, sizeof b, "%02x", x); s += b; }
  return s;
}

int main() {
  std::string line;
  while (std::getline(std::cin, line)) {
    std::istringstream in(line);
    std::string h; int wm = -1, wk = -1;
    in >> h >> wm >> wk;
    if (!in || (h != "-" && h.size() % 2)) { fprintf(stderr, "bad case: %s\n", line.c_str()); return 2; }
    const size_t len = h == "-" ? 0 : h.size() / 2;
    std::unique_ptr<uint8_t[]> buf(new uint8_t[len]);
    for (size_t i = 0; i < len; i++) buf[i] = (uint8_t)std::stoul(h.substr(2 * i, 2), nullptr, 16);
    ProofFile f;
    const int e = read_proof_file(buf.get(), len, wm, wk, &f);
    if (e) { printf("refused %s\n", CODE[e]); continue; }
    const std::vector<uint8_t> again = write_proof_file(f);
    const bool same = again.size() == len && (len == 0 || memcmp(again.data(), buf.get(), len) == 0);
    printf("ok %u %u %llu %llu %llu %llu %s %s %s %s\n", f.mode, f.kzg, (unsigned long long)f.num_cons, (unsigned long long)f.num_vars, (unsigned long long)f.num_inputs,
           (unsigned long long)f.num_nz_entries, hex(f.digest).c_str(), hex(f.inputs).c_str(), hex(f.proof).c_str(), same ? "same" : "differs");
  }
  puts("STANDALONE HOST CHECK DONE");
  return 0;
}
