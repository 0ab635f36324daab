// The host half of the circom readers (csrc/circom_host.hpp: r1cs_scan, r1cs_walk, wtns_scan, shape_of) as a stand-alone program: one case per line of stdin,
// one line of results per case.  tests/test_circom_host_cpu.py builds it under ASan + UBSan and compares every line with tests/circom_model.py.  The file
// is passed as hex ("-" for no bytes) and copied into a heap buffer of exactly its length, so that ASan sees a read past its end.
//   r1cs FILE   -> "ok" field_size nWires nPubOut nPubIn nPrvIn nLabels nConstraints num_pub payload_off payload_len num_vars num_inputs nc_padded nv_padded
//                  nnzA nnzB nnzC | run_first... | mat_first...        or "refused" CODE
//   wtns FILE   -> "ok" offset count                                    or "refused" CODE
#include "../spartan-bn254_amd/csrc/circom_host.hpp"
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <memory>
#include <sstream>
#include <string>
#include <vector>

using namespace sbn_host;

static const char* const CODE[] = {"ok", "io", "magic", "version", "no_header", "no_constraints", "field_size", "prime", "wires", "section_end", "too_many", "twice", "none", "size"};

int main() {
  std::string line;
  while (std::getline(std::cin, line)) {
    std::istringstream in(line);
    std::string cmd, hex; in >> cmd >> hex;
    if (hex.empty() || (hex != "-" && hex.size() % 2)) { fprintf(stderr, "bad case: %s\n", line.c_str()); return 2; }
    const size_t len = hex == "-" ? 0 : hex.size() / 2;
    std::unique_ptr<uint8_t[]> buf(new uint8_t[len]);                  // exactly len bytes (new uint8_t[0] is a valid, unreadable pointer)
    for (size_t i = 0; i < len; i++) buf[i] = (uint8_t)std::stoul(hex.substr(2 * i, 2), nullptr, 16);
    if (cmd == "r1cs") {
      circom::R1csScan s;
      int e = circom::r1cs_scan(buf.get(), len, &s);
      std::vector<uint32_t> rf, mf; uint64_t nnz[3] = {0, 0, 0};
      snark::Shape sh;
      if (!e) e = circom::r1cs_walk(buf.get(), s, rf, mf, nnz);
      if (e) { printf("refused %s\n", CODE[e]); continue; }
      if (!circom::shape_of(s, &sh)) { puts("refused shape"); continue; }
      printf("ok %u %llu %llu %llu %llu %llu %llu %llu %zu %zu %zu %zu %zu %zu %llu %llu %llu |", s.field_size, (unsigned long long)s.n_wires, (unsigned long long)s.n_pub_out,
             (unsigned long long)s.n_pub_in, (unsigned long long)s.n_prv_in, (unsigned long long)s.n_labels, (unsigned long long)s.n_cons, (unsigned long long)s.n_pub, s.payload_off,
             s.payload_len, sh.num_vars, sh.num_inputs, sh.nc, sh.nv, (unsigned long long)nnz[0], (unsigned long long)nnz[1], (unsigned long long)nnz[2]);
      for (uint32_t x : rf) printf(" %u", x);
      printf(" |");
      for (uint32_t x : mf) printf(" %u", x);
      printf("\n");
    } else if (cmd == "wtns") {
      circom::WtnsSpan w;
      const int e = circom::wtns_scan(buf.get(), len, &w);
      if (e) printf("refused %s\n", CODE[e]); else printf("ok %zu %zu\n", w.off, w.count);
    } else { fprintf(stderr, "unknown case: %s\n", line.c_str()); return 2; }
  }
  puts("CIRCOM HOST CHECK DONE");
  return 0;
}
