// The host half of the circuit digest (csrc/circom_host.hpp: digest_leaves, digest_leaf, digest_root — the root is what sbn_circom_r1cs_digest runs over
// the leaves the device made) as a stand-alone program: one circuit per line of stdin, one digest per line.  tests/test_circuit_digest_cpu.py builds it under
// ASan + UBSan and compares every line with tests/circuit_digest_model.py.  Every array is a heap buffer of exactly its length.
//   S0 S1 S2 S3 S4 NNZ0 NNZ1 NNZ2 ENTRIES     the five shape fields, the three counts, then nnz0 + nnz1 + nnz2 entries as hex: u32le row | u32le col | val[32]
//                                              ("-" for none)
//   -> the root as hex, then the leaves of the three matrices as one hex string ("-" for none)
#include "../spartan-bn254_amd/csrc/circom_host.hpp"
#include <cstdio>
#include <iostream>
#include <memory>
#include <sstream>
#include <string>
#include <vector>

using namespace sbn_host;

int main() {
  std::string line;
  while (std::getline(std::cin, line)) {
    std::istringstream in(line);
    uint64_t shape[5], nnz[3];
    std::string hex;
    for (auto& x : shape) in >> x;
    for (auto& x : nnz) in >> x;
    in >> hex;
    const size_t total = (size_t)(nnz[0] + nnz[1] + nnz[2]);
    if (!in || (hex == "-" ? 0 : hex.size()) != 80 * total) { fprintf(stderr, "bad case: %s\n", line.c_str()); return 2; }
    std::unique_ptr<uint32_t[]> rows(new uint32_t[total]), cols(new uint32_t[total]);
    std::unique_ptr<uint8_t[]> vals(new uint8_t[32 * total]);
    for (size_t e = 0; e < total; e++) {
      uint8_t b[40];
      for (int i = 0; i < 40; i++) b[i] = (uint8_t)std::stoul(hex.substr(80 * e + 2 * i, 2), nullptr, 16);
      rows[e] = circom::get_u32(b); cols[e] = circom::get_u32(b + 4);
      memcpy(vals.get() + 32 * e, b + 8, 32);
    }
    std::unique_ptr<uint8_t[]> lv[3];
    const uint8_t* lp[3];
    std::string leaves_hex;
    size_t off = 0;
    for (int m = 0; m < 3; m++) {
      const size_t nl = circom::digest_leaves(nnz[m]);
      lv[m].reset(new uint8_t[32 * nl]);                              // exactly the matrix's leaves
      for (size_t j = 0; j < nl; j++) {
        const size_t e0 = off + circom::DIGEST_LEAF_ENTRIES * j, left = (size_t)nnz[m] - circom::DIGEST_LEAF_ENTRIES * j;
        const uint32_t k = (uint32_t)(left < circom::DIGEST_LEAF_ENTRIES ? left : circom::DIGEST_LEAF_ENTRIES);
        circom::digest_leaf((uint8_t)m, j, k, rows.get() + e0, cols.get() + e0, vals.get() + 32 * e0, lv[m].get() + 32 * j);
      }
      char b[3];
      for (size_t i = 0; i < 32 * nl; i++) { snprintf(b, sizeof b, "%02x", lv[m][i]); leaves_hex += b; }
      lp[m] = lv[m].get();
      off += (size_t)nnz[m];
    }
    uint8_t root[32];
    circom::digest_root(shape, nnz, lp, root);
    for (int i = 0; i < 32; i++) printf("%02x", root[i]);
    printf(" %s\n", leaves_hex.empty() ? "-" : leaves_hex.c_str());
  }
  puts("CIRCUIT DIGEST CHECK DONE");
  return 0;
}
