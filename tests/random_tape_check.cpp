// The RandomTape and the draw plans (csrc/random_tape_host.hpp) as a stand-alone program: one tape per line of stdin, one line of draws per tape.
// tests/test_random_tape_cpu.py builds it under ASan + UBSan and compares every line with tests/random_tape_model.py.  Every plan writes into a heap
// buffer of exactly its count, so that ASan sees a draw too many.
//   NAME INIT OP...     NAME, INIT: hex ("-" for no bytes; INIT is 32 bytes); the OPs run one after the other on the one tape:
//     raw LABEL N            N x challenge_scalar(LABEL)          (LABEL: hex, "-" for the empty label)
//     zk ROUNDS N            plan_zk_sumcheck
//     pe LG                  plan_polyeval
//     pe_beta LG             plan_polyeval with r_beta drawn under b"r_beta": NOT the reference's label
//     r1cs L NX NY LG        plan_r1cs_proof
//     se LGD LGO LGM KZG     plan_sparse_eval
//   -> the draws of all OPs as one hex string ("-" for none)
#include "../spartan-bn254_amd/csrc/random_tape_host.hpp"
#include <cstdio>
#include <iostream>
#include <memory>
#include <sstream>
#include <string>
#include <vector>

using namespace sbn_host;

static std::vector<uint8_t> unhex(const std::string& h) {
  std::vector<uint8_t> out;
  if (h == "-") return out;
  for (size_t i = 0; i + 1 < h.size(); i += 2) out.push_back((uint8_t)std::stoul(h.substr(i, 2), nullptr, 16));
  return out;
}

int main() {
  std::string line;
  while (std::getline(std::cin, line)) {
    std::istringstream in(line);
    std::string name_h, init_h, op;
    in >> name_h >> init_h;
    const std::vector<uint8_t> name = unhex(name_h), init = unhex(init_h);
    if (init.size() != 32) { fprintf(stderr, "bad case: %s\n", line.c_str()); return 2; }
    tape::RandomTape T;
    static const uint8_t NONE[1] = {0};
    T.init(name.empty() ? NONE : name.data(), name.size(), init.data());
    std::string out;
    auto emit = [&](const uint8_t* p, size_t n) { char b[3]; for (size_t i = 0; i < 32 * n; i++) { snprintf(b, sizeof b, "%02x", p[i]); out += b; } };
    while (in >> op) {
      size_t a[4] = {0, 0, 0, 0}, count = 0;
      std::string label_h;
      if (op == "raw") { in >> label_h >> a[0]; count = a[0]; }
      else if (op == "zk") { in >> a[0] >> a[1]; count = tape::count_zk_sumcheck(a[0], a[1]); }
      else if (op == "pe" || op == "pe_beta") { in >> a[0]; count = tape::count_polyeval(a[0]); }
      else if (op == "r1cs") { in >> a[0] >> a[1] >> a[2] >> a[3]; count = tape::count_r1cs_proof(a[0], a[1], a[2], a[3]); }
      else if (op == "se") { in >> a[0] >> a[1] >> a[2] >> a[3]; count = tape::count_sparse_eval(a[0], a[1], a[2], a[3] != 0); }
      else { fprintf(stderr, "unknown op: %s\n", op.c_str()); return 2; }
      if (!in) { fprintf(stderr, "bad case: %s\n", line.c_str()); return 2; }
      std::unique_ptr<uint8_t[]> buf(new uint8_t[32 * count]);        // exactly the plan's count
      uint8_t* end = buf.get() + 32 * count;
      if (op == "raw") { const std::vector<uint8_t> l = unhex(label_h); T.draw(Label(l.empty() ? NONE : l.data(), l.size()), buf.get(), count); }
      else if (op == "zk") end = tape::plan_zk_sumcheck(T, a[0], a[1], buf.get());
      else if (op == "pe") end = tape::plan_polyeval(T, a[0], buf.get());
      else if (op == "pe_beta") end = tape::plan_polyeval(T, a[0], buf.get(), "r_beta");
      else if (op == "r1cs") end = tape::plan_r1cs_proof(T, a[0], a[1], a[2], a[3], buf.get());
      else end = tape::plan_sparse_eval(T, a[0], a[1], a[2], a[3] != 0, buf.get());
      if (end != buf.get() + 32 * count) { fprintf(stderr, "%s: the plan wrote %td bytes, its count says %zu\n", op.c_str(), end - buf.get(), 32 * count); return 3; }
      emit(buf.get(), count);
    }
    T.wipe();
    for (size_t i = 0; i < sizeof T; i++) if (((const uint8_t*)&T)[i]) { fprintf(stderr, "wipe left byte %zu\n", i); return 3; }
    printf("%s\n", out.empty() ? "-" : out.c_str());
  }
  puts("RANDOM TAPE CHECK DONE");
  return 0;
}
