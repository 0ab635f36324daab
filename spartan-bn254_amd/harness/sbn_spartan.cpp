// sbn_spartan — a compiled caller of the C ABI (plain g++, no HIP) that takes files: circom's .r1cs and .wtns in, a commitment and a proof file out, and back
// through verify, on one MI355X with no Rust anywhere.  What the reference's examples/keyless_benchmark.rs does: files in, stage times, proof-size breakdown, verify.
//
//   sbn_spartan info   C.r1cs                                   the sbn_circom_info fields and the circuit digest in hex
//   sbn_spartan encode C.r1cs -o C.comm [--srs F]               the sbn_snark_key_comm bytes (--srs: the file is loaded and checked to be long enough)
//   sbn_spartan prove  --mode snark|nizk C.r1cs W.wtns -o P.sbnp [--srs F] [--check-sat] [--label L] [--tape-init HEX]
//   sbn_spartan verify --mode snark C.comm P.sbnp [--srs F] [--label L]
//   sbn_spartan verify --mode nizk  C.r1cs P.sbnp [--label L]
//   sbn_spartan info   F.ptau                                   the sbn_ptau_info fields of a powers-of-tau ceremony file (host only)
//   sbn_spartan srs    F.ptau -o F.srs [--n N] [--check]        the first N powers (default: all) as the reference's SRS file (sbn_kzg_srs_save)
//
// prove: both files are loaded onto the device, then gens, then encode (snark) or the NIZK instance under the DEVICE digest (sbn_circom_r1cs_digest: the
// library's own, not the reference's get_digest), then tape -> draw plan -> one prove call; the proof file (standalone_host.hpp) holds the raw shape, the
// inputs and the proof, so verify takes inputs and shape from it.  The transcript label defaults to "keyless_snark" (keyless_benchmark.rs:166).
// --srs: the KZG build, through sbn_kzg_srs_load, sbn_derefs_key_build and the _kzg calls.  A file that begins with "ptau" is a ceremony file: it is
// mapped, not read, and goes through sbn_kzg_srs_load_ptau, which takes the prefix the circuit needs (npo2(2 batch) N powers for encode and prove, known
// once the circuit is encoded; one power for verify, which needs the two G2 points only).
// --tape-init HEX (64 hex digits, a canonical scalar, little-endian) fixes the prover's randomness.  IT EXISTS FOR TESTS: a proof made with a known init has
// known blinds and hides nothing.  Without it the tape is seeded from the operating system.
// Exit status: 0 done or accepted; 1 proof refused; 2 usage, file or library error (sbn_last_error on stderr); 3 the witness does not satisfy the circuit
// under --check-sat (the count and the first violated constraint on stderr).
#include "../../include/sbn254.h"
#include "standalone_host.hpp"
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>
#include <fcntl.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>

namespace sa = sbn_standalone;

namespace {

struct Fail { int status; std::string text; };
[[noreturn]] void die(int status, const std::string& text) { throw Fail{status, text}; }

struct Handles {                                   // everything the run holds, released in the order the header asks for
  sbn_ctx* ctx = nullptr;
  sbn_circom_r1cs* circ = nullptr;
  sbn_snark_gens* gens = nullptr;
  sbn_snark_key* key = nullptr;
  sbn_nizk_inst* inst = nullptr;
  sbn_table* vars = nullptr;
  sbn_bases* srs = nullptr;
  sbn_g2_lines *g2 = nullptr, *tau_g2 = nullptr;
  sbn_derefs_key* dkey = nullptr;
  sbn_random_tape* tape = nullptr;
  sbn_transcript* tr = nullptr;
  ~Handles() {
    if (tape) sbn_random_tape_free(tape);
    if (tr) sbn_transcript_free(tr);
    if (!ctx) return;
    if (dkey) sbn_derefs_key_free(ctx, dkey);
    if (vars) sbn_table_free(ctx, vars);
    if (inst) sbn_nizk_instance_free(ctx, inst);
    if (key) sbn_snark_key_free(ctx, key);
    if (gens) sbn_snark_gens_free(ctx, gens);
    if (circ) sbn_circom_r1cs_free(ctx, circ);
    if (g2) sbn_g2_lines_free(ctx, g2);
    if (tau_g2) sbn_g2_lines_free(ctx, tau_g2);
    if (srs) sbn_bases_free(ctx, srs);
    sbn_ctx_destroy(ctx);
  }
};

void check(const Handles& h, int rc, const char* what) {
  if (rc) die(2, std::string(what) + " failed (" + std::to_string(rc) + "): " + (h.ctx ? sbn_last_error(h.ctx) : ""));
}

std::vector<uint8_t> read_file(const std::string& path) {
  FILE* f = fopen(path.c_str(), "rb");
  if (!f) die(2, "cannot open " + path);
  std::vector<uint8_t> out; uint8_t buf[1 << 16]; size_t n;
  while ((n = fread(buf, 1, sizeof buf, f)) > 0) out.insert(out.end(), buf, buf + n);
  const bool bad = ferror(f) != 0;
  fclose(f);
  if (bad) die(2, "cannot read " + path);
  return out;
}
void write_file(const std::string& path, const std::vector<uint8_t>& data) {
  FILE* f = fopen(path.c_str(), "wb");
  if (!f) die(2, "cannot create " + path);
  const bool ok = fwrite(data.data(), 1, data.size(), f) == data.size();
  if (fclose(f) || !ok) die(2, "cannot write " + path);
}
struct Mapped {                                     // a file mapped read-only: a 32 GiB ceremony file costs the pages that are touched
  const uint8_t* p = nullptr; size_t len = 0;
  explicit Mapped(const std::string& path) {
    const int fd = open(path.c_str(), O_RDONLY);
    if (fd < 0) die(2, "cannot open " + path);
    struct stat st;
    if (fstat(fd, &st) || st.st_size < 0) { close(fd); die(2, "cannot read " + path); }
    len = (size_t)st.st_size;
    if (len) {
      void* m = mmap(nullptr, len, PROT_READ, MAP_PRIVATE, fd, 0);
      if (m == MAP_FAILED) { close(fd); die(2, "cannot map " + path); }
      p = (const uint8_t*)m;
    }
    close(fd);
  }
  ~Mapped() { if (p) munmap((void*)p, len); }
  Mapped(const Mapped&) = delete;
  Mapped& operator=(const Mapped&) = delete;
};
bool is_ptau(const std::string& path) {
  FILE* f = fopen(path.c_str(), "rb");
  if (!f) die(2, "cannot open " + path);
  char m[4] = {0, 0, 0, 0};
  const size_t got = fread(m, 1, 4, f);
  fclose(f);
  return got == 4 && !memcmp(m, "ptau", 4);
}
std::string hex(const uint8_t* p, size_t n) { std::string s; char b[3]; for (size_t i = 0; i < n; i++) { snprintf(b, sizeof b, "%02x", p[i]); s += b; } return s; }

struct Stages {                                     // per-stage wall times, printed in the order they ran
  std::vector<std::pair<std::string, double>> ms;
  std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
  void mark(const char* name) {
    const auto t1 = std::chrono::steady_clock::now();
    ms.emplace_back(name, std::chrono::duration<double, std::milli>(t1 - t0).count());
    t0 = t1;
  }
  void print() const { double sum = 0; for (const auto& s : ms) { printf("stage %-18s %10.3f ms\n", s.first.c_str(), s.second); sum += s.second; } printf("stage %-18s %10.3f ms\n", "total", sum); }
};

struct Args {
  std::string cmd, mode, out, srs, label = "keyless_snark", tape_init;
  bool check_sat = false, check_srs = false;
  size_t n = 0;
  std::vector<std::string> files;
};
const char USAGE[] =
    "usage: sbn_spartan info C.r1cs\n"
    "       sbn_spartan encode C.r1cs -o C.comm [--srs F]\n"
    "       sbn_spartan prove --mode snark|nizk C.r1cs W.wtns -o P.sbnp [--srs F] [--check-sat] [--label L] [--tape-init HEX (tests only)]\n"
    "       sbn_spartan verify --mode snark C.comm P.sbnp [--srs F] [--label L]\n"
    "       sbn_spartan verify --mode nizk C.r1cs P.sbnp [--label L]\n"
    "       sbn_spartan info F.ptau\n"
    "       sbn_spartan srs F.ptau -o F.srs [--n N] [--check]\n";

Args parse(int argc, char** argv) {
  Args a;
  if (argc < 2) die(2, USAGE);
  a.cmd = argv[1];
  for (int i = 2; i < argc; i++) {
    const std::string s = argv[i];
    auto value = [&]() -> std::string { if (i + 1 >= argc) die(2, s + " needs a value\n" + USAGE); return argv[++i]; };
    if (s == "--mode") a.mode = value();
    else if (s == "-o") a.out = value();
    else if (s == "--srs") a.srs = value();
    else if (s == "--label") a.label = value();
    else if (s == "--tape-init") a.tape_init = value();
    else if (s == "--check-sat") a.check_sat = true;
    else if (s == "--check") a.check_srs = true;
    else if (s == "--n") {
      const std::string v = value();
      if (v.empty() || v.size() > 18 || v.find_first_not_of("0123456789") != std::string::npos) die(2, "--n takes a count\n" + std::string(USAGE));
      a.n = (size_t)std::stoull(v);
    }
    else if (s.size() > 1 && s[0] == '-') die(2, "unknown option " + s + "\n" + USAGE);
    else a.files.push_back(s);
  }
  const size_t nfiles = a.cmd == "info" || a.cmd == "encode" || a.cmd == "srs" ? 1 : 2;
  if ((a.cmd != "info" && a.cmd != "encode" && a.cmd != "prove" && a.cmd != "verify" && a.cmd != "srs") || a.files.size() != nfiles) die(2, USAGE);
  if ((a.cmd == "prove" || a.cmd == "verify") && a.mode != "snark" && a.mode != "nizk") die(2, std::string("--mode snark|nizk is needed\n") + USAGE);
  if ((a.cmd == "encode" || a.cmd == "prove" || a.cmd == "srs") && a.out.empty()) die(2, std::string("-o is needed\n") + USAGE);
  if (a.mode == "nizk" && !a.srs.empty()) die(2, "--srs is the KZG build of snark mode: nizk mode has no commitment to open");
  return a;
}

void open_ctx(Handles& h) { if (sbn_ctx_create(0, &h.ctx)) { h.ctx = nullptr; die(2, "sbn_ctx_create failed: no usable gfx950 device"); } }

sbn_circom_info load_circuit(Handles& h, const std::string& path) {
  const std::vector<uint8_t> bytes = read_file(path);
  check(h, sbn_circom_r1cs_load(h.ctx, bytes.data(), bytes.size(), &h.circ), "sbn_circom_r1cs_load");
  sbn_circom_info info;
  check(h, sbn_circom_r1cs_info(h.circ, &info), "sbn_circom_r1cs_info");
  return info;
}
size_t max_nnz(const sbn_circom_info& i) { uint64_t m = i.nnz[0]; if (i.nnz[1] > m) m = i.nnz[1]; if (i.nnz[2] > m) m = i.nnz[2]; return (size_t)m; }

void load_srs(Handles& h, const std::string& path, bool want_g2) {
  const std::vector<uint8_t> bytes = read_file(path);
  size_t bad = 0;
  check(h, sbn_kzg_srs_load(h.ctx, bytes.data(), bytes.size(), 0, &h.srs, want_g2 ? &h.g2 : nullptr, want_g2 ? &h.tau_g2 : nullptr, nullptr, &bad), "sbn_kzg_srs_load");
}
// the first n powers (0: all) of a ceremony file; g2_xy (or NULL) receives g2 | tau_g2
void load_ptau(Handles& h, const std::string& path, size_t n, uint32_t flags, bool want_g2, uint8_t* g2_xy = nullptr) {
  const Mapped m(path);
  size_t bad = 0;
  check(h, sbn_kzg_srs_load_ptau(h.ctx, m.p, m.len, n, flags, &h.srs, want_g2 ? &h.g2 : nullptr, want_g2 ? &h.tau_g2 : nullptr, g2_xy, &bad), "sbn_kzg_srs_load_ptau");
}
// the powers the KZG build of this circuit touches: the derefs polynomial's padded length npo2(2 batch) N (sbn_sparse_eval_prove_kzg opens over one fewer)
size_t srs_powers_needed(const sbn_snark_key* key) {
  const sbn_dense* d = sbn_snark_key_dense(key);
  size_t k = 1;
  while (k < 2 * sbn_dense_batch(d)) k <<= 1;
  return k * sbn_dense_num_ops(d);
}

void new_transcript(Handles& h, const std::string& label) {
  if (sbn_transcript_new((const uint8_t*)label.data(), label.size(), &h.tr)) die(2, "sbn_transcript_new failed");
}

void new_tape(Handles& h, const char* name, const std::string& init_hex) {
  uint8_t init[32];
  if (!init_hex.empty()) {
    if (init_hex.size() != 64 || init_hex.find_first_not_of("0123456789abcdefABCDEF") != std::string::npos) die(2, "--tape-init takes 64 hex digits");
    for (int i = 0; i < 32; i++) init[i] = (uint8_t)std::stoul(init_hex.substr(2 * i, 2), nullptr, 16);
  }
  if (sbn_random_tape_new((const uint8_t*)name, strlen(name), init_hex.empty() ? nullptr : init, &h.tape))
    die(2, std::string("sbn_random_tape_new failed: ") + sbn_random_tape_last_error(nullptr));
}

void print_info(const sbn_circom_info& i, const uint8_t digest[32]) {
  printf("num_constraints %llu\nnum_variables %llu\nnum_pub_inputs %llu\nnum_prv_inputs %llu\nnum_labels %llu\n", (unsigned long long)i.num_constraints,
         (unsigned long long)i.num_variables, (unsigned long long)i.num_pub_inputs, (unsigned long long)i.num_prv_inputs, (unsigned long long)i.num_labels);
  printf("nnz %llu %llu %llu\ndropped %llu %llu %llu\n", (unsigned long long)i.nnz[0], (unsigned long long)i.nnz[1], (unsigned long long)i.nnz[2],
         (unsigned long long)i.dropped[0], (unsigned long long)i.dropped[1], (unsigned long long)i.dropped[2]);
  printf("num_vars %llu\nnum_cons_padded %llu\nnum_vars_padded %llu\n", (unsigned long long)i.num_vars, (unsigned long long)i.num_cons_padded, (unsigned long long)i.num_vars_padded);
  printf("digest %s\n", hex(digest, 32).c_str());
}

size_t log2z(uint64_t n) { size_t l = 0; while (((uint64_t)1 << l) < n) l++; return l; }

void print_spans(int mode, uint64_t nc_padded, uint64_t nv_padded, size_t proof_bytes) {
  size_t sat = 0;
  if (sbn_r1cs_proof_sizes((size_t)nc_padded, (size_t)nv_padded, nullptr, &sat)) return;
  for (const sa::Span& s : sa::proof_spans(mode, sat, log2z(nc_padded), log2z(2 * nv_padded), proof_bytes))
    printf("proof %-16s bytes %zu .. %zu (%zu)\n", s.name, s.first, s.end, s.end - s.first);
  printf("proof %-16s bytes %zu\n", "total", proof_bytes);
}

int run_ptau_info(const Args& a) {
  const Mapped m(a.files[0]);
  sbn_ptau_info i;
  if (sbn_ptau_scan(m.p, m.len, &i)) die(2, a.files[0] + " is not a .ptau file this library loads (sbn_ptau_scan)");
  printf("power %u\nceremonyPower %u\nn_g1 %llu\nn_g2 %llu\noff_g1 %llu\noff_g2 %llu\n", i.power, i.ceremony_power, (unsigned long long)i.n_g1, (unsigned long long)i.n_g2,
         (unsigned long long)i.off_g1, (unsigned long long)i.off_g2);
  return 0;
}

int run_srs(const Args& a) {
  Handles h; open_ctx(h);
  Stages st;
  uint8_t g2_xy[256];
  load_ptau(h, a.files[0], a.n, a.check_srs ? SBN_SRS_CHECK : 0, false, g2_xy); st.mark(a.check_srs ? "load_ptau+check" : "load_ptau");
  size_t len = 0;
  check(h, sbn_kzg_srs_save(h.ctx, h.srs, nullptr, nullptr, 0, nullptr, 0, &len), "sbn_kzg_srs_save");
  std::vector<uint8_t> out(len);
  check(h, sbn_kzg_srs_save(h.ctx, h.srs, g2_xy, g2_xy + 128, 0, out.data(), out.size(), &len), "sbn_kzg_srs_save"); st.mark("save");
  write_file(a.out, out); st.mark("write");
  st.print();
  printf("powers %zu\nsrs bytes %zu\n", sbn_bases_len(h.srs), len);
  return 0;
}

int run_info(const Args& a) {
  if (is_ptau(a.files[0])) return run_ptau_info(a);
  Handles h; open_ctx(h);
  const sbn_circom_info info = load_circuit(h, a.files[0]);
  uint8_t d[32];
  check(h, sbn_circom_r1cs_digest(h.ctx, h.circ, d), "sbn_circom_r1cs_digest");
  print_info(info, d);
  return 0;
}

int run_encode(const Args& a) {
  Handles h; open_ctx(h);
  Stages st;
  const sbn_circom_info info = load_circuit(h, a.files[0]); st.mark("load_r1cs");
  const bool ptau = !a.srs.empty() && is_ptau(a.srs);
  if (!a.srs.empty() && !ptau) { load_srs(h, a.srs, false); st.mark("load_srs"); }
  check(h, sbn_snark_gens_new(h.ctx, (size_t)info.num_constraints, (size_t)info.num_vars, (size_t)info.num_pub_inputs, max_nnz(info), &h.gens), "sbn_snark_gens_new"); st.mark("gens");
  check(h, sbn_snark_encode_circom(h.ctx, h.circ, h.gens, &h.key), "sbn_snark_encode_circom"); st.mark("encode");
  if (ptau) { load_ptau(h, a.srs, srs_powers_needed(h.key), 0, false); st.mark("load_srs"); }
  if (h.srs) { check(h, sbn_derefs_key_build(h.ctx, sbn_snark_key_dense(h.key), h.srs, &h.dkey), "sbn_derefs_key_build"); st.mark("derefs_key"); }
  size_t n = 0;
  check(h, sbn_snark_key_comm(h.key, nullptr, 0, &n), "sbn_snark_key_comm");
  std::vector<uint8_t> comm(n);
  check(h, sbn_snark_key_comm(h.key, comm.data(), n, &n), "sbn_snark_key_comm");
  write_file(a.out, comm); st.mark("write");
  st.print();
  printf("commitment bytes %zu\n", n);
  return 0;
}

int unsat(Handles& h, bool nizk, const uint8_t* input, size_t ni) {
  int sat = 1; uint64_t bad = 0, first = 0;
  check(h, nizk ? sbn_nizk_is_sat(h.ctx, h.inst, h.vars, input, ni, &sat, &bad, &first) : sbn_snark_is_sat(h.ctx, h.key, h.vars, input, ni, &sat, &bad, &first), "is_sat");
  fprintf(stderr, "sbn_spartan: the witness does not satisfy the circuit: %llu constraints violated, the first is constraint %llu\n", (unsigned long long)bad, (unsigned long long)first);
  return 3;
}

int run_prove(const Args& a) {
  const bool nizk = a.mode == "nizk", kzg = !a.srs.empty();
  Handles h; open_ctx(h);
  Stages st;
  const sbn_circom_info info = load_circuit(h, a.files[0]); st.mark("load_r1cs");
  const size_t nc = (size_t)info.num_constraints, nv = (size_t)info.num_vars, ni = (size_t)info.num_pub_inputs;
  sa::ProofFile pf;
  pf.mode = nizk ? sa::MODE_NIZK : sa::MODE_SNARK; pf.kzg = kzg ? 1 : 0;
  pf.num_cons = nc; pf.num_vars = nv; pf.num_inputs = ni; pf.num_nz_entries = max_nnz(info);
  pf.inputs.resize(32 * ni);
  {
    const std::vector<uint8_t> w = read_file(a.files[1]);
    size_t nwit = 0;
    check(h, sbn_circom_wtns_load(h.ctx, w.data(), w.size(), ni, &h.vars, pf.inputs.data(), &nwit), "sbn_circom_wtns_load");
    if (nwit != info.num_variables) die(2, "the witness holds " + std::to_string(nwit) + " values, the circuit has " + std::to_string(info.num_variables) + " wires");
  }
  st.mark("load_wtns");
  const bool ptau = kzg && is_ptau(a.srs);
  if (kzg && !ptau) { load_srs(h, a.srs, false); st.mark("load_srs"); }
  size_t n_rnd = 0, n_proof = 0;
  if (nizk) {
    check(h, sbn_nizk_gens_new(h.ctx, nc, nv, ni, &h.gens), "sbn_nizk_gens_new"); st.mark("gens");
    pf.digest.resize(32);
    check(h, sbn_circom_r1cs_digest(h.ctx, h.circ, pf.digest.data()), "sbn_circom_r1cs_digest"); st.mark("digest");
    check(h, sbn_nizk_instance_from_circom(h.ctx, h.circ, pf.digest.data(), 32, &h.inst), "sbn_nizk_instance_from_circom"); st.mark("instance");
    check(h, sbn_nizk_sizes(h.inst, &n_rnd, &n_proof), "sbn_nizk_sizes");
  } else {
    check(h, sbn_snark_gens_new(h.ctx, nc, nv, ni, (size_t)pf.num_nz_entries, &h.gens), "sbn_snark_gens_new"); st.mark("gens");
    check(h, sbn_snark_encode_circom(h.ctx, h.circ, h.gens, &h.key), "sbn_snark_encode_circom"); st.mark("encode");
    if (ptau) { load_ptau(h, a.srs, srs_powers_needed(h.key), 0, false); st.mark("load_srs"); }
    if (kzg) { check(h, sbn_derefs_key_build(h.ctx, sbn_snark_key_dense(h.key), h.srs, &h.dkey), "sbn_derefs_key_build"); st.mark("derefs_key"); }
    check(h, sbn_snark_sizes(h.key, kzg, &n_rnd, &n_proof), "sbn_snark_sizes");
  }
  new_tape(h, nizk ? "proof" : "snark_proof", a.tape_init);                     // snark.rs:210, :438
  std::vector<uint8_t> rnd(32 * n_rnd + 1);
  if (nizk ? sbn_nizk_draw_rnd(h.inst, h.tape, rnd.data(), n_rnd) : sbn_snark_draw_rnd(h.key, kzg, h.tape, rnd.data(), n_rnd))
    die(2, std::string("the draw plan failed: ") + sbn_random_tape_last_error(h.tape));
  st.mark("tape");
  new_transcript(h, a.label);
  pf.proof.resize(n_proof);
  const uint32_t flags = a.check_sat ? SBN_SNARK_CHECK_SAT : 0;
  const uint8_t* inp = ni ? pf.inputs.data() : nullptr;
  int rc;
  if (nizk) rc = sbn_nizk_prove(h.ctx, h.inst, h.vars, inp, ni, h.gens, flags, rnd.data(), h.tr, pf.proof.data());
  else if (kzg) rc = sbn_snark_prove_kzg(h.ctx, h.key, h.vars, inp, ni, h.gens, h.srs, h.dkey, flags, rnd.data(), h.tr, pf.proof.data());
  else rc = sbn_snark_prove(h.ctx, h.key, h.vars, inp, ni, h.gens, flags, rnd.data(), h.tr, pf.proof.data());
  for (auto& b : rnd) { volatile uint8_t* v = &b; *v = 0; }
  if (rc == SBN_EUNSAT) return unsat(h, nizk, inp, ni);
  check(h, rc, "prove");
  st.mark(a.check_sat ? "check_sat+prove" : "prove");
  write_file(a.out, sa::write_proof_file(pf)); st.mark("write");
  st.print();
  print_spans(pf.mode, info.num_cons_padded, info.num_vars_padded, n_proof);
  return 0;
}

int run_verify(const Args& a) {
  const bool nizk = a.mode == "nizk", kzg = !a.srs.empty();
  sa::ProofFile pf;
  {
    const std::vector<uint8_t> bytes = read_file(a.files[1]);
    const int e = sa::read_proof_file(bytes.data(), bytes.size(), nizk ? sa::MODE_NIZK : sa::MODE_SNARK, kzg ? 1 : 0, &pf);
    if (e) die(2, "the proof file is refused: " + std::string(sa::why(e)));
  }
  Handles h; open_ctx(h);
  Stages st;
  const size_t ni = (size_t)pf.num_inputs;
  const uint8_t* inp = ni ? pf.inputs.data() : nullptr;
  int accepted = 0;
  new_transcript(h, a.label);
  if (nizk) {
    const sbn_circom_info info = load_circuit(h, a.files[0]); st.mark("load_r1cs");
    if (info.num_constraints != pf.num_cons || info.num_vars != pf.num_vars || info.num_pub_inputs != pf.num_inputs) {
      fprintf(stderr, "sbn_spartan: the proof was made for a circuit of another shape\n");
      return 1;
    }
    uint8_t d[32];
    check(h, sbn_circom_r1cs_digest(h.ctx, h.circ, d), "sbn_circom_r1cs_digest"); st.mark("digest");
    check(h, sbn_nizk_gens_new(h.ctx, (size_t)pf.num_cons, (size_t)pf.num_vars, ni, &h.gens), "sbn_nizk_gens_new"); st.mark("gens");
    check(h, sbn_nizk_instance_from_circom(h.ctx, h.circ, d, 32, &h.inst), "sbn_nizk_instance_from_circom"); st.mark("instance");
    size_t n_rnd = 0, n_proof = 0;
    check(h, sbn_nizk_sizes(h.inst, &n_rnd, &n_proof), "sbn_nizk_sizes");
    if (n_proof != pf.proof.size()) { fprintf(stderr, "sbn_spartan: the proof has %zu bytes, this circuit's has %zu\n", pf.proof.size(), n_proof); return 1; }
    check(h, sbn_nizk_verify(h.ctx, h.inst, inp, ni, h.gens, pf.proof.data(), pf.proof.size(), h.tr, &accepted), "sbn_nizk_verify");
  } else {
    const std::vector<uint8_t> comm = read_file(a.files[0]);
    check(h, sbn_snark_key_from_comm(h.ctx, comm.data(), comm.size(), &h.key), "sbn_snark_key_from_comm"); st.mark("load_comm");
    if (kzg) { if (is_ptau(a.srs)) load_ptau(h, a.srs, 1, 0, true); else load_srs(h, a.srs, true); st.mark("load_srs"); }
    check(h, sbn_snark_gens_new(h.ctx, (size_t)pf.num_cons, (size_t)pf.num_vars, ni, (size_t)pf.num_nz_entries, &h.gens), "sbn_snark_gens_new"); st.mark("gens");
    size_t n_rnd = 0, n_proof = 0;
    check(h, sbn_snark_sizes(h.key, kzg, &n_rnd, &n_proof), "sbn_snark_sizes");
    if (n_proof != pf.proof.size()) { fprintf(stderr, "sbn_spartan: the proof has %zu bytes, this commitment's has %zu\n", pf.proof.size(), n_proof); return 1; }
    if (kzg) check(h, sbn_snark_verify_kzg(h.ctx, h.key, inp, ni, h.gens, h.g2, h.tau_g2, pf.proof.data(), pf.proof.size(), h.tr, &accepted), "sbn_snark_verify_kzg");
    else check(h, sbn_snark_verify(h.ctx, h.key, inp, ni, h.gens, pf.proof.data(), pf.proof.size(), h.tr, &accepted), "sbn_snark_verify");
  }
  st.mark("verify");
  st.print();
  printf(accepted ? "accepted\n" : "refused\n");
  return accepted ? 0 : 1;
}

}  // namespace

int main(int argc, char** argv) {
  try {
    const Args a = parse(argc, argv);
    if (a.cmd == "info") return run_info(a);
    if (a.cmd == "encode") return run_encode(a);
    if (a.cmd == "prove") return run_prove(a);
    if (a.cmd == "srs") return run_srs(a);
    return run_verify(a);
  } catch (const Fail& f) {
    fprintf(stderr, "sbn_spartan: %s\n", f.text.c_str());
    return f.status;
  } catch (const std::exception& e) {
    fprintf(stderr, "sbn_spartan: %s\n", e.what());
    return 2;
  }
}
