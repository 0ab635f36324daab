"""CPU: the GLV endomorphism of the single-MSM path (spartan-bn254_amd/csrc/glv_kernels.cuh), re-derived with exact integers.

- beta, lambda are cube roots of unity and phi(G) = (beta x, y) = lambda G;
- the short lattice basis from extended Euclid on (r, lambda) and the rounding constants are the ones the kernel carries;
- the shifted (floor) decomposition k = k1 + lambda k2 (mod r) gives 0 <= k1, k2 below 0x6f4e * 2^112, so the top 16-bit window of a
  127-bit half-scalar never reaches 2^15 (8 windows of c = 16, no carry out of the top one);
- the kernel's own arithmetic (glv_split, compiled for the host) equals the model on random, edge and rounding-boundary scalars."""
import math
import os
import random
import re
import subprocess

from conftest import ROOT

P = 0x30644e72e131a029b85045b68181585d97816a916871ca8d3c208c16d87cfd47
R = 0x30644e72e131a029b85045b68181585d2833e84879b9709143e1f593f0000001
LAM = 0x30644e72e131a029048b6e193fd84104cc37a73fec2bc5e9b8ca0b2d36636f23
BETA = 0x30644e72e131a0295e6dd9e7e0acccb0c28f069fbb966e3de4bd44e5607cfd48
HDR = os.path.join(ROOT, "spartan-bn254_amd", "csrc", "glv_kernels.cuh")
M128, M256 = (1 << 128) - 1, (1 << 256) - 1


def ec_add(p, q):
    if p is None:
        return q
    if q is None:
        return p
    if p[0] == q[0] and (p[1] + q[1]) % P == 0:
        return None
    if p == q:
        m = 3 * p[0] * p[0] * pow(2 * p[1], -1, P) % P
    else:
        m = (q[1] - p[1]) * pow(q[0] - p[0], -1, P) % P
    x = (m * m - p[0] - q[0]) % P
    return (x, (m * (p[0] - x) - p[1]) % P)


def ec_mul(p, k):
    acc = None
    while k:
        if k & 1:
            acc = ec_add(acc, p)
        p = ec_add(p, p); k >>= 1
    return acc


def short_basis():
    """extended Euclid on (r, lambda): remainders r_i = t_i lambda (mod r); the first r_i below sqrt(r) and the shorter neighbour"""
    seq = [(R, 0), (LAM, 1)]
    a, b, t0, t1 = R, LAM, 0, 1
    while b:
        q = a // b
        a, b, t0, t1 = b, a - q * b, t1, t0 - q * t1
        seq.append((b, t1))
    sq = math.isqrt(R)
    i = next(j for j, (rj, _) in enumerate(seq) if rj < sq)
    v1 = (seq[i][0], -seq[i][1])
    v2 = min([(seq[i - 1][0], -seq[i - 1][1]), (seq[i + 1][0], -seq[i + 1][1])], key=lambda v: v[0] ** 2 + v[1] ** 2)
    return v1, v2


def kernel_constants():
    src = open(HDR).read()

    def arr(name):
        m = re.search(r"constexpr uint64_t %s(?:\[\d+\])? = \{?([^;}]*)\}?;" % name, src)
        limbs = [int(x.strip().rstrip("ul"), 16) for x in m.group(1).replace("ull", "").split(",")]
        return sum(v << (64 * i) for i, v in enumerate(limbs))
    m = re.search(r"constexpr uint32_t BETA\[8\] = \{([^}]*)\}", src)
    beta = sum(int(x.strip().rstrip("u"), 16) << (32 * i) for i, x in enumerate(m.group(1).split(",")))
    return {k: arr(k) for k in ("A", "B", "C", "G1", "G2", "R")}, beta


V1, V2 = short_basis()
A, B, C = V1[0], V2[0], V2[1]
G1C, G2C = (C << 256) // R, (B << 256) // R
TOP = 0x6f4e << 112          # both halves stay below this: top 16-bit digit (with carry) <= 0x6f4e < 2^15


def split(k):
    """the kernel's decomposition, step by step (glv_split)"""
    c1, c2 = (k * G1C) >> 256, (k * G2C) >> 256
    if ((k * C - c1 * R) & M256) >= R:
        c1 += 1
    if ((k * B - c2 * R) & M256) >= R:
        c2 += 1
    k1, k2 = (k - c1 * A - c2 * B) & M128, (c1 * B - c2 * C) & M128
    if k2 >> 127:
        k1, k2 = (k1 + B) & M128, (k2 + C) & M128
    return k1, k2


def edge_scalars():
    ks = [0, 1, 2, R - 1, R - 2, LAM, R - LAM, (1 << 127) - 1, 1 << 127, (1 << 127) + 1, A, B, C, A + B, R - A, R - C, (1 << 253), (1 << 253) + 12345]
    for j in list(range(1, 300)) + [random.Random(j).randrange(1, C) for j in range(300)]:
        for num in (C, B):                                  # k C / r and k B / r next to an integer: the floor's correction step
            kk = (j * R) // num
            ks += [kk + d for d in (-1, 0, 1, 2) if 0 <= kk + d < R]
    return ks


def test_cube_roots_and_endomorphism():
    assert pow(LAM, 3, R) == 1 and LAM != 1
    assert pow(BETA, 3, P) == 1 and BETA != 1
    G = (1, 2)
    assert ec_mul(G, LAM) == (BETA * G[0] % P, G[1])
    Q = ec_mul(G, 0x1234567890abcdef)                       # another point: phi is lambda on the whole group
    assert ec_mul(Q, LAM) == (BETA * Q[0] % P, Q[1])


def test_basis_and_kernel_constants():
    assert (V1[0] + LAM * V1[1]) % R == 0 and (V2[0] + LAM * V2[1]) % R == 0
    assert V1[1] == -B and V2 == (B, C)                     # v1 = (A, -B), v2 = (B, C)
    assert (A.bit_length(), B.bit_length(), C.bit_length()) == (127, 64, 127)
    assert A * C + B * B == R                               # |det| = r: a basis of the whole lattice
    assert A + 2 * B < TOP and C <= TOP
    consts, beta = kernel_constants()
    assert consts == {"A": A, "B": B, "C": C, "G1": G1C, "G2": G2C, "R": R}
    assert beta == BETA


def test_decomposition_model():
    rnd = random.Random(5)
    ks = edge_scalars() + [rnd.randrange(R) for _ in range(20000)]
    for k in ks:
        k1, k2 = split(k)
        assert (k1 + LAM * k2 - k) % R == 0, hex(k)
        assert 0 <= k1 < A + 2 * B and 0 <= k2 < C, hex(k)
        assert k1 < TOP and k2 < TOP
        # the floor is exact: (k1, k2) - (k, 0) is the lattice point c1 v1 + c2 v2 with c_i = floor(k x_i / r) (or v2 once more)
        c1, c2 = k * C // R, k * B // R
        e1, e2 = k - c1 * A - c2 * B, c1 * B - c2 * C
        assert (k1, k2) == ((e1, e2) if e2 >= 0 else (e1 + B, e2 + C))


def test_top_window_never_carries():
    """c = 16: digits of the 127-bit halves recoded into [-2^15, 2^15) over 8 windows — the top window never leaves a carry"""
    rnd = random.Random(9)
    for k in edge_scalars()[:400] + [rnd.randrange(R) for _ in range(2000)]:
        for h in split(k):
            carry, total = 0, 0
            for w in range(8):
                v = ((h >> (16 * w)) & 0xFFFF) + carry
                d, carry = (v - (1 << 16), 1) if v >= (1 << 15) else (v, 0)
                total += d << (16 * w)
            assert carry == 0 and total == h


def test_kernel_split_compiled_for_host(tmp_path):
    """glv_split from glv_kernels.cuh, compiled by g++ with 64-bit host stand-ins, against the model"""
    src = open(HDR).read()
    body = src[src.index("namespace glv {"):src.index("// n canonical 32-byte scalars")]
    cpp = tmp_path / "glv_host.cpp"
    cpp.write_text("#include <cstdint>\n#include <cstdio>\n#define __device__\n#define __forceinline__ inline\n"
                   "static inline uint64_t __umul64hi(uint64_t a, uint64_t b) { return (uint64_t)(((unsigned __int128)a * b) >> 64); }\n"
                   + body +
                   "int main() { unsigned long long k[4]; while (scanf(\"%llx %llx %llx %llx\", &k[0], &k[1], &k[2], &k[3]) == 4) {\n"
                   "  const uint64_t kk[4] = {k[0], k[1], k[2], k[3]}; uint64_t a[2], b[2]; sbn::glv_split(kk, a, b);\n"
                   "  printf(\"%016llx%016llx %016llx%016llx\\n\", (unsigned long long)a[1], (unsigned long long)a[0], (unsigned long long)b[1], (unsigned long long)b[0]); } }\n"
                   .replace("sbn::", ""))
    exe = str(tmp_path / "glv_host")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", str(cpp), "-o", exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    rnd = random.Random(11)
    ks = edge_scalars() + [rnd.randrange(R) for _ in range(20000)]
    inp = "\n".join(" ".join("%x" % ((k >> (64 * i)) & 0xFFFFFFFFFFFFFFFF) for i in range(4)) for k in ks) + "\n"
    r = subprocess.run([exe], input=inp, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    lines = r.stdout.split()
    assert len(lines) == 2 * len(ks)
    for i, k in enumerate(ks):
        assert (int(lines[2 * i], 16), int(lines[2 * i + 1], 16)) == split(k), hex(k)
