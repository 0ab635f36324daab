"""The KZG SRS file in plain Python integers: the literal model of csrc/srs_host.hpp, k_srs_decompress / k_srs_compress and sbn_kzg_srs_check.

The file is what #[derive(CanonicalSerialize)] writes for KZGSrs { powers_g1: Vec<G1Affine>, tau_g2: G2Affine, g2: G2Affine } in compressed mode:

    n (u64 little-endian) | n x 32 B powers | tau_g2 64 B | g2 64 B | anything (ignored)

A G1 point is x little-endian with bit 7 of byte 31 = "y is the larger of y and q - y" and bit 6 = identity; a G2 point is x.c0 then x.c1 with the
two bits on top of byte 63, "larger" ordering Fq2 by c1 first and c0 on a tie.  Points are (x, y) tuples as pairing_model.py holds them, None is the
identity.  Written from that description on top of pairing_model.py and kzg_model.py; a refusal is SrsError(reason, index or None)."""
import kzg_model as km
import pairing_model as pm

Q, R = pm.Q, km.R
G1_REASONS = ("g1_flags", "g1_identity", "g1_not_canonical", "g1_not_on_curve")
G2_REASONS = ("g2_not_canonical", "g2_flags", "g2_identity", "g2_off_curve", "g2_not_in_subgroup")


class SrsError(Exception):
    def __init__(self, reason, index=None):
        super().__init__(reason, index)
        self.reason, self.index = reason, index


# ---- G1 ----
def g1_y(x):
    """a square root of x^3 + 3 or None (q = 3 mod 4)"""
    a = (x * x * x + 3) % Q
    y = pow(a, (Q + 1) // 4, Q)
    return y if y * y % Q == a else None


def g1_compress(P):
    if P is None:
        return bytes(31) + b"\x40"
    x, y = P
    b = bytearray(x.to_bytes(32, "little"))
    if y > Q - y:
        b[31] |= 0x80
    return bytes(b)


def g1_decompress(b):
    """the refusals in the order the library names them: both flags, the identity, x >= q, x^3 + 3 not a square"""
    flags = b[31] >> 6
    if flags == 3:
        raise SrsError("g1_flags")
    if flags & 1:
        raise SrsError("g1_identity")
    x = int.from_bytes(b[:31] + bytes([b[31] & 0x3f]), "little")
    if x >= Q:
        raise SrsError("g1_not_canonical")
    y = g1_y(x)
    if y is None:
        raise SrsError("g1_not_on_curve")
    if (y > Q - y) != bool(flags & 2):
        y = Q - y
    return (x, y)


def g1_non_residue_x(start=1):
    """the first x >= start with x^3 + 3 a non-residue"""
    x = start
    while g1_y(x) is not None:
        x += 1
    return x


# ---- G2 ----
def f2_larger(y):
    ny = pm.f2_neg(y)
    return (y[1], y[0]) > (ny[1], ny[0])


def g2_compress(P):
    (x0, x1), y = P
    b = bytearray(x0.to_bytes(32, "little") + x1.to_bytes(32, "little"))
    if f2_larger(y):
        b[63] |= 0x80
    return bytes(b)


def g2_decompress(b):
    """the refusals in the order deserialize_compressed meets them (c0, the flags on c1, c1, the identity), then the twist and the subgroup"""
    c0 = int.from_bytes(b[:32], "little")
    if c0 >= Q:
        raise SrsError("g2_not_canonical")
    flags = b[63] >> 6
    if flags == 3:
        raise SrsError("g2_flags")
    c1 = int.from_bytes(b[32:63] + bytes([b[63] & 0x3f]), "little")
    if c1 >= Q:
        raise SrsError("g2_not_canonical")
    if flags & 1:
        raise SrsError("g2_identity")
    x = (c0, c1)
    y = pm.f2_sqrt(pm.f2_add(pm.f2_mul(x, pm.f2_mul(x, x)), pm.B_TWIST))
    if y is None:
        raise SrsError("g2_off_curve")
    if f2_larger(y) != bool(flags & 2):
        y = pm.f2_neg(y)
    if not pm.g2_in_subgroup((x, y)):
        raise SrsError("g2_not_in_subgroup")
    return (x, y)


# ---- the file ----
def file_bytes(n):
    return 8 + 32 * n + 128


def write_srs(powers, tau_g2, g2, trailing=b""):
    return len(powers).to_bytes(8, "little") + b"".join(g1_compress(P) for P in powers) + g2_compress(tau_g2) + g2_compress(g2) + trailing


def scan(data):
    """-> n, or SrsError: 'short' (the file is shorter than its length field says), 'empty' (n = 0)"""
    if len(data) < 8:
        raise SrsError("short")
    n = int.from_bytes(data[:8], "little")
    if n == 0:
        raise SrsError("empty")
    if file_bytes(n) > len(data):
        raise SrsError("short")
    return n


def read_srs(data):
    """-> (powers, tau_g2, g2).  The two G2 points are read first, as the library reads them on the host before any power goes up; a refused power
    carries the smallest refused index"""
    n = scan(data)
    o = 8 + 32 * n
    tau_g2 = g2_decompress(data[o:o + 64])
    g2 = g2_decompress(data[o + 64:o + 128])
    powers = []
    for i in range(n):
        try:
            powers.append(g1_decompress(data[8 + 32 * i:40 + 32 * i]))
        except SrsError as e:
            raise SrsError(e.reason, i) from None
    return powers, tau_g2, g2


# ---- an SRS from tau, and the consistency check ----
def g2_from_tau(tau):
    return pm.G2, pm.g2_mul(pm.G2, tau % R)


def powers_from_tau(tau, n, mul_gen=None):
    """[tau^i] G for i < n; mul_gen(k) -> point may replace the plain double-and-add"""
    mul_gen = mul_gen or (lambda k: pm.g1_mul(pm.G1, k))
    out, x = [], 1
    for _ in range(n):
        out.append(mul_gen(x)); x = x * tau % R
    return out


def msm_plain(scalars, points):
    acc = None
    for k, P in zip(scalars, points):
        acc = pm.g1_add(acc, pm.g1_mul(P, k))
    return acc


def srs_check(powers, g2, tau_g2, rho, msm=msm_plain):
    """P_0 = (1, 2) and e(P_{i+1}, g2) = e(P_i, tau_g2) for all i < n - 1, batched by the powers of rho:
        T = sum_i rho^i P_i,  A = T - P_0,  B = rho T - rho^n P_{n-1},  e(A, g2) e(-B, tau_g2) == 1"""
    if not 0 < rho < R:
        raise ValueError("rho must be in [1, r)")
    n = len(powers)
    if n == 0:
        raise ValueError("no powers")
    if powers[0] != pm.G1:
        return False
    if n == 1:
        return True
    T = msm([pow(rho, i, R) for i in range(n)], powers)
    A = pm.g1_add(T, pm.g1_neg(powers[0]))
    B = pm.g1_add(pm.g1_mul(T, rho), pm.g1_neg(pm.g1_mul(powers[-1], pow(rho, n, R))))
    return pm.pairing_product([(A, g2), (pm.g1_neg(B), tau_g2)]) == pm.F12_ONE


def srs_check_literal(powers, g2, tau_g2):
    """the statement itself, one pairing equation per power (small n only)"""
    if powers[0] != pm.G1:
        return False
    return all(pm.pairing(powers[i + 1], g2) == pm.pairing(powers[i], tau_g2) for i in range(len(powers) - 1))


# ---- the seeded fixture the CPU and GPU tests share ----
FIXTURE_TAU = 0x1d2c3b4a5968778695a4b3c2d1e0f1021324354657687980a9bacbdcedfe0f1 % R
FIXTURE_RHO = 0x0123456789abcdef00112233445566778899aabbccddeeff1032547698badcf % R


def other_curve_point(seed):
    """a point of G1 that is no power of the fixture's tau in any position the tests use: hashed to the curve"""
    import hashlib
    ctr = 0
    while True:
        x = int.from_bytes(hashlib.sha256(b"sbn-srs-g1-%d-%d" % (seed, ctr)).digest(), "little") % Q
        y = g1_y(x)
        if y is not None:
            return (x, y)
        ctr += 1


CORRUPTIONS = ("P_0 replaced", "P_100 replaced", "P_last replaced", "two powers swapped", "tau_g2 of another tau", "g2 and tau_g2 exchanged")


def corruptions(powers, tau_g2, g2):
    """name -> (powers, g2, tau_g2) of every corruption the check must reject"""
    n = len(powers)
    other = other_curve_point(1)
    swap = list(powers); swap[3], swap[n - 4] = swap[n - 4], swap[3]
    g2b, tau1_g2 = g2_from_tau(FIXTURE_TAU + 1)
    return {
        "P_0 replaced": ([other] + powers[1:], g2, tau_g2),
        "P_100 replaced": (powers[:100] + [other] + powers[101:], g2, tau_g2),
        "P_last replaced": (powers[:-1] + [other], g2, tau_g2),
        "two powers swapped": (swap, g2, tau_g2),
        "tau_g2 of another tau": (powers, g2, tau1_g2),
        "g2 and tau_g2 exchanged": (powers, tau_g2, g2),
    }
