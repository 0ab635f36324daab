"""A powers-of-tau ceremony file (.ptau) as the KZG SRS in plain Python integers: the literal model of csrc/ptau_host.hpp, k_ptau_points and
sbn_kzg_srs_load_ptau.  Written from the description in include/sbn254.h; NOT compared with a file snarkjs wrote.  All integers little-endian:

    "ptau" | u32 version = 1 | u32 nSections | nSections x ( u32 id | u64 size | size bytes )
    section 1   u32 n8 = 32 | n8 bytes q | u32 power | u32 ceremonyPower                  (44 bytes)
    section 2   2^(power+1) - 1 points of G1, 64 B each: x | y;  point i = [tau^i] G1
    section 3   2^power points of G2, 128 B each: x.c0 | x.c1 | y.c0 | y.c1;  point i = [tau^i] G2 (only 0 and 1 are read)

A coordinate is 32 bytes of v 2^256 mod q (ark-ff's and ffjavascript's Montgomery form); all-zero bytes are the identity.  Sections come in any order,
ids other than 1, 2, 3 are skipped, a second section 1, 2 or 3 is refused.  Points are (x, y) tuples as pairing_model.py holds them, None is the
identity.  A refusal is PtauError(reason, index or None)."""
import pairing_model as pm
import srs_model as sm

Q, R = pm.Q, sm.R
MONT = (1 << 256) % Q
MONT_INV = pow(MONT, -1, Q)
MAX_POWER = 28
SCAN_REASONS = ("short", "magic", "version", "section_past_end", "duplicate_section", "missing_section", "header_size", "n8", "prime", "power", "g1_size", "g2_size")
G1_REASONS = ("g1_not_canonical", "g1_identity", "g1_not_on_curve")
G2_REASONS = ("g2_not_canonical", "g2_identity", "g2_off_curve", "g2_not_in_subgroup")


class PtauError(Exception):
    def __init__(self, reason, index=None):
        super().__init__(reason, index)
        self.reason, self.index = reason, index


def fq_bytes(v):
    """a residue in the file's form: v 2^256 mod q, 32 bytes little-endian"""
    return (v * MONT % Q).to_bytes(32, "little")


def g1_bytes(P):
    return bytes(64) if P is None else fq_bytes(P[0]) + fq_bytes(P[1])


def g2_bytes(P):
    return bytes(128) if P is None else fq_bytes(P[0][0]) + fq_bytes(P[0][1]) + fq_bytes(P[1][0]) + fq_bytes(P[1][1])


# ---- reading a point ----
def g1_read(b):
    """64 bytes -> a point; the refusals in the order the library names them: a residue >= q, the all-zero point, off the curve"""
    x, y = int.from_bytes(b[:32], "little"), int.from_bytes(b[32:64], "little")
    if x >= Q or y >= Q:
        raise PtauError("g1_not_canonical")
    if x == 0 and y == 0:
        raise PtauError("g1_identity")
    x, y = x * MONT_INV % Q, y * MONT_INV % Q
    if (y * y - x * x * x - 3) % Q:
        raise PtauError("g1_not_on_curve")
    return (x, y)


def g2_read(b):
    """128 bytes -> a point of G2: out of Montgomery form, then the refusals of g2_parse_checked in its order"""
    c = [int.from_bytes(b[32 * i:32 * i + 32], "little") for i in range(4)]
    if any(v >= Q for v in c):
        raise PtauError("g2_not_canonical")
    if not any(c):
        raise PtauError("g2_identity")
    c = [v * MONT_INV % Q for v in c]
    P = ((c[0], c[1]), (c[2], c[3]))
    if not pm.g2_on_curve(P):
        raise PtauError("g2_off_curve")
    if not pm.g2_in_subgroup(P):
        raise PtauError("g2_not_in_subgroup")
    return P


# ---- the section table ----
def sections(parts):
    """[(id, payload)] -> the file's bytes"""
    out = b"ptau" + (1).to_bytes(4, "little") + len(parts).to_bytes(4, "little")
    for sid, payload in parts:
        out += sid.to_bytes(4, "little") + len(payload).to_bytes(8, "little") + payload
    return out


def header_section(power, ceremony_power=None, prime=Q, n8=32):
    return n8.to_bytes(4, "little") + prime.to_bytes(n8, "little") + power.to_bytes(4, "little") + (power if ceremony_power is None else ceremony_power).to_bytes(4, "little")


def counts(power):
    return (2 << power) - 1, 1 << power


def scan(data):
    """-> dict(power, ceremony_power, n_g1, n_g2, off_g1, off_g2), or PtauError with one of SCAN_REASONS; no point is touched"""
    n = len(data)
    if n < 12:
        raise PtauError("short")
    if data[:4] != b"ptau":
        raise PtauError("magic")
    if int.from_bytes(data[4:8], "little") != 1:
        raise PtauError("version")
    found, pos = {}, 12
    for _ in range(int.from_bytes(data[8:12], "little")):
        if n - pos < 12:
            raise PtauError("short")
        sid, size = int.from_bytes(data[pos:pos + 4], "little"), int.from_bytes(data[pos + 4:pos + 12], "little")
        pos += 12
        if size > n - pos:
            raise PtauError("section_past_end")
        if sid in (1, 2, 3):
            if sid in found:
                raise PtauError("duplicate_section")
            found[sid] = (pos, size)
        pos += size
    if len(found) != 3:
        raise PtauError("missing_section")
    o1, s1 = found[1]
    if s1 < 4:
        raise PtauError("header_size")
    if int.from_bytes(data[o1:o1 + 4], "little") != 32:
        raise PtauError("n8")
    if s1 != 44:
        raise PtauError("header_size")
    if int.from_bytes(data[o1 + 4:o1 + 36], "little") != Q:
        raise PtauError("prime")
    power = int.from_bytes(data[o1 + 36:o1 + 40], "little")
    if not 1 <= power <= MAX_POWER:
        raise PtauError("power")
    n_g1, n_g2 = counts(power)
    if found[2][1] != 64 * n_g1:
        raise PtauError("g1_size")
    if found[3][1] != 128 * n_g2:
        raise PtauError("g2_size")
    return dict(power=power, ceremony_power=int.from_bytes(data[o1 + 40:o1 + 44], "little"), n_g1=n_g1, n_g2=n_g2, off_g1=found[2][0], off_g2=found[3][0])


def read_ptau(data, n=0):
    """-> (the first n powers (0: all), tau_g2, g2).  The order is the library's: the scan, n, tauG2[1], tauG2[0], then the powers; a refused power carries the
    smallest refused index"""
    s = scan(data)
    if n > s["n_g1"]:
        raise PtauError("n_too_large")
    n = n or s["n_g1"]
    o = s["off_g2"]
    tau_g2 = g2_read(data[o + 128:o + 256])
    g2 = g2_read(data[o:o + 128])
    powers = []
    for i in range(n):
        try:
            powers.append(g1_read(data[s["off_g1"] + 64 * i:s["off_g1"] + 64 * i + 64]))
        except PtauError as e:
            raise PtauError(e.reason, i) from None
    return powers, tau_g2, g2


# ---- writing a file ----
def filler(sid, power):
    """sections 4 .. 7 of a real file, at their sizes: alphaTauG1 and betaTauG1 (2^power G1 points), betaG2 (one G2 point), contributions (an empty list).
    The bytes are a pattern: nothing reads them"""
    size = {4: 64 << power, 5: 64 << power, 6: 128, 7: 4}[sid]
    return bytes((37 * sid + 11 * k) & 0xff for k in range(size)) if sid != 7 else bytes(4)


def write_ptau(power, tau, order=(1, 2, 3, 4, 5, 6, 7), powers=None, g2_real=None, ceremony_power=None, mul_gen=None):
    """the file of [tau^i] G1, i < 2^(power+1) - 1, and [tau^i] G2, i < 2^power, with sections 4 .. 7 as filler, in the section order `order`.
    powers: the G1 points where the caller has them from a faster source (srs_model.powers_from_tau otherwise).  g2_real: how many points of section 3 are
    computed (all by default); the points behind them, which no reader of this library touches, repeat the last computed one"""
    n_g1, n_g2 = counts(power)
    powers = sm.powers_from_tau(tau, n_g1, mul_gen) if powers is None else powers
    assert len(powers) == n_g1
    g2_real = n_g2 if g2_real is None else min(g2_real, n_g2)
    g2s, P = [], pm.G2
    for i in range(g2_real):
        g2s.append(P)
        P = pm.g2_mul(P, tau % R) if i + 1 < g2_real else P
    assert (g2s[0], g2s[1]) == sm.g2_from_tau(tau)
    g2s += [g2s[-1]] * (n_g2 - g2_real)
    body = {1: header_section(power, ceremony_power), 2: b"".join(g1_bytes(P) for P in powers), 3: b"".join(g2_bytes(P) for P in g2s)}
    return sections([(sid, body[sid] if sid in body else filler(sid, power)) for sid in order])


def replace_g1(data, i, point_bytes):
    """the file with the 64 bytes of power i replaced"""
    o = scan(data)["off_g1"] + 64 * i
    return data[:o] + point_bytes + data[o + 64:]


def replace_g2(data, i, point_bytes):
    o = scan(data)["off_g2"] + 128 * i
    return data[:o] + point_bytes + data[o + 128:]
