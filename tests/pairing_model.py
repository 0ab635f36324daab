"""The BN254 optimal-ate pairing in plain Python integers: the literal model of pairing_host.hpp (line tables) and k_pairing_products (GT bytes).

    e(P, Q) = ( f_{6u+2,Q}(P) * l_{[6u+2]Q, pi(Q)}(P) * l_{[6u+2]Q + pi(Q), -pi^2(Q)}(P) ) ^ ((q^12 - 1) / r)

Tower (arkworks'): Fq2 = Fq[u]/(u^2 + 1), xi = 9 + u, Fq6 = Fq2[v]/(v^3 - xi), Fq12 = Fq6[w]/(w^2 - v).  An Fq12 value is held here as its six
Fq2 coefficients of 1, w, ..., w^5 (w^6 = xi); gt_bytes writes arkworks' order c0.c0.c0, c0.c0.c1, c0.c1.c0, ..., c1.c2.c1 (c_h.c_m is the
coefficient of w^(2m + h)).  The twist is E': y^2 = x^3 + 3/xi (D-type), untwisted by (x, y) -> (x w^2, y w^3).  G2 arithmetic is affine with
slopes by inversion, the final exponentiation is square-and-multiply on the literal integer: nothing here is optimised, on purpose.

A line through T = (xT, yT) with slope lam is  l(P) = yP - lam xP w + (lam xT - yT) w^3 ; a table holds per line the two Fq2 values
(-lam, lam xT - yT): that normal form does not depend on how a G2 point is represented, so a table has ONE byte image.
"""
import hashlib

U = 4965661367192848881
Q = 36 * U**4 + 36 * U**3 + 24 * U**2 + 6 * U + 1
R = 36 * U**4 + 36 * U**3 + 18 * U**2 + 6 * U + 1
ATE = 6 * U + 2
XI = (9, 1)
FINAL_EXPONENT = (Q**12 - 1) // R
COFACTOR = 2 * Q - R

G1 = (1, 2)
G2 = ((10857046999023057135944570762232829481370756359578518086990519993285655852781,
       11559732032986387107991004021392285783925812861821192530917403151452391805634),
      (8495653923123431417604973247489272438418190587263600148770280649306958101930,
       4082367875863433681332203403145435568316851327593401208105741076214120093531))


# ---- Fq2 ----
def f2_add(a, b): return ((a[0] + b[0]) % Q, (a[1] + b[1]) % Q)
def f2_sub(a, b): return ((a[0] - b[0]) % Q, (a[1] - b[1]) % Q)
def f2_neg(a): return (-a[0] % Q, -a[1] % Q)
def f2_mul(a, b): return ((a[0] * b[0] - a[1] * b[1]) % Q, (a[0] * b[1] + a[1] * b[0]) % Q)
def f2_scale(a, k): return (a[0] * k % Q, a[1] * k % Q)
def f2_conj(a): return (a[0], -a[1] % Q)


def f2_inv(a):
    n = pow(a[0] * a[0] + a[1] * a[1], -1, Q)
    return (a[0] * n % Q, -a[1] * n % Q)


def f2_pow(a, e):
    r = (1, 0)
    for bit in bin(e)[2:]:
        r = f2_mul(r, r)
        if bit == "1":
            r = f2_mul(r, a)
    return r


F2_ZERO, F2_ONE = (0, 0), (1, 0)
B_TWIST = f2_mul((3, 0), f2_inv(XI))


def f2_sqrt(a):
    """a square root in Fq2 or None (q = 3 mod 4: the complex method)"""
    if a == F2_ZERO:
        return a
    a1 = f2_pow(a, (Q - 3) // 4)
    alpha = f2_mul(a1, f2_mul(a1, a))
    x0 = f2_mul(a1, a)
    if alpha == (Q - 1, 0):
        x = f2_mul((0, 1), x0)
    else:
        x = f2_mul(f2_pow(f2_add(F2_ONE, alpha), (Q - 1) // 2), x0)
    return x if f2_mul(x, x) == a else None


# ---- Fq12 as six Fq2 coefficients of w^i, w^6 = xi ----
F12_ONE = (F2_ONE,) + (F2_ZERO,) * 5


def f12_mul(a, b):
    out = [F2_ZERO] * 6
    for i in range(6):
        if a[i] == F2_ZERO:
            continue
        for j in range(6):
            t = f2_mul(a[i], b[j])
            if i + j >= 6:
                t = f2_mul(t, XI)
            out[(i + j) % 6] = f2_add(out[(i + j) % 6], t)
    return tuple(out)


def f12_pow(a, e):
    r = F12_ONE
    for bit in bin(e)[2:]:
        r = f12_mul(r, r)
        if bit == "1":
            r = f12_mul(r, a)
    return r


def f12_conj(a):
    """a^(q^6): w -> -w"""
    return tuple(a[i] if i % 2 == 0 else f2_neg(a[i]) for i in range(6))


def f12_from_fq2(c, power=0):
    out = [F2_ZERO] * 6
    out[power] = c
    return tuple(out)


def gt_bytes(f):
    out = b""
    for h in (0, 1):
        for m in (0, 1, 2):
            for part in (0, 1):
                out += f[2 * m + h][part].to_bytes(32, "little")
    return out


GT_ONE = gt_bytes(F12_ONE)


# ---- E'(Fq2), affine; None is the identity ----
def g2_on_curve(P):
    if P is None:
        return True
    x, y = P
    return f2_mul(y, y) == f2_add(f2_mul(x, f2_mul(x, x)), B_TWIST)


def g2_neg(P):
    return None if P is None else (P[0], f2_neg(P[1]))


def g2_slope(A, B):
    """the slope of the line through A and B (the tangent when A == B); None when the line is vertical"""
    if A == B:
        if A[1] == F2_ZERO:
            return None
        return f2_mul(f2_scale(f2_mul(A[0], A[0]), 3), f2_inv(f2_scale(A[1], 2)))
    if A[0] == B[0]:
        return None
    return f2_mul(f2_sub(B[1], A[1]), f2_inv(f2_sub(B[0], A[0])))


def g2_add(A, B):
    if A is None:
        return B
    if B is None:
        return A
    lam = g2_slope(A, B)
    if lam is None:
        return None
    x = f2_sub(f2_sub(f2_mul(lam, lam), A[0]), B[0])
    return (x, f2_sub(f2_mul(lam, f2_sub(A[0], x)), A[1]))


def g2_mul(P, k):
    acc = None
    for bit in bin(k)[2:] if k else "":
        acc = g2_add(acc, acc)
        if bit == "1":
            acc = g2_add(acc, P)
    return acc


def g2_in_subgroup(P):
    return g2_on_curve(P) and g2_mul(P, R) is None


def g2_curve_point(seed):
    """a point of E'(Fq2) from a seed, NOT multiplied by the cofactor: outside G2 with overwhelming probability"""
    ctr = 0
    while True:
        h = hashlib.sha256(b"sbn-g2-%d-%d" % (seed, ctr)).digest()
        x = (int.from_bytes(h, "little") % Q, int.from_bytes(hashlib.sha256(h).digest(), "little") % Q)
        y = f2_sqrt(f2_add(f2_mul(x, f2_mul(x, x)), B_TWIST))
        if y is not None:
            return (x, y)
        ctr += 1


def g2_from_seed(seed):
    return g2_mul(g2_curve_point(seed), COFACTOR)


def g2_bytes(P):
    return b"".join(c.to_bytes(32, "little") for c in (P[0][0], P[0][1], P[1][0], P[1][1]))


# Frobenius of the twist: pi(x, y) = (conj(x) xi^((q-1)/3), conj(y) xi^((q-1)/2))
GAMMA_X = f2_pow(XI, (Q - 1) // 3)
GAMMA_Y = f2_pow(XI, (Q - 1) // 2)


def g2_frobenius(P):
    return (f2_mul(f2_conj(P[0]), GAMMA_X), f2_mul(f2_conj(P[1]), GAMMA_Y))


# ---- G1, affine; None is the identity ----
def g1_add(A, B):
    if A is None:
        return B
    if B is None:
        return A
    if A[0] == B[0]:
        if (A[1] + B[1]) % Q == 0:
            return None
        lam = 3 * A[0] * A[0] * pow(2 * A[1], -1, Q) % Q
    else:
        lam = (B[1] - A[1]) * pow(B[0] - A[0], -1, Q) % Q
    x = (lam * lam - A[0] - B[0]) % Q
    return (x, (lam * (A[0] - x) - A[1]) % Q)


def g1_neg(P):
    return None if P is None else (P[0], -P[1] % Q)


def g1_mul(P, k):
    acc = None
    for bit in bin(k % R)[2:] if k % R else "":
        acc = g1_add(acc, acc)
        if bit == "1":
            acc = g1_add(acc, P)
    return acc


def g1_bytes(P):
    return bytes(64) if P is None else P[0].to_bytes(32, "little") + P[1].to_bytes(32, "little")


def g1_from_bytes(b):
    return None if b == bytes(64) else (int.from_bytes(b[:32], "little"), int.from_bytes(b[32:], "little"))


# ---- schedules: signed digits of 6u + 2, most significant first (the leading digit is 1 and starts the loop) ----
def schedule_binary(n=ATE):
    return [int(b) for b in bin(n)[2:]]


def schedule_naf(n=ATE):
    d = []
    while n:
        if n & 1:
            z = 2 - (n & 3)
            n -= z
        else:
            z = 0
        d.append(z)
        n >>= 1
    return d[::-1]


def line_table(Qp, schedule):
    """[(square_first, -lam, lam xT - yT)]: the lines of the Miller loop over `schedule`, then the two Frobenius lines"""
    assert schedule[0] == 1
    table, T = [], Qp

    def step(A, B, sq):
        lam = g2_slope(A, B)
        assert lam is not None, "a vertical line: the point is not of order r"
        table.append((sq, f2_neg(lam), f2_sub(f2_mul(lam, A[0]), A[1])))
        return g2_add(A, B)

    for d in schedule[1:]:
        T = step(T, T, 1)
        if d:
            T = step(T, Qp if d > 0 else g2_neg(Qp), 0)
    q1 = g2_frobenius(Qp)
    q2 = g2_neg(g2_frobenius(q1))
    T = step(T, q1, 0)
    step(T, q2, 0)
    return table


def line_table_bytes(table):
    """128 bytes a line: -lam.c0, -lam.c1, c.c0, c.c1 as canonical integers (the header prints the same before it converts to device limbs)"""
    return b"".join(c.to_bytes(32, "little") for (_, nl, cc) in table for c in (nl[0], nl[1], cc[0], cc[1]))


def line_eval(line, P):
    _, nl, cc = line
    return ((P[1], 0), f2_scale(nl, P[0]), F2_ZERO, cc, F2_ZERO, F2_ZERO)


def miller(P, table):
    f = F12_ONE
    for line in table:
        if line[0]:
            f = f12_mul(f, f)
        f = f12_mul(f, line_eval(line, P))
    return f


def miller_product(pairs_tables):
    """one shared accumulator over several (P, table) of the SAME schedule"""
    f = F12_ONE
    live = [(P, t) for (P, t) in pairs_tables if P is not None]
    if not live:
        return f
    for s in range(len(live[0][1])):
        if live[0][1][s][0]:
            f = f12_mul(f, f)
        for P, t in live:
            f = f12_mul(f, line_eval(t[s], P))
    return f


def final_exp(f):
    return f12_pow(f, FINAL_EXPONENT)


def pairing(P, Qp, schedule=None):
    if P is None or Qp is None:
        return F12_ONE
    return final_exp(miller(P, line_table(Qp, schedule or schedule_binary())))


def pairing_product(pairs, schedule=None):
    sch = schedule or schedule_binary()
    return final_exp(miller_product([(P, line_table(Qp, sch)) for (P, Qp) in pairs if P is not None and Qp is not None]))


# ---- the hard part by the exact decomposition the kernel uses: (q^4 - q^2 + 1)/r = l0 + l1 q + l2 q^2 + q^3 ----
LAMBDA = (-36 * U**3 - 30 * U**2 - 18 * U - 2, -36 * U**3 - 18 * U**2 - 12 * U + 1, 6 * U**2 + 1, 1)
FROB_GAMMA = [[f2_pow(XI, i * (Q**k - 1) // 6) for i in range(6)] for k in (0, 1, 2, 3)]


def f12_frobenius(a, k=1):
    return tuple(f2_mul(a[i] if k % 2 == 0 else f2_conj(a[i]), FROB_GAMMA[k][i]) for i in range(6))


def kzg_check(C, z, y, pi, g2, tau_g2, schedule=None):
    """KZGProof::verify as the product  e(C - y G + z pi, g2) * e(-pi, tau_g2) == 1  (points as (x, y) or None)"""
    L = g1_add(g1_add(C, g1_neg(g1_mul(G1, y))), g1_mul(pi, z))
    return pairing_product([(L, g2), (g1_neg(pi), tau_g2)], schedule) == F12_ONE
