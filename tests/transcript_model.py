"""Merlin v1.0 transcripts over STROBE-128 in plain Python integers: the checker of the library's host and device transcripts.

Written from the public Merlin / STROBE specifications (Keccak-f[1600] from FIPS 202), not from the library's code.
The state record is the one of sbn_transcript_state: 200 state bytes, then pos, pos_begin, cur_flags.
"""

R_MOD = 21888242871839275222246405745257275088548364400416034343698204186575808495617      # BN254's scalar field
RATE = 166                                                                                # STROBE-128: 200 - 128 / 4 - 2
FLAG_I, FLAG_A, FLAG_C, FLAG_T, FLAG_M, FLAG_K = 1, 2, 4, 8, 16, 32
M64 = (1 << 64) - 1


def _rol(x, n):
    n %= 64
    return ((x << n) | (x >> (64 - n))) & M64 if n else x


def _round_constants():
    rc, lfsr = [], 1
    for _ in range(24):
        c = 0
        for j in range(7):
            if lfsr & 1:
                c |= 1 << ((1 << j) - 1)
            lfsr = ((lfsr << 1) ^ (0x71 if lfsr & 0x80 else 0)) & 0xFF
        rc.append(c)
    return rc


def _rho_offsets():
    rho = [0] * 25
    x, y = 1, 0
    for t in range(24):
        rho[x + 5 * y] = ((t + 1) * (t + 2) // 2) % 64
        x, y = y, (2 * x + 3 * y) % 5
    return rho


_RC, _RHO = _round_constants(), _rho_offsets()


def keccak_f1600(state):
    """the permutation on 200 bytes (lane x + 5 y = bytes 8 (x + 5 y) .. + 8, little-endian)"""
    a = [int.from_bytes(state[8 * i:8 * i + 8], "little") for i in range(25)]
    for rnd in range(24):
        c = [a[x] ^ a[x + 5] ^ a[x + 10] ^ a[x + 15] ^ a[x + 20] for x in range(5)]
        d = [c[(x + 4) % 5] ^ _rol(c[(x + 1) % 5], 1) for x in range(5)]
        a = [a[i] ^ d[i % 5] for i in range(25)]
        b = [0] * 25
        for x in range(5):
            for y in range(5):
                b[y + 5 * ((2 * x + 3 * y) % 5)] = _rol(a[x + 5 * y], _RHO[x + 5 * y])
        a = [b[i] ^ (~b[(i % 5 + 1) % 5 + 5 * (i // 5)] & M64 & b[(i % 5 + 2) % 5 + 5 * (i // 5)]) for i in range(25)]
        a[0] ^= _RC[rnd]
    return bytearray(b"".join(v.to_bytes(8, "little") for v in a))


class Strobe128:
    def __init__(self, protocol_label):
        st = bytearray(200)
        st[0:6] = bytes([1, RATE + 2, 1, 0, 1, 96])
        st[6:18] = b"STROBEv1.0.2"
        self.st = keccak_f1600(st)
        self.pos = self.pos_begin = self.cur_flags = 0
        self.permutations = 0
        self.meta_ad(protocol_label, False)

    def _run_f(self):
        self.st[self.pos] ^= self.pos_begin
        self.st[self.pos + 1] ^= 0x04
        self.st[RATE + 1] ^= 0x80
        self.st = keccak_f1600(self.st)
        self.pos = self.pos_begin = 0
        self.permutations += 1

    def _absorb(self, data):
        for b in data:
            self.st[self.pos] ^= b
            self.pos += 1
            if self.pos == RATE:
                self._run_f()

    def _squeeze(self, n):
        out = bytearray()
        for _ in range(n):
            out.append(self.st[self.pos])
            self.st[self.pos] = 0
            self.pos += 1
            if self.pos == RATE:
                self._run_f()
        return bytes(out)

    def _begin_op(self, flags, more):
        if more:
            assert flags == self.cur_flags
            return
        old = self.pos_begin
        self.pos_begin = self.pos + 1
        self.cur_flags = flags
        self._absorb(bytes([old, flags]))
        if flags & (FLAG_C | FLAG_K) and self.pos != 0:
            self._run_f()

    def meta_ad(self, data, more):
        self._begin_op(FLAG_M | FLAG_A, more)
        self._absorb(data)

    def ad(self, data, more):
        self._begin_op(FLAG_A, more)
        self._absorb(data)

    def prf(self, n, more):
        self._begin_op(FLAG_I | FLAG_A | FLAG_C, more)
        return self._squeeze(n)


class Transcript:
    def __init__(self, label=None, _strobe=None):
        if _strobe is not None:
            self.s = _strobe
            return
        self.s = Strobe128(b"Merlin v1.0")
        self.append_message(b"dom-sep", label)

    def append_message(self, label, msg):
        self.s.meta_ad(label, False)
        self.s.meta_ad(len(msg).to_bytes(4, "little"), True)
        self.s.ad(msg, False)

    def challenge_bytes(self, label, n):
        self.s.meta_ad(label, False)
        self.s.meta_ad(n.to_bytes(4, "little"), True)
        return self.s.prf(n, False)

    def challenge_scalar(self, label):
        """transcript.rs:56-67: 64 bytes, little-endian, mod r; the canonical integer"""
        return int.from_bytes(self.challenge_bytes(label, 64), "little") % R_MOD

    def append_scalar(self, label, x):
        self.append_message(label, int(x).to_bytes(32, "little"))

    def state(self):
        return bytes(self.s.st) + bytes([self.s.pos, self.s.pos_begin, self.s.cur_flags])

    @classmethod
    def from_state(cls, rec):
        assert len(rec) == 203
        s = Strobe128.__new__(Strobe128)
        s.st = bytearray(rec[:200]); s.pos, s.pos_begin, s.cur_flags = rec[200], rec[201], rec[202]
        s.permutations = 0
        return cls(_strobe=s)

    def clone(self):
        return Transcript.from_state(self.state())

    @property
    def permutations(self):
        return self.s.permutations


# ---- one sumcheck round as the reference writes it (unipoly.rs:28-59, 117-122; sumcheck.rs:269-301) -----------------------------

def unipoly_from_evals4(e):
    """[p(0), p(1), p(2), p(3)] -> [d, c, b, a] of a x^3 + b x^2 + c x + d"""
    inv2, inv6 = pow(2, -1, R_MOD), pow(6, -1, R_MOD)
    d = e[0] % R_MOD
    a = inv6 * (e[3] - 3 * e[2] + 3 * e[1] - e[0]) % R_MOD
    b = inv2 * (2 * e[0] - 5 * e[1] + 4 * e[2] - e[3]) % R_MOD
    c = (e[1] - d - a - b) % R_MOD
    return [d, c, b, a]


def unipoly_eval(co, r):
    return sum(c * pow(r, i, R_MOD) for i, c in enumerate(co)) % R_MOD


def sumcheck_round_step(tr, claim, e0, e2, e3):
    """the host's work between two round kernels: returns (coeffs [c0..c3], r_j, the next claim)"""
    co = unipoly_from_evals4([e0, (claim - e0) % R_MOD, e2, e3])
    tr.append_message(b"poly", b"UniPoly_begin")
    for c in co:
        tr.append_scalar(b"coeff", c)
    tr.append_message(b"poly", b"UniPoly_end")
    r = tr.challenge_scalar(b"challenge_nextround")
    return co, r, unipoly_eval(co, r)
