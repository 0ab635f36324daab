"""CPU: csrc/srs_host.hpp — the length field of a KZG SRS file, the two G2 points through the Fq2 square root and g2_parse_checked, and g2 / [tau] g2
from tau — against the literal model of tests/srs_model.py.  tests/srs_host_check.cpp includes the header alone and is built with g++ under
ASan + UBSan as a stand-alone program; it is fed one case per line, each copied into a buffer of exactly its length, and compared line by line."""
import os
import subprocess

import pytest

import oracle_lib as ol
import pairing_model as pm
import srs_model as sm
from conftest import ROOT

Q, R = sm.Q, sm.R
TAU = sm.FIXTURE_TAU


@pytest.fixture(scope="module")
def check(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("srs_host") / "srs_host_check")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        os.path.join(ROOT, "tests", "srs_host_check.cpp"), "-o", exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr

    def run(kind, cases):
        """-> the words of each case's result line"""
        text = "".join(f"{kind} {bytes(f).hex() or '-'}\n" for f in cases)
        r = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]                # a sanitizer report ends the program with another status
        lines = r.stdout.splitlines()
        assert lines[-1] == "SRS HOST CHECK DONE" and len(lines) == len(cases) + 1
        return [ln.split() for ln in lines[:-1]]
    return run


def srs_file(n, tau=TAU, **kw):
    """a file of n powers of tau; the powers by the oracle's fixed-base multiplication (the host half never reads them)"""
    sc = b"".join(pow(tau, i, R).to_bytes(32, "little") for i in range(n))
    xy = ol.g1_mul_gen_batch(sc)
    powers = [pm.g1_from_bytes(xy[64 * i:64 * i + 64]) for i in range(n)]
    g2, tau_g2 = sm.g2_from_tau(tau)
    return sm.write_srs(powers, tau_g2, g2, **kw)


def model_line(data):
    """the line srs_host_check prints for a file, from the model"""
    try:
        n = sm.scan(data)
        o = 8 + 32 * n
        t, g = sm.g2_decompress(data[o:o + 64]), sm.g2_decompress(data[o + 64:o + 128])
    except sm.SrsError as e:
        return ["refused", e.reason]
    return ["ok", str(n), str(o), str(o + 64), pm.g2_bytes(t).hex(), pm.g2_bytes(g).hex(), sm.g2_compress(t).hex(), sm.g2_compress(g).hex()]


def test_header_fields_and_trailing_bytes(check):
    files = [srs_file(n) for n in (1, 3, 64)]
    files.append(srs_file(3, trailing=b"\xff" * 7))                                   # bytes behind g2 are ignored
    got = check("srs", files)
    for f, g in zip(files, got):
        want = model_line(f)
        assert want[0] == "ok" and g == want
        # compressing what was decompressed gives the file's own bytes back
        n = int(g[1])
        assert bytes.fromhex(g[6]) == f[8 + 32 * n:72 + 32 * n] and bytes.fromhex(g[7]) == f[72 + 32 * n:136 + 32 * n]
    assert [int(g[1]) for g in got] == [1, 3, 64, 3]
    assert got[3][1:] == got[1][1:]


def test_g2_points_of_both_signs_round_trip(check):
    pts, P = [], None
    for _ in range(64):                                                               # the seeded search: [k] G2 for k = 1 .. 64
        P = pm.g2_add(P, pm.G2)
        pts.append(P)
    signs = {sm.f2_larger(P[1]) for P in pts}
    assert signs == {True, False}
    ties = [P for P in pts if P[1][1] == 0]                                           # y.c1 = 0: the order falls to c0.  none found among these 64
    cases = [sm.g2_compress(P) for P in pts]
    got = check("g2", cases)
    for P, c, g in zip(pts, cases, got):
        assert sm.g2_decompress(c) == P
        assert g == ["ok", pm.g2_bytes(P).hex(), c.hex()]
    # the flag alone picks the root: flipping bit 7 gives the negated point
    flipped = [c[:63] + bytes([c[63] ^ 0x80]) for c in cases[:4]]
    for P, g in zip(pts, check("g2", flipped)):
        assert g[:2] == ["ok", pm.g2_bytes(pm.g2_neg(P)).hex()]
    # the tie in arkworks' order of Fq2, on values: c1 equal, so c0 decides
    assert sm.f2_larger((Q - 1, 0)) and not sm.f2_larger((1, 0))
    assert len(ties) == 0 or all(sm.g2_decompress(sm.g2_compress(P)) == P for P in ties)


def test_every_prefix_of_a_three_power_file_is_refused(check):
    f = srs_file(3)
    assert len(f) == 232
    prefixes = [f[:n] for n in range(len(f))]
    assert len(prefixes) == 232
    got = check("srs", prefixes)
    for n, (p, g) in enumerate(zip(prefixes, got)):
        with pytest.raises(sm.SrsError) as e:
            sm.read_srs(p)
        assert e.value.reason == "short" and g == ["refused", "short"], n


def test_length_fields_that_overflow_and_zero(check):
    f = srs_file(3)
    cases = [("short", (1 << 61).to_bytes(8, "little") + f[8:]), ("short", ((1 << 64) - 1).to_bytes(8, "little") + f[8:]),
             ("short", (4).to_bytes(8, "little") + f[8:]), ("empty", bytes(8) + f[8:]), ("empty", bytes(8) + f[-128:])]
    got = check("srs", [c for _, c in cases])
    for (why, c), g in zip(cases, got):
        with pytest.raises(sm.SrsError) as e:
            sm.read_srs(c)
        assert e.value.reason == why and g == ["refused", why]


def g2_refusals():
    g2, tau_g2 = sm.g2_from_tau(TAU)
    good = sm.g2_compress(tau_g2)
    le = lambda v: v.to_bytes(32, "little")       # noqa: E731
    yield "g2_not_canonical", le(Q) + good[32:]
    yield "g2_not_canonical", le((1 << 256) - 1) + good[32:]
    yield "g2_not_canonical", good[:32] + le(Q)                                       # c1 = q under clear flag bits
    yield "g2_not_canonical", good[:32] + le(Q | 1 << 255)                            # ... and under the sign bit
    yield "g2_flags", good[:63] + bytes([good[63] | 0xc0])
    yield "g2_identity", bytes(63) + b"\x40"
    yield "g2_identity", good[:63] + bytes([(good[63] & 0x3f) | 0x40])                # the flag decides, whatever x holds
    x = (5, 0)
    while pm.f2_sqrt(pm.f2_add(pm.f2_mul(x, pm.f2_mul(x, x)), pm.B_TWIST)) is not None:
        x = (x[0] + 1, 0)
    yield "g2_off_curve", le(x[0]) + le(x[1])
    P = pm.g2_curve_point(7)
    assert pm.g2_on_curve(P) and not pm.g2_in_subgroup(P)
    yield "g2_not_in_subgroup", sm.g2_compress(P)


def test_every_g2_refusal(check):
    cases = list(g2_refusals())
    assert {w for w, _ in cases} == set(sm.G2_REASONS)
    got = check("g2", [c for _, c in cases])
    for (why, c), g in zip(cases, got):
        with pytest.raises(sm.SrsError) as e:
            sm.g2_decompress(c)
        assert e.value.reason == why and g == ["refused", why], (why, g)
    # the same through a whole file, in either position
    f = srs_file(3)
    files = [f[:104] + c + f[168:] for _, c in cases] + [f[:168] + c for _, c in cases]
    got = check("srs", files)
    for (why, _), g in zip(cases + cases, got):
        assert g == ["refused", why]
    for fl in files:
        with pytest.raises(sm.SrsError):
            sm.read_srs(fl)


def test_g2_from_tau(check):
    taus = [1, 2, TAU, R - 1]
    got = check("tau", [t.to_bytes(32, "little") for t in taus] + [bytes(32), R.to_bytes(32, "little")])
    for t, g in zip(taus, got):
        g2, tau_g2 = sm.g2_from_tau(t)
        assert g == ["ok", pm.g2_bytes(g2).hex(), pm.g2_bytes(tau_g2).hex()]
    assert got[-2:] == [["refused", "tau"], ["refused", "tau"]]
