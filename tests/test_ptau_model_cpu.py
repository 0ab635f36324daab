"""CPU: the literal model of a .ptau file (tests/ptau_model.py) against itself and the committed fixture tests/golden/ptau_kat.json: read of write in
every section order the tests use, the fixture's bytes and points, and each named refusal."""
import pytest

import pairing_model as pm
import ptau_model as ptm
import srs_model as sm
from conftest import golden

Q, R = ptm.Q, ptm.R
PERMUTED = (7, 3, 5, 2, 6, 1, 4)
le32 = lambda v: v.to_bytes(4, "little")       # noqa: E731
le64 = lambda v: v.to_bytes(8, "little")       # noqa: E731


@pytest.fixture(scope="module")
def kat():
    k = golden("ptau_kat.json")
    return dict(tau=int(k["tau"], 16), power=k["power"], file=bytes.fromhex(k["file"]), permuted=bytes.fromhex(k["file_permuted"]),
                g1=[pm.g1_from_bytes(bytes.fromhex(h)) for h in k["g1"]], g2=bytes.fromhex(k["g2"]), tau_g2=bytes.fromhex(k["tau_g2"]), scan=k["scan"])


def test_the_fixture_is_what_the_model_writes(kat):
    assert kat["power"] == 3 and len(kat["g1"]) == 15
    assert ptm.write_ptau(3, kat["tau"]) == kat["file"]
    assert ptm.write_ptau(3, kat["tau"], order=PERMUTED) == kat["permuted"]
    assert kat["g1"] == sm.powers_from_tau(kat["tau"], 15)
    g2, tau_g2 = sm.g2_from_tau(kat["tau"])
    assert (kat["g2"], kat["tau_g2"]) == (pm.g2_bytes(g2), pm.g2_bytes(tau_g2))
    assert ptm.scan(kat["file"]) == kat["scan"]
    # the points hold roots of both signs, so a sign slip in a reader cannot pass
    assert {P[1] > Q - P[1] for P in kat["g1"]} == {True, False}


def test_read_of_write(kat):
    g2, tau_g2 = sm.g2_from_tau(kat["tau"])
    for f in (kat["file"], kat["permuted"]):
        assert ptm.read_ptau(f) == (kat["g1"], tau_g2, g2)
        for n in (1, 2, 14, 15):
            assert ptm.read_ptau(f, n) == (kat["g1"][:n], tau_g2, g2)
    s, sp = ptm.scan(kat["file"]), ptm.scan(kat["permuted"])
    assert (s["power"], s["ceremony_power"], s["n_g1"], s["n_g2"]) == (3, 3, 15, 8) == (sp["power"], sp["ceremony_power"], sp["n_g1"], sp["n_g2"])
    assert s["off_g1"] == 12 + 12 + 44 + 12 and s["off_g2"] == s["off_g1"] + 960 + 12
    assert sp["off_g2"] == 12 + 12 + 4 + 12 and sp["off_g1"] != s["off_g1"]
    # the coordinates are v 2^256 mod q, not v
    assert kat["file"][s["off_g1"]:s["off_g1"] + 32] == ((1 << 256) % Q).to_bytes(32, "little")
    # every point of section 3 is the power of tau it stands for
    P = pm.G2
    for i in range(8):
        assert ptm.g2_read(kat["file"][s["off_g2"] + 128 * i:s["off_g2"] + 128 * i + 128]) == P
        P = pm.g2_mul(P, kat["tau"])
    assert ptm.write_ptau(3, kat["tau"], ceremony_power=28)[ptm.scan(kat["file"])["off_g1"] - 16:][:4] == le32(28)


def test_every_prefix_is_refused(kat):
    for f in (kat["file"], kat["permuted"]):
        for n in range(len(f)):
            with pytest.raises(ptm.PtauError) as e:
                ptm.scan(f[:n])
            assert e.value.reason in ("short", "section_past_end", "missing_section"), n
        assert ptm.scan(f + b"trailing")["n_g1"] == 15


def scan_refusals(kat):
    """(reason, file) for every refusal of the scan"""
    f, tau = kat["file"], kat["tau"]
    s = ptm.scan(f)
    sec = {1: ptm.header_section(3), 2: f[s["off_g1"]:s["off_g1"] + 960], 3: f[s["off_g2"]:s["off_g2"] + 1024]}
    build = lambda **kw: ptm.sections([(i, kw.get("s%d" % i, sec[i])) for i in kw.get("order", (1, 2, 3))])      # noqa: E731
    yield "short", f[:11]
    yield "magic", b"ptaU" + f[4:]
    yield "version", f[:4] + le32(2) + f[8:]
    yield "short", f[:8] + le32(8) + f[12:]                                             # one section more than the file holds
    yield "short", f[:8] + le32(0xffffffff) + f[12:]
    # size fields that overflow an offset: 2^61, 2^64 - 1, and one byte too many
    for size in (1 << 61, (1 << 64) - 1, len(f) - 24 + 1):
        yield "section_past_end", f[:16] + le64(size) + f[24:]
    yield "section_past_end", f[:-1]
    yield "duplicate_section", build(order=(1, 2, 3, 2))
    yield "duplicate_section", build(order=(1, 1, 2, 3))
    yield "duplicate_section", build(order=(3, 1, 2, 3))
    yield "missing_section", build(order=(1, 2))
    yield "missing_section", build(order=(2, 3))
    yield "missing_section", ptm.sections([(4, b"abc")])
    yield "header_size", build(s1=b"\x20\0")
    yield "header_size", build(s1=sec[1] + b"\0")
    yield "header_size", build(s1=sec[1][:-1])
    yield "n8", build(s1=ptm.header_section(3, prime=Q, n8=48))
    yield "n8", build(s1=le32(31) + sec[1][4:])
    yield "prime", build(s1=ptm.header_section(3, prime=R))
    yield "prime", build(s1=ptm.header_section(3, prime=Q + 1))
    yield "power", build(s1=ptm.header_section(0))
    yield "power", build(s1=ptm.header_section(29))
    yield "power", build(s1=ptm.header_section(63))                                      # 64 * 2^64 would overflow
    yield "power", build(s1=ptm.header_section(0xffffffff))
    yield "g1_size", build(s2=sec[2][:-64])
    yield "g1_size", build(s2=sec[2] + bytes(64))
    yield "g1_size", build(s1=ptm.header_section(4))
    yield "g1_size", build(s1=ptm.header_section(28))
    yield "g2_size", build(s3=sec[3][:-128])
    yield "g2_size", build(s3=sec[3] + bytes(1))


def test_every_scan_refusal(kat):
    cases = list(scan_refusals(kat))
    assert {w for w, _ in cases} == set(ptm.SCAN_REASONS)
    for why, f in cases:
        with pytest.raises(ptm.PtauError) as e:
            ptm.read_ptau(f)
        assert e.value.reason == why and e.value.index is None, why


def g1_refusals(kat):
    good = ptm.g1_bytes(kat["g1"][5])
    yield "g1_not_canonical", Q.to_bytes(32, "little") + good[32:]
    yield "g1_not_canonical", good[:32] + Q.to_bytes(32, "little")
    yield "g1_not_canonical", ((1 << 256) - 1).to_bytes(32, "little") + good[32:]
    yield "g1_not_canonical", good[:32] + ((1 << 256) - 1).to_bytes(32, "little")
    yield "g1_identity", bytes(64)
    yield "g1_not_on_curve", good[:32] + bytes([good[32] ^ 1]) + good[33:]
    yield "g1_not_on_curve", pm.g1_bytes(kat["g1"][5])                                  # canonical bytes where Montgomery ones belong
    yield "g1_not_on_curve", bytes(32) + good[32:]


def g2_refusals(kat):
    good = ptm.g2_bytes(sm.g2_from_tau(kat["tau"])[1])
    for k in range(4):
        yield "g2_not_canonical", good[:32 * k] + Q.to_bytes(32, "little") + good[32 * k + 32:]
    yield "g2_not_canonical", ((1 << 256) - 1).to_bytes(32, "little") + good[32:]
    yield "g2_identity", bytes(128)
    yield "g2_off_curve", good[:64] + bytes([good[64] ^ 1]) + good[65:]
    P = pm.g2_curve_point(7)
    assert pm.g2_on_curve(P) and not pm.g2_in_subgroup(P)
    yield "g2_not_in_subgroup", ptm.g2_bytes(P)


def test_every_point_refusal(kat):
    f = kat["file"]
    cases = list(g1_refusals(kat))
    assert {w for w, _ in cases} == set(ptm.G1_REASONS)
    for why, b in cases:
        for at in (0, 7, 14):
            with pytest.raises(ptm.PtauError) as e:
                ptm.read_ptau(ptm.replace_g1(f, at, b))
            assert (e.value.reason, e.value.index) == (why, at)
        assert len(ptm.read_ptau(ptm.replace_g1(f, 14, b), 14)[0]) == 14              # behind the prefix that is asked for: not read
    two = ptm.replace_g1(ptm.replace_g1(f, 9, bytes(64)), 4, cases[0][1])
    with pytest.raises(ptm.PtauError) as e:
        ptm.read_ptau(two)
    assert (e.value.reason, e.value.index) == ("g1_not_canonical", 4)
    cases = list(g2_refusals(kat))
    assert {w for w, _ in cases} == set(ptm.G2_REASONS)
    for why, b in cases:
        for at in (0, 1):
            with pytest.raises(ptm.PtauError) as e:
                ptm.read_ptau(ptm.replace_g2(f, at, b))
            assert (e.value.reason, e.value.index) == (why, None)
        assert ptm.read_ptau(ptm.replace_g2(f, 2, b)) == ptm.read_ptau(f)              # tauG2[2 ..] is never read
    with pytest.raises(ptm.PtauError) as e:
        ptm.read_ptau(f, 16)
    assert e.value.reason == "n_too_large"
