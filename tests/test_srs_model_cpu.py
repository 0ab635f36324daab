"""CPU: tests/srs_model.py against itself, the committed G1 vectors and the oracle: a written file reads back as what was written, its G1 part is the
compressed form tests/golden/g1_kat.json pins, the seeded fixture the GPU tests load holds roots of both signs, and the batched consistency check
accepts the fixture and rejects every corruption the GPU test rejects."""
import pytest

import oracle_lib as ol
import pairing_model as pm
import srs_model as sm
from conftest import golden

Q, R = sm.Q, sm.R
TAU, RHO = sm.FIXTURE_TAU, sm.FIXTURE_RHO
N = 200


def oracle_mul_gen(k):
    return pm.g1_from_bytes(ol.g1_mul_gen_batch((k % R).to_bytes(32, "little")))


def oracle_msm(scalars, points):
    return pm.g1_from_bytes(ol.msm_naive(b"".join(k.to_bytes(32, "little") for k in scalars), b"".join(pm.g1_bytes(P) for P in points)))


@pytest.fixture(scope="module")
def fixture():
    g2, tau_g2 = sm.g2_from_tau(TAU)
    return sm.powers_from_tau(TAU, N, oracle_mul_gen), tau_g2, g2


def test_the_oracle_and_the_plain_model_agree_on_g1():
    pts = sm.powers_from_tau(TAU, 4)
    assert pts == sm.powers_from_tau(TAU, 4, oracle_mul_gen) and pts[0] == pm.G1
    sc = [pow(RHO, i, R) for i in range(4)]
    assert sm.msm_plain(sc, pts) == oracle_msm(sc, pts)


@pytest.mark.parametrize("n", [1, 2, 3, 64])
def test_read_of_write_is_the_identity(fixture, n):
    powers, tau_g2, g2 = fixture
    f = sm.write_srs(powers[:n], tau_g2, g2)
    assert len(f) == sm.file_bytes(n) == 8 + 32 * n + 128
    assert sm.read_srs(f) == (powers[:n], tau_g2, g2)
    assert sm.read_srs(f + b"tail") == (powers[:n], tau_g2, g2)
    assert sm.write_srs(*sm.read_srs(f)) == f


def test_g1_part_is_the_pinned_compressed_form(fixture):
    _, tau_g2, g2 = fixture
    kat = [e for e in golden("g1_kat.json")["mul"]]
    pts = [pm.g1_from_bytes(bytes.fromhex(e["kG"])) for e in kat]
    f = sm.write_srs(pts, tau_g2, g2)
    assert len(pts) >= 8
    assert f[8:8 + 32 * len(pts)] == b"".join(bytes.fromhex(e["compressed"]) for e in kat)
    assert {bytes.fromhex(e["compressed"])[31] >> 7 for e in kat} == {0, 1}             # both sign bits among the pinned vectors
    for e, P in zip(kat, pts):
        if P is not None:
            assert sm.g1_decompress(bytes.fromhex(e["compressed"])) == P
    comp = golden("g1_kat.json")["compressed"]
    assert sm.g1_compress(pm.G1).hex() == comp["generator"] and sm.g1_compress(None).hex() == comp["infinity"]


def test_the_fixture_holds_roots_of_both_signs(fixture):
    powers, _, _ = fixture
    larger = [P[1] > Q - P[1] for P in powers]
    assert any(larger) and not all(larger)
    assert len(set(larger[:63])) == 2                                                  # and so does every prefix the GPU test loads from n = 63 on
    assert len(set(larger[64:128])) == 2                                               # ... and the second chunk of 64 on its own


def test_every_g1_refusal_carries_its_index(fixture):
    powers, tau_g2, g2 = fixture
    f = bytearray(sm.write_srs(powers[:8], tau_g2, g2))
    bad = {"g1_not_canonical": Q.to_bytes(32, "little"), "g1_not_on_curve": sm.g1_non_residue_x().to_bytes(32, "little"),
           "g1_identity": bytes(31) + b"\x40", "g1_flags": bytes(f[8:39]) + bytes([f[39] | 0xc0])}
    assert set(bad) == set(sm.G1_REASONS)
    for why, b in bad.items():
        for i in (0, 5, 7):
            g = bytearray(f); g[8 + 32 * i:40 + 32 * i] = b
            with pytest.raises(sm.SrsError) as e:
                sm.read_srs(bytes(g))
            assert (e.value.reason, e.value.index) == (why, i)
    g = bytearray(f); g[8 + 32 * 6:40 + 32 * 6] = bad["g1_identity"]; g[8 + 32 * 2:40 + 32 * 2] = bad["g1_not_canonical"]
    with pytest.raises(sm.SrsError) as e:
        sm.read_srs(bytes(g))
    assert (e.value.reason, e.value.index) == ("g1_not_canonical", 2)                  # the smallest index


def test_check_accepts_the_fixture(fixture):
    powers, tau_g2, g2 = fixture
    for n in (1, 2, N):
        assert sm.srs_check(powers[:n], g2, tau_g2, RHO, msm=oracle_msm)
    assert sm.srs_check(powers[:3], g2, tau_g2, RHO) and sm.srs_check_literal(powers[:3], g2, tau_g2)      # the plain sum, and the statement itself
    for rho in (0, R):
        with pytest.raises(ValueError):
            sm.srs_check(powers[:2], g2, tau_g2, rho)


@pytest.mark.parametrize("name", sm.CORRUPTIONS)
def test_check_rejects_each_corruption(fixture, name):
    powers, tau_g2, g2 = fixture
    p, g, t = sm.corruptions(powers, tau_g2, g2)[name]
    assert not sm.srs_check(p, g, t, RHO, msm=oracle_msm)


def test_check_rejects_a_small_corruption_as_the_statement_does(fixture):
    powers, tau_g2, g2 = fixture
    p = [powers[0], powers[2], powers[1]]
    assert not sm.srs_check_literal(p, g2, tau_g2) and not sm.srs_check(p, g2, tau_g2, RHO)
