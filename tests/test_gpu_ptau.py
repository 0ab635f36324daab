"""GPU: a powers-of-tau ceremony file (.ptau) as the KZG SRS — sbn_ptau_scan and sbn_kzg_srs_load_ptau — against the two other producers of the same handle
(sbn_kzg_srs_from_tau, sbn_kzg_srs_load on the model's reference-format file) and the literal model of tests/ptau_model.py.  The files are written by
the model around powers the oracle computes; seams are met in a context of its own with SBN_SRS_CHUNK=64.

One case of the list of per-point refusals cannot be a per-point refusal: a point of srs_model.other_curve_point IS a point of G1 (the curve's cofactor
is 1), so no test of one point can tell it from a power of tau.  It loads without SBN_SRS_CHECK, as the model reads it, and is refused with it, by the
consistency check and therefore without an index; that is what the test of that case asserts, at the same four positions."""
import os

import pytest

import kzg_model as km
import oracle_lib as ol
import pairing_model as pm
import ptau_model as ptm
import srs_model as sm
from conftest import golden, rand_scalars

pytestmark = pytest.mark.gpu
Q, R = sm.Q, sm.R
TAU, RHO = sm.FIXTURE_TAU, sm.FIXTURE_RHO
POWER, NG1 = 7, 255
N = 200                                          # the prefix the refusal tests load: four chunks of 64, the last one short
SIZES = [1, 2, 63, 64, 65, 127, 128, 129, 255]
PERMUTED = (7, 3, 5, 2, 6, 1, 4)
sb = lambda x: (x % R).to_bytes(32, "little")      # noqa: E731
le = lambda v: v.to_bytes(32, "little")            # noqa: E731


def oracle_powers(tau, n):
    xy = ol.g1_mul_gen_batch(b"".join(sb(pow(tau, i, R)) for i in range(n)))
    return [pm.g1_from_bytes(xy[64 * i:64 * i + 64]) for i in range(n)]


def oracle_msm(scalars, points):
    return pm.g1_from_bytes(ol.msm_naive(b"".join(k.to_bytes(32, "little") for k in scalars), b"".join(pm.g1_bytes(P) for P in points)))


@pytest.fixture(scope="module")
def fx():
    """the power-7 file of the fixture's tau: (powers, tau_g2, g2, the file, the same file with its sections permuted)"""
    powers = oracle_powers(TAU, NG1)
    g2, tau_g2 = sm.g2_from_tau(TAU)
    f = ptm.write_ptau(POWER, TAU, powers=powers, g2_real=2)
    return dict(powers=powers, tau_g2=tau_g2, g2=g2, file=f, permuted=ptm.write_ptau(POWER, TAU, order=PERMUTED, powers=powers, g2_real=2))


@pytest.fixture(scope="module")
def cx(sbn):
    """a context that cuts the file into chunks of 64 points"""
    old = os.environ.get("SBN_SRS_CHUNK")
    os.environ["SBN_SRS_CHUNK"] = "64"
    try:
        c = sbn.Context(0)
    finally:
        if old is None:
            del os.environ["SBN_SRS_CHUNK"]
        else:
            os.environ["SBN_SRS_CHUNK"] = old
    yield c
    c.close()


def free(*hs):
    for h in hs:
        if h is not None:
            h.free()


def load_points(c, data, n=0, **kw):
    """load, download, free -> (the points' bytes, g2_xy, tau_g2_xy)"""
    srs, l_g2, l_tau, g2_xy, tau_xy = c.kzg_srs_load_ptau(data, n, **kw)
    try:
        return c.bases_download(srs, 0, len(srs)), g2_xy, tau_xy
    finally:
        free(srs, l_g2, l_tau)


def from_tau_points(c, n):
    ref = c.kzg_srs_from_tau(sb(TAU), n)
    try:
        return c.bases_download(ref, 0, n)
    finally:
        ref.free()


def test_scan_equals_the_model(sbn, fx):
    for f in (fx["file"], fx["permuted"]):
        i, want = sbn.ptau_scan(f), ptm.scan(f)
        assert {k: getattr(i, k) for k in want} == want
    assert (i.power, i.n_g1, i.n_g2) == (POWER, NG1, 128)
    with pytest.raises(sbn.SbnError):
        sbn.ptau_scan(fx["file"][:-1])


@pytest.mark.parametrize("n", SIZES)
def test_load_equals_srs_from_tau(cx, sbn, fx, n):
    want = from_tau_points(cx, n)
    got, g2_xy, tau_xy = load_points(cx, fx["file"], n)
    assert got == want == b"".join(pm.g1_bytes(P) for P in fx["powers"][:n])
    assert (g2_xy, tau_xy) == sbn.kzg_srs_g2_from_tau(sb(TAU)) == (pm.g2_bytes(fx["g2"]), pm.g2_bytes(fx["tau_g2"]))
    got2, _, _ = load_points(cx, fx["file"], n, want_lines=False)                     # a prover that never verifies
    assert got2 == want


def test_default_chunk_4097_of_a_power_12_file(ctx):
    n, ng1 = 4097, (2 << 12) - 1
    powers = oracle_powers(TAU, n)
    f = ptm.write_ptau(12, TAU, powers=powers + [powers[-1]] * (ng1 - n), g2_real=2)   # the powers behind the prefix are never read
    got, _, _ = load_points(ctx, f, n)
    assert got == from_tau_points(ctx, n) == b"".join(pm.g1_bytes(P) for P in powers)


def test_n_zero_takes_every_power_of_the_power_3_fixture(ctx, sbn):
    k = golden("ptau_kat.json")
    got, g2_xy, tau_xy = load_points(ctx, bytes.fromhex(k["file"]))
    assert got == from_tau_points(ctx, 15) == b"".join(bytes.fromhex(h) for h in k["g1"])
    assert (g2_xy, tau_xy) == (bytes.fromhex(k["g2"]), bytes.fromhex(k["tau_g2"])) == sbn.kzg_srs_g2_from_tau(sb(int(k["tau"], 16)))
    assert int(k["tau"], 16) == TAU


def test_load_equals_srs_load_of_the_reference_format_file(cx, fx):
    for n in (65, NG1):
        srs, a, b, g2_xy, tau_xy = cx.kzg_srs_load(sm.write_srs(fx["powers"][:n], fx["tau_g2"], fx["g2"]))
        try:
            want = cx.bases_download(srs, 0, n)
        finally:
            free(srs, a, b)
        assert load_points(cx, fx["file"], n) == (want, g2_xy, tau_xy)


def test_permuted_sections_load_the_same(cx, fx):
    assert load_points(cx, fx["permuted"], N) == load_points(cx, fx["file"], N)
    assert load_points(cx, fx["permuted"]) == load_points(cx, fx["file"])


def test_loaded_handles_commit_open_and_verify(cx, fx):
    srs, l_g2, l_tau, _, _ = cx.kzg_srs_load_ptau(fx["file"], N)
    vals = km.from_bytes(rand_scalars(N, 11))
    t = cx.table_upload(km.to_bytes(vals + [0] * (256 - N)))
    try:
        comm, _ = cx.kzg_commit(srs, t, N)
        ev, pi, _ = cx.kzg_open(srs, t, N, sb(987654321))
        assert km.from_bytes(ev)[0] == km.evaluate_poly(vals, 987654321)
        assert cx.kzg_verify(l_g2, l_tau, comm, sb(987654321), ev, pi)
        assert not cx.kzg_verify(l_tau, l_g2, comm, sb(987654321), ev, pi)
    finally:
        t.free(); free(srs, l_g2, l_tau)


def bad_points(fx, at):
    """name -> (64 bytes, the model's reason, a word of the library's text)"""
    good = ptm.g1_bytes(fx["powers"][at])
    return {"a residue equal to q": (le(Q) + good[32:], "g1_not_canonical", "not canonical"),
            "a residue equal to 2^256 - 1": (good[:32] + le((1 << 256) - 1), "g1_not_canonical", "not canonical"),
            "a y with one bit flipped": (good[:32] + bytes([good[32] ^ 4]) + good[33:], "g1_not_on_curve", "not on the curve"),
            "the all-zero point": (bytes(64), "g1_identity", "identity")}


def expect_refusal(cx, sbn, fx, f, at, reason, text):
    with pytest.raises(ptm.PtauError) as me:
        ptm.read_ptau(f, N)
    assert (me.value.reason, me.value.index) == (reason, at)
    with pytest.raises(sbn.SbnError) as e:
        cx.kzg_srs_load_ptau(f, N)
    assert e.value.bad_index == at and not any(e.value.handles)
    assert text in str(e.value) and f"power {at}:" in str(e.value)
    got, _, _ = load_points(cx, fx["file"], N)                                         # the context still loads a good file
    assert got == b"".join(pm.g1_bytes(P) for P in fx["powers"][:N])


@pytest.mark.parametrize("case", ["a residue equal to q", "a residue equal to 2^256 - 1", "a y with one bit flipped", "the all-zero point"])
@pytest.mark.parametrize("at", [0, 63, 64, N - 1])
def test_refused_point_reports_its_index(cx, sbn, fx, case, at):
    b, reason, text = bad_points(fx, at)[case]
    expect_refusal(cx, sbn, fx, ptm.replace_g1(fx["file"], at, b), at, reason, text)


def test_two_refused_points_report_the_smaller_index(cx, sbn, fx):
    f = ptm.replace_g1(fx["file"], 150, bad_points(fx, 150)["the all-zero point"][0])
    f = ptm.replace_g1(f, 70, bad_points(fx, 70)["a y with one bit flipped"][0])
    expect_refusal(cx, sbn, fx, f, 70, "g1_not_on_curve", "not on the curve")
    f = ptm.replace_g1(f, N + 3, bytes(64))                                            # behind the prefix: not read, not reported
    expect_refusal(cx, sbn, fx, f, 70, "g1_not_on_curve", "not on the curve")


@pytest.mark.parametrize("at", [0, 63, 64, N - 1])
def test_another_curve_point_is_refused_by_the_check_alone(cx, sbn, fx, at):
    other = sm.other_curve_point(1)
    f = ptm.replace_g1(fx["file"], at, ptm.g1_bytes(other))
    powers = fx["powers"][:at] + [other] + fx["powers"][at + 1:N]
    assert ptm.read_ptau(f, N)[0] == powers                                            # a point of G1: nothing about it alone is wrong
    got, _, _ = load_points(cx, f, N)
    assert got == b"".join(pm.g1_bytes(P) for P in powers)
    assert sm.srs_check(powers, fx["g2"], fx["tau_g2"], RHO, msm=oracle_msm) is False
    with pytest.raises(sbn.SbnError) as e:
        cx.kzg_srs_load_ptau(f, N, flags=sbn.SBN_SRS_CHECK)
    assert e.value.bad_index is None and not any(e.value.handles) and "sbn_kzg_srs_check" in str(e.value)
    got, _, _ = load_points(cx, fx["file"], N, flags=sbn.SBN_SRS_CHECK)
    assert got == b"".join(pm.g1_bytes(P) for P in fx["powers"][:N])


def test_the_check_flag_gives_the_models_verdict(cx, sbn, fx):
    swapped = list(fx["powers"]); swapped[3], swapped[N - 4] = swapped[N - 4], swapped[3]
    _, tau1_g2 = sm.g2_from_tau(TAU + 1)
    f_swap = ptm.replace_g1(ptm.replace_g1(fx["file"], 3, ptm.g1_bytes(swapped[3])), N - 4, ptm.g1_bytes(swapped[N - 4]))
    cases = [(fx["file"], fx["powers"], fx["tau_g2"]), (f_swap, swapped, fx["tau_g2"]), (ptm.replace_g2(fx["file"], 1, ptm.g2_bytes(tau1_g2)), fx["powers"], tau1_g2)]
    verdicts = []
    for f, powers, tau_g2 in cases:
        want = sm.srs_check(powers[:N], fx["g2"], tau_g2, RHO, msm=oracle_msm)
        try:
            srs, a, b, _, _ = cx.kzg_srs_load_ptau(f, N, flags=sbn.SBN_SRS_CHECK)
            free(srs, a, b)
            got = True
        except sbn.SbnError as e:
            assert e.bad_index is None and not any(e.handles) and "sbn_kzg_srs_check" in str(e)
            got = False
        assert got == want
        verdicts.append(got)
    assert verdicts == [True, False, False]
    for want_lines in (True, False):
        srs, l_g2, l_tau, _, _ = cx.kzg_srs_load_ptau(fx["file"], N, flags=sbn.SBN_SRS_CHECK, want_lines=want_lines)
        try:
            assert (l_g2 is None) == (not want_lines) and len(srs) == N
        finally:
            free(srs, l_g2, l_tau)


def test_refusals_that_are_no_point_leave_no_index(cx, sbn, fx):
    f = fx["file"]
    off = ptm.scan(f)["off_g1"]
    P = pm.g2_curve_point(7)
    files = [f[:off + 64 * N - 1],                                                      # cut inside the first 64 n bytes of section 2
             f[:off + 64 * 10], b"ptaU" + f[4:], ptm.replace_g2(f, 0, bytes(128)), ptm.replace_g2(f, 1, bytes(128)), ptm.replace_g2(f, 1, ptm.g2_bytes(P))]
    for fl in files:
        with pytest.raises(ptm.PtauError):
            ptm.read_ptau(fl, N)
        with pytest.raises(sbn.SbnError) as e:
            cx.kzg_srs_load_ptau(fl, N)
        assert e.value.bad_index is None and not any(e.value.handles)
    with pytest.raises(sbn.SbnError) as e:                                              # n > n_g1
        cx.kzg_srs_load_ptau(f, NG1 + 1)
    assert e.value.bad_index is None and not any(e.value.handles) and "255" in str(e.value)
    with pytest.raises(sbn.SbnError):
        cx.kzg_srs_load_ptau(f, N, flags=2)
    assert len(load_points(cx, f, NG1)[0]) == 64 * NG1
