"""GPU: the KZG SRS as a file buffer — sbn_kzg_srs_load, _save, _check and _g2_from_tau — against an independent producer of the same points
(sbn_kzg_srs_from_tau) and the literal model of tests/srs_model.py.  The seeded fixture holds roots of both signs (asserted on the CPU in
test_srs_model_cpu.py); seams are met in a context of its own with SBN_SRS_CHUNK=64."""
import os

import pytest

import kzg_model as km
import oracle_lib as ol
import pairing_model as pm
import srs_model as sm
from conftest import rand_scalars

pytestmark = pytest.mark.gpu
Q, R = sm.Q, sm.R
TAU, RHO = sm.FIXTURE_TAU, sm.FIXTURE_RHO
N = 200
SIZES = [1, 2, 63, 64, 65, 128, 129, 200]
sb = lambda x: (x % R).to_bytes(32, "little")      # noqa: E731


def oracle_msm(scalars, points):
    return pm.g1_from_bytes(ol.msm_naive(b"".join(k.to_bytes(32, "little") for k in scalars), b"".join(pm.g1_bytes(P) for P in points)))


@pytest.fixture(scope="module")
def fx():
    """the fixture of the CPU tests: (powers, tau_g2, g2) as model points"""
    g2, tau_g2 = sm.g2_from_tau(TAU)
    xy = ol.g1_mul_gen_batch(b"".join(sb(pow(TAU, i, R)) for i in range(N)))
    return [pm.g1_from_bytes(xy[64 * i:64 * i + 64]) for i in range(N)], tau_g2, g2


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


def file_of(fx, n):
    powers, tau_g2, g2 = fx
    return sm.write_srs(powers[:n], tau_g2, g2)


def file_of_powers(xy):
    return b"".join(sm.g1_compress(pm.g1_from_bytes(xy[i:i + 64])) for i in range(0, len(xy), 64))


def free(*hs):
    for h in hs:
        if h is not None:
            h.free()


def load_points(c, data, **kw):
    """load, download, free -> (the points' bytes, g2_xy, tau_g2_xy)"""
    srs, l_g2, l_tau, g2_xy, tau_xy = c.kzg_srs_load(data, **kw)
    try:
        return c.bases_download(srs, 0, len(srs)), g2_xy, tau_xy
    finally:
        free(srs, l_g2, l_tau)


@pytest.mark.parametrize("n", SIZES)
def test_load_equals_the_independent_producer(cx, fx, n):
    ref = cx.kzg_srs_from_tau(sb(TAU), n)
    try:
        want = cx.bases_download(ref, 0, n)
    finally:
        ref.free()
    got, g2_xy, tau_xy = load_points(cx, file_of(fx, n) + b"trailing bytes are ignored")
    assert got == want == b"".join(pm.g1_bytes(P) for P in fx[0][:n])
    assert g2_xy == pm.g2_bytes(fx[2]) and tau_xy == pm.g2_bytes(fx[1])
    got2, _, _ = load_points(cx, file_of(fx, n), want_lines=False)                   # a prover that never verifies
    assert got2 == want


def test_loaded_handles_commit_open_and_verify(cx, fx):
    srs, l_g2, l_tau, _, _ = cx.kzg_srs_load(file_of(fx, N))
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


def test_default_chunk(ctx, sbn):
    n = 4097
    ref = ctx.kzg_srs_from_tau(sb(TAU), n)
    g2_xy, tau_xy = sbn.kzg_srs_g2_from_tau(sb(TAU))
    try:
        want = ctx.bases_download(ref, 0, n)
        f = ctx.kzg_srs_save(ref, g2_xy, tau_xy)
    finally:
        ref.free()
    assert len(f) == 8 + 32 * n + 128 and f[:8] == n.to_bytes(8, "little")
    assert f[8:8 + 32 * N] == file_of_powers(want[:64 * N])
    got, g, t = load_points(ctx, f)
    assert got == want and (g, t) == (g2_xy, tau_xy)


def test_sign_bit_flipped_loads_the_negated_points(cx, fx):
    f = bytearray(file_of(fx, N))
    for i in range(N):
        f[8 + 32 * i + 31] ^= 0x80
    got, _, _ = load_points(cx, bytes(f))
    assert got == b"".join(pm.g1_bytes(pm.g1_neg(P)) for P in fx[0])


def bad_powers(f):
    return {"x is not canonical": Q.to_bytes(32, "little"), "not a square": sm.g1_non_residue_x().to_bytes(32, "little"),
            "identity": bytes(31) + b"\x40", "both flag bits": bytes(f[8:39]) + bytes([f[39] | 0xc0])}


@pytest.mark.parametrize("case", ["x is not canonical", "not a square", "identity", "both flag bits"])
@pytest.mark.parametrize("at", [0, 63, 64, N - 1])
def test_refused_power_reports_its_index(cx, fx, sbn, case, at):
    good = file_of(fx, N)
    f = bytearray(good)
    f[8 + 32 * at:40 + 32 * at] = bad_powers(good)[case]
    with pytest.raises(sm.SrsError) as me:
        sm.read_srs(bytes(f))
    assert me.value.index == at
    with pytest.raises(sbn.SbnError) as e:
        cx.kzg_srs_load(bytes(f))
    assert e.value.bad_index == at and not any(e.value.handles)
    assert case in str(e.value) and f"power {at}:" in str(e.value)
    got, _, _ = load_points(cx, good)                                                 # the context still loads a good file
    assert got == b"".join(pm.g1_bytes(P) for P in fx[0])


def test_two_refused_powers_report_the_smaller_index(cx, fx, sbn):
    good = file_of(fx, N)
    f = bytearray(good)
    f[8 + 32 * 150:40 + 32 * 150] = bad_powers(good)["identity"]
    f[8 + 32 * 70:40 + 32 * 70] = bad_powers(good)["not a square"]
    with pytest.raises(sbn.SbnError) as e:
        cx.kzg_srs_load(bytes(f))
    assert e.value.bad_index == 70 and "not a square" in str(e.value) and not any(e.value.handles)


def test_refusals_that_are_no_power_leave_no_index(cx, fx, sbn):
    good = file_of(fx, 3)
    for f in (good[:-1], bytes(8) + good[8:], good[:104] + bytes(63) + b"\x40" + good[168:], good[:168] + sm.g2_compress(pm.g2_curve_point(7))):
        with pytest.raises(sbn.SbnError) as e:
            cx.kzg_srs_load(f)
        assert e.value.bad_index is None and not any(e.value.handles)


@pytest.mark.parametrize("n", SIZES)
def test_save_equals_the_model_and_loads_back(cx, fx, sbn, n):
    g2_xy, tau_xy = sbn.kzg_srs_g2_from_tau(sb(TAU))
    assert (g2_xy, tau_xy) == (pm.g2_bytes(fx[2]), pm.g2_bytes(fx[1]))
    ref = cx.kzg_srs_from_tau(sb(TAU), n)
    try:
        assert cx.kzg_srs_save_size(ref) == 8 + 32 * n + 128
        f = cx.kzg_srs_save(ref, g2_xy, tau_xy)
        assert f == file_of(fx, n)
        got, g, t = load_points(cx, f)
        assert got == cx.bases_download(ref, 0, n) and (g, t) == (g2_xy, tau_xy)
        # one byte short: refused, and the buffer is untouched
        buf = bytearray(b"\xa5" * (len(f) - 1))
        with pytest.raises(sbn.SbnError):
            cx.kzg_srs_save(ref, g2_xy, tau_xy, out=buf)
        assert buf == b"\xa5" * (len(f) - 1)
        # a larger buffer takes the file and nothing behind it
        big = bytearray(b"\xa5" * (len(f) + 9))
        assert cx.kzg_srs_save(ref, g2_xy, tau_xy, out=big) == len(f) and big == f + b"\xa5" * 9
    finally:
        ref.free()


def test_save_writes_an_identity_as_g1_compress_does(cx, fx, sbn):
    g2_xy, tau_xy = sbn.kzg_srs_g2_from_tau(sb(TAU))
    xy = b"".join(pm.g1_bytes(P) for P in (fx[0][0], None, fx[0][5], None))
    h = cx.bases_upload(xy)
    try:
        f = cx.kzg_srs_save(h, g2_xy, tau_xy)
        with pytest.raises(sbn.SbnError):                                              # a G2 point g2_parse_checked refuses
            cx.kzg_srs_save(h, g2_xy, pm.g2_bytes(pm.g2_curve_point(7)))
    finally:
        h.free()
    assert f[8:8 + 128] == sbn.g1_compress(xy) and f[8 + 32:8 + 64] == bytes(31) + b"\x40"
    with pytest.raises(sbn.SbnError) as e:                                             # and the loader refuses that file: an identity among the powers
        cx.kzg_srs_load(f)
    assert e.value.bad_index == 1


@pytest.mark.parametrize("n", [1, 2, N])
def test_check_accepts_the_fixture(cx, fx, n):
    srs, l_g2, l_tau, _, _ = cx.kzg_srs_load(file_of(fx, n))
    try:
        assert cx.kzg_srs_check(srs, l_g2, l_tau, sb(RHO)) is True
        assert cx.kzg_srs_check(srs, l_g2, l_tau, sb(1)) is True and cx.kzg_srs_check(srs, l_g2, l_tau, sb(R - 1)) is True
    finally:
        free(srs, l_g2, l_tau)
    assert sm.srs_check(fx[0][:n], fx[2], fx[1], RHO, msm=oracle_msm)


@pytest.mark.parametrize("name", sm.CORRUPTIONS)
def test_check_rejects_each_corruption_as_the_model_does(cx, fx, name):
    powers, g2, tau_g2 = sm.corruptions(*fx)[name]
    srs, l_g2, l_tau, _, _ = cx.kzg_srs_load(sm.write_srs(powers, tau_g2, g2))        # loaded as the reference loads it: no relation is checked
    try:
        got = cx.kzg_srs_check(srs, l_g2, l_tau, sb(RHO))
    finally:
        free(srs, l_g2, l_tau)
    assert got is False and got == sm.srs_check(powers, g2, tau_g2, RHO, msm=oracle_msm)


def test_check_refuses_rho_zero_and_rho_r(cx, fx, sbn):
    srs, l_g2, l_tau, _, _ = cx.kzg_srs_load(file_of(fx, 2))
    try:
        for rho in (bytes(32), R.to_bytes(32, "little")):
            with pytest.raises(sbn.SbnError):
                cx.kzg_srs_check(srs, l_g2, l_tau, rho)
    finally:
        free(srs, l_g2, l_tau)


def test_load_with_the_check_flag(cx, fx, sbn):
    powers, g2, tau_g2 = sm.corruptions(*fx)["P_100 replaced"]
    with pytest.raises(sbn.SbnError) as e:
        cx.kzg_srs_load(sm.write_srs(powers, tau_g2, g2), flags=sbn.SBN_SRS_CHECK)
    assert e.value.bad_index is None and not any(e.value.handles) and "sbn_kzg_srs_check" in str(e.value)
    for want_lines in (True, False):
        srs, l_g2, l_tau, _, _ = cx.kzg_srs_load(file_of(fx, N), flags=sbn.SBN_SRS_CHECK, want_lines=want_lines)
        try:
            assert cx.bases_download(srs, 0, N) == b"".join(pm.g1_bytes(P) for P in fx[0])
            assert (l_g2 is None) == (not want_lines)
        finally:
            free(srs, l_g2, l_tau)
