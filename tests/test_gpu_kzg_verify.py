"""GPU: sbn_kzg_verify / sbn_kzg_verify_batched (KZGProof::verify, KZGBatchProof::batch_verify as a two-term pairing product over prepared G2
points) on what sbn_kzg_commit / sbn_kzg_open / sbn_kzg_open_batched produce over an SRS from a known tau.  With tau known, the reference's
pairing check is the relation C - y G == (tau - z) pi in G1 (sparse_eval_kzg_model.kzg_verify): every verdict, honest or tampered, equals it."""
import ctypes as C
import random

import pytest

from conftest import golden, rand_scalars
import kzg_model as km
import oracle_lib as ol
import sparse_eval_kzg_model as skm

pytestmark = pytest.mark.gpu
KAT = golden("pairing_kat.json")
R = km.R
TAU = int(KAT["tau"], 16)
G = skm.G
INF = bytes(64)
SRS_N = 1 << 10
sb = lambda x: (x % R).to_bytes(32, "little")      # noqa: E731


@pytest.fixture(scope="module")
def kzg(ctx):
    srs = ctx.kzg_srs_from_tau(sb(TAU), SRS_N)
    hs = {k: ctx.g2_prepare(bytes.fromhex(KAT["g2"][k])) for k in ("gen", "tau", "tau1")}
    yield srs, hs
    for h in hs.values():
        h.free()
    srs.free()


MODEL_SRS = skm.Srs(TAU, SRS_N)


def model(Cxy, z, y, pi):
    return skm.kzg_verify(Cxy, z, y, pi, MODEL_SRS)


def verdict(ctx, hs, Cxy, z, y, pi, g2="gen", tau_g2="tau"):
    return ctx.kzg_verify(hs[g2], hs[tau_g2], Cxy, sb(z), sb(y), pi)


def open_at(ctx, srs, vals, z):
    L = 1 << max(0, (max(len(vals), 1) - 1).bit_length())
    t = ctx.table_upload(km.to_bytes(list(vals) + [5] * (L - len(vals))))
    try:
        Cxy, _ = ctx.kzg_commit(srs, t, len(vals))
        ev, pi, _ = ctx.kzg_open(srs, t, len(vals), sb(z))
    finally:
        t.free()
    return Cxy, km.from_bytes(ev)[0], pi


def poly(n, seed):
    return km.from_bytes(rand_scalars(n, seed)) if n else []


@pytest.mark.parametrize("n,z", [(1, 12345), (2, 7), (5, R - 1), (SRS_N, 99), (5, 0), (5, TAU), (3, None)])
def test_accepts_what_the_device_opens(ctx, kzg, n, z):
    srs, hs = kzg
    vals = [0, 0, 0] if z is None else poly(n, 40 + n)          # z None: the zero polynomial, C = O and y = 0
    z = 31 if z is None else z
    Cxy, y, pi = open_at(ctx, srs, vals, z)
    if n == 1:
        assert pi == INF
    if vals == [0, 0, 0]:
        assert Cxy == INF and y == 0 and pi == INF
    assert model(Cxy, z, y, pi) and verdict(ctx, hs, Cxy, z, y, pi)


def test_refuses_every_tampered_tuple_as_the_model_does(ctx, kzg):
    srs, hs = kzg
    z = 424242
    Cxy, y, pi = open_at(ctx, srs, poly(5, 77), z)
    assert verdict(ctx, hs, Cxy, z, y, pi)
    tampered = [(Cxy, z, y + 1, pi), (Cxy, z, y, ol.g1_add(pi, pi)), (ol.g1_add(Cxy, G), z, y, pi), (Cxy, z + 1, y, pi), (Cxy, z, y, INF), (INF, z, y, pi)]
    for t in tampered:
        assert not model(*t)
        assert not verdict(ctx, hs, *t)
    # C + G with y + 1 is the polynomial plus one: honest again, in the model and on the device
    shifted = (ol.g1_add(Cxy, G), z, y + 1, pi)
    assert model(*shifted) and verdict(ctx, hs, *shifted)
    assert not verdict(ctx, hs, Cxy, z, y, pi, g2="tau", tau_g2="gen")          # the two G2 points swapped
    assert not verdict(ctx, hs, Cxy, z, y, pi, tau_g2="tau1")                   # the SRS of tau + 1
    assert verdict(ctx, hs, Cxy, z, y, pi)                                      # and the honest tuple again


def test_a_proof_point_off_the_curve_is_a_refusal_not_an_error(ctx, kzg):
    srs, hs = kzg
    Cxy, y, pi = open_at(ctx, srs, poly(4, 5), 9)
    bad_pi = pi[:32] + Cxy[32:]
    assert not ol.g1_on_curve(bad_pi)
    assert verdict(ctx, hs, Cxy, 9, y, bad_pi) is False


@pytest.mark.parametrize("count", [1, 2, 4, 62])
@pytest.mark.parametrize("gamma", [0, 1, None])
def test_batched_accepts_the_devices_batched_opening(ctx, kzg, count, gamma):
    srs, hs = kzg
    rng = random.Random(1000 * count + (gamma or 7))
    gamma = rng.randrange(R) if gamma is None else gamma
    z = rng.randrange(R)
    lens = [1 + (3 * k + count) % 9 for k in range(count)]
    tabs = [ctx.table_upload(km.to_bytes(poly(n, 300 + k) + [0] * (16 - n))) for k, n in enumerate(lens)]
    try:
        evals, pi, _ = ctx.kzg_open_batched(srs, tabs, lens, sb(z), sb(gamma))
        comms = b"".join(ctx.kzg_commit(srs, t, n)[0] for t, n in zip(tabs, lens))
    finally:
        for t in tabs:
            t.free()
    assert ctx.kzg_verify_batched(hs["gen"], hs["tau"], comms, sb(z), sb(gamma), evals, pi)
    # one eval off by one: refused unless gamma^k = 0 hides it (gamma = 0 and k > 0), exactly as the reference's combination does
    k = count - 1
    bad = list(evals); bad[k] = sb(km.from_bytes(bad[k])[0] + 1)
    hidden = gamma == 0 and k > 0
    assert ctx.kzg_verify_batched(hs["gen"], hs["tau"], comms, sb(z), sb(gamma), bad, pi) is hidden
    bad0 = list(evals); bad0[0] = sb(km.from_bytes(bad0[0])[0] + 1)
    assert not ctx.kzg_verify_batched(hs["gen"], hs["tau"], comms, sb(z), sb(gamma), bad0, pi)
    assert ctx.kzg_verify_batched(hs["gen"], hs["tau"], comms, sb(z), sb(gamma), evals, pi)


def test_misuse_is_einval_before_any_launch(ctx, kzg, sbn):
    srs, hs = kzg
    Cxy, y, pi = open_at(ctx, srs, poly(4, 6), 11)
    off_curve = Cxy[:32] + pi[32:]
    assert not ol.g1_on_curve(off_curve)
    L = sbn.lib()
    g2, tg2 = hs["gen"].h, hs["tau"].h
    big = R.to_bytes(32, "little")
    fresh = sbn.Context(0)
    ctx.prof_enable(True)
    try:
        foreign = fresh.g2_prepare(bytes.fromhex(KAT["g2"]["gen"]))
        ctx.prof_reset()
        acc = C.c_int(7)
        a = C.byref(acc)
        bad = [(None, tg2, Cxy, sb(11), sb(y), pi, a), (g2, None, Cxy, sb(11), sb(y), pi, a), (g2, tg2, None, sb(11), sb(y), pi, a), (g2, tg2, Cxy, None, sb(y), pi, a),
               (g2, tg2, Cxy, sb(11), None, pi, a), (g2, tg2, Cxy, sb(11), sb(y), None, a), (g2, tg2, Cxy, sb(11), sb(y), pi, None),
               (g2, tg2, Cxy, big, sb(y), pi, a), (g2, tg2, Cxy, sb(11), big, pi, a), (g2, tg2, off_curve, sb(11), sb(y), pi, a), (foreign.h, tg2, Cxy, sb(11), sb(y), pi, a)]
        for args in bad:
            assert L.sbn_kzg_verify(ctx.h, *args) == -1
        assert L.sbn_kzg_verify(None, g2, tg2, Cxy, sb(11), sb(y), pi, a) == -1
        comms, evals = Cxy * 63, sb(y) * 63
        assert L.sbn_kzg_verify_batched(ctx.h, g2, tg2, comms, C.c_size_t(63), sb(11), sb(1), evals, pi, a) == -1
        assert L.sbn_kzg_verify_batched(ctx.h, g2, tg2, Cxy, C.c_size_t(1), sb(11), big, sb(y), pi, a) == -1
        assert L.sbn_kzg_verify_batched(ctx.h, g2, tg2, Cxy, C.c_size_t(1), sb(11), sb(1), big, pi, a) == -1
        assert L.sbn_kzg_verify_batched(ctx.h, g2, tg2, off_curve, C.c_size_t(1), sb(11), sb(1), sb(y), pi, a) == -1
        assert L.sbn_kzg_verify_batched(ctx.h, g2, tg2, None, C.c_size_t(1), sb(11), sb(1), sb(y), pi, a) == -1
        assert acc.value == 7, "a refused call wrote its verdict"
        assert ctx.prof_get() == {}, "a refused call launched something"
        foreign.free()
    finally:
        ctx.prof_enable(False)
        fresh.close()
    assert verdict(ctx, hs, Cxy, 11, y, pi)


def test_launches_of_one_check(ctx, kzg):
    srs, hs = kzg
    Cxy, y, pi = open_at(ctx, srs, poly(6, 8), 13)
    ctx.prof_enable(True)
    try:
        ctx.prof_reset()
        assert verdict(ctx, hs, Cxy, 13, y, pi)
        prof = {k: v[1] for k, v in ctx.prof_get().items()}
    finally:
        ctx.prof_enable(False)
    assert prof == {"k_window_sums": 1, "k_sums_to_host": 1, "k_pairing_products": 1}
