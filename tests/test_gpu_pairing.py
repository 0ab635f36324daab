"""GPU: sbn_g2_prepare + sbn_pairing_products (k_pairing_products: one wave a product, the Fq12 product shared by the wave's lanes, the exact final
exponentiation) against the GT bytes tests/golden/pairing_kat.json holds from the literal model (tests/pairing_model.py): single pairings, products
of one to four terms, the identity as a term, the empty product, a product that is one, a handle used twice, bilinearity, many checks in one
launch, the refusals and the launches."""
import ctypes as C

import pytest

from conftest import golden
import pairing_model as pm

pytestmark = pytest.mark.gpu
KAT = golden("pairing_kat.json")
CASES = {c["name"]: c for c in KAT["cases"]}
Q_MOD = pm.Q


@pytest.fixture(scope="module")
def lines(ctx):
    hs = {k: ctx.g2_prepare(bytes.fromhex(v)) for k, v in KAT["g2"].items()}
    yield hs
    for h in hs.values():
        h.free()


def run(ctx, lines, names, want_gt=True):
    """the named cases as the checks of ONE call -> (is_one list, gt list)"""
    p, q, counts = b"", [], []
    for n in names:
        terms = CASES[n]["terms"]
        p += b"".join(bytes.fromhex(t[0]) for t in terms)
        q += [lines[t[1]] for t in terms]
        counts.append(len(terms))
    one, gt = ctx.pairing_products(p, q, counts, want_gt)
    assert len(one) == len(names) and (gt is None or len(gt) == len(names))
    return list(one), gt


def check(ctx, lines, names):
    one, gt = run(ctx, lines, names)
    for i, n in enumerate(names):
        assert gt[i].hex() == CASES[n]["gt"], (i, n)
        assert one[i] == (1 if CASES[n]["is_one"] else 0), (i, n)


@pytest.mark.parametrize("name", list(CASES))
def test_gt_bytes_equal_the_models(ctx, lines, name):
    check(ctx, lines, [name])


def test_the_fixture_has_the_cases_the_kernel_can_get_wrong():
    assert [len(CASES[n]["terms"]) for n in ("gen", "two", "three", "four", "empty")] == [1, 2, 3, 4, 0]
    assert CASES["identity_term"]["terms"][1][0] == bytes(64).hex() and CASES["only_identity"]["terms"][0][0] == bytes(64).hex()
    assert CASES["cancel"]["is_one"] and CASES["cancel"]["gt"] == pm.GT_ONE.hex() and CASES["empty"]["gt"] == pm.GT_ONE.hex()
    assert len({t[1] for t in CASES["same_handle_twice"]["terms"]}) == 1
    assert sum(1 for c in CASES.values() if not c["is_one"]) >= 9


def test_device_bilinearity(ctx, lines):
    """e(aP, bQ) from the device == e(P, Q)^(ab) from the model's square-and-multiply"""
    _, gt = run(ctx, lines, [KAT["bilinear"]["case"]])
    assert gt[0].hex() == KAT["bilinear"]["gt_pow_ab"]


@pytest.mark.parametrize("nchecks", [1, 2, 65])
def test_every_check_of_a_call_is_its_own(ctx, lines, nchecks):
    order = list(CASES)
    names = [order[(5 * i + nchecks) % len(order)] for i in range(nchecks)]
    assert nchecks < len(order) or set(names) == set(order)
    check(ctx, lines, names)


def test_a_check_that_is_one_between_two_that_are_not(ctx, lines):
    names = ["pair1", "cancel", "two", "empty", "four"]
    check(ctx, lines, names)
    one, gt = run(ctx, lines, names, want_gt=False)
    assert gt is None and one == [0, 1, 0, 1, 0]


def test_two_contexts_agree_and_an_msm_before_changes_nothing(ctx, lines, sbn, ol):
    names = ["gen", "three", "cancel"]
    first = run(ctx, lines, names)
    fresh = sbn.Context(0)
    hs = {}
    try:
        pts = ol.g1_mul_gen_batch(b"".join((7 * i + 3).to_bytes(32, "little") for i in range(100)), 1)
        fresh.msm(b"".join(pow(11, i + 1, pm.R).to_bytes(32, "little") for i in range(100)), pts)
        hs = {k: fresh.g2_prepare(bytes.fromhex(v)) for k, v in KAT["g2"].items()}
        assert run(fresh, hs, names) == first
        with pytest.raises(sbn.SbnError):                                   # a handle of another context
            run(fresh, lines, ["gen"])
    finally:
        for h in hs.values():
            h.free()
        fresh.close()


def test_g2_prepare_refuses_what_is_not_a_point_of_g2(ctx, sbn):
    gen = bytes.fromhex(KAT["g2"]["gen"])
    x_plus_q = (int.from_bytes(gen[:32], "little") + Q_MOD).to_bytes(32, "little") + gen[32:]
    off_curve = gen[:64] + bytes.fromhex(KAT["g2"]["s1"])[64:]
    bad = [x_plus_q, off_curve, bytes(128)] + [bytes.fromhex(h) for h in KAT["g2_off_subgroup"]]
    assert all(pm.g2_on_curve(_g2(b)) for b in bad[3:]) and not pm.g2_on_curve(_g2(off_curve))
    for b in bad:
        with pytest.raises(sbn.SbnError):
            ctx.g2_prepare(b)
    with pytest.raises(sbn.SbnError):
        ctx.g2_prepare(gen, flags=4)
    out = C.c_void_p()
    assert sbn.lib().sbn_g2_prepare(ctx.h, None, 0, C.byref(out)) == -1 and sbn.lib().sbn_g2_prepare(ctx.h, gen, 0, None) == -1 and not out.value


def _g2(b):
    c = [int.from_bytes(b[32 * i:32 * i + 32], "little") for i in range(4)]
    return ((c[0], c[1]), (c[2], c[3]))


def test_montgomery_limbs_give_the_same_handle(ctx, lines):
    gen = bytes.fromhex(KAT["g2"]["gen"])
    mont = b"".join((int.from_bytes(gen[32 * i:32 * i + 32], "little") * (1 << 256) % Q_MOD).to_bytes(32, "little") for i in range(4))
    h = ctx.g2_prepare(mont, flags=2)
    try:
        assert run(ctx, {"gen": h}, ["gen"])[1][0].hex() == CASES["gen"]["gt"]
    finally:
        h.free()


def test_refusals_come_before_any_launch(ctx, lines, sbn):
    P = [bytes.fromhex(t[0]) for t in CASES["four"]["terms"]]
    off_curve = P[0][:32] + P[1][32:]
    x_plus_q = (int.from_bytes(P[0][:32], "little") + Q_MOD).to_bytes(32, "little") + P[0][32:]
    g = lines["gen"]
    L = sbn.lib()
    ctx.prof_enable(True)
    try:
        ctx.prof_reset()
        for p, q, counts in ((b"".join(P) + P[0], [g] * 5, [5]), (off_curve, [g], [1]), (x_plus_q, [g], [1]), (P[0] + off_curve, [g, g], [1, 1])):
            with pytest.raises(sbn.SbnError):
                ctx.pairing_products(p, q, counts)
        one, gt = (C.c_uint8 * 1)(7), (C.c_uint8 * 384)(*([7] * 384))
        cnt = (C.c_uint32 * 1)(1)
        pbuf = (C.c_uint8 * 64).from_buffer_copy(P[0])
        arr = (C.c_void_p * 1)(g.h)
        null_handle = (C.c_void_p * 1)(None)
        for args in ((None, arr, cnt, one), (pbuf, None, cnt, one), (pbuf, arr, None, one), (pbuf, arr, cnt, None), (pbuf, null_handle, cnt, one)):
            assert L.sbn_pairing_products(ctx.h, args[0], args[1], args[2], C.c_size_t(1), args[3], gt) == -1
        assert L.sbn_pairing_products(None, pbuf, arr, cnt, C.c_size_t(1), one, gt) == -1
        assert bytes(one) == b"\x07" and bytes(gt) == b"\x07" * 384, "a refused call wrote an output"
        assert ctx.pairing_products(b"", [], []) == (b"", [])
        assert ctx.prof_get() == {}, "a refused call launched something"
    finally:
        ctx.prof_enable(False)
    check(ctx, lines, ["pair2"])                                            # and the context serves the next call


@pytest.mark.parametrize("nchecks", [1, 65])
def test_one_launch_whatever_the_number_of_checks(ctx, lines, nchecks):
    order = list(CASES)
    names = [order[i % len(order)] for i in range(nchecks)]
    ctx.prof_enable(True)
    try:
        ctx.prof_reset()
        check(ctx, lines, names)
        prof = {k: v[1] for k, v in ctx.prof_get().items()}
    finally:
        ctx.prof_enable(False)
    assert prof == {"k_pairing_products": 1}
