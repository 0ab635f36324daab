"""GPU: sbn_g1_decompress / sbn_bases_from_compressed against the oracle's g1_decompress, bit for bit, flags included."""
import pytest

import oracle_lib as ol
import polyeval_model as pm

pytestmark = pytest.mark.gpu
Q_MOD = 0x30644e72e131a029b85045b68181585d97816a916871ca8d3c208c16d87cfd47
SIZES = [1, 63, 64, 65, 300]


def _refused_by_incrementing(comp, want_geq_p):
    """increment the x of a valid compressed point until the oracle refuses it; want_geq_p: start from the largest x values instead"""
    flags = comp[31] & 0x80
    x = int.from_bytes(comp, "little") & ((1 << 254) - 1)
    if want_geq_p:
        x = Q_MOD + (x % 1000)                              # below 2^254: it fits the 254 bits under the flags
        assert x < 1 << 254
    while True:
        x += 1
        c = bytearray(x.to_bytes(32, "little")); c[31] |= flags
        if ol.g1_decompress(bytes(c)) is None:
            return bytes(c)


_BATCH = {}


def _batch(n):
    """n compressed entries with their class: oracle points of both signs, the identity, x >= p, x^3 + 3 a non-residue; reference computed once"""
    if n not in _BATCH:
        pts = ol.g1_mul_gen_batch(b"".join(pm.sb(7 * i + 3) for i in range(n)), 1)
        entries, classes = [], []
        for i in range(n):
            c = ol.g1_compress(pts[64 * i:64 * i + 64])
            kind = None if n == 1 else ("inf", "geq_p", "nonres", None, None, None)[i % 6]      # None: the point itself
            if kind == "inf":
                c = ol.g1_compress(pm.INF)
            elif kind == "geq_p":
                c = _refused_by_incrementing(c, True)
            elif kind == "nonres":
                c = _refused_by_incrementing(c, False)
            if kind in (None, "pos", "neg"):
                kind = "neg" if c[31] & 0x80 else "pos"
            entries.append(c); classes.append(kind)
        want = [ol.g1_decompress(c) for c in entries]
        _BATCH[n] = (b"".join(entries), classes, want)
    return _BATCH[n]


def test_the_fixture_holds_every_class():
    seen = set()
    for n in SIZES:
        comp, classes, want = _batch(n)
        seen |= set(classes)
        for c, k, w in zip((comp[32 * i:32 * i + 32] for i in range(n)), classes, want):
            x = int.from_bytes(c, "little") & ((1 << 254) - 1)
            if k == "inf":
                assert w == pm.INF and c[31] == 0x40
            elif k == "geq_p":
                assert w is None and x >= Q_MOD
            elif k == "nonres":
                assert w is None and x < Q_MOD
            else:
                assert w is not None and w != pm.INF and ol.g1_compress(w) == c and bool(c[31] & 0x80) == (k == "neg")
    assert seen == {"pos", "neg", "inf", "geq_p", "nonres"}
    for n in SIZES[1:]:
        assert set(_batch(n)[1]) == {"pos", "neg", "inf", "geq_p", "nonres"}


@pytest.mark.parametrize("n", SIZES)
def test_decompress_equals_the_oracle_entry_by_entry(ctx, n):
    comp, _, want = _batch(n)
    xy, ok = ctx.g1_decompress(comp)
    assert len(xy) == 64 * n and len(ok) == n
    for i in range(n):
        assert ok[i] == (0 if want[i] is None else 1), i
        assert xy[64 * i:64 * i + 64] == (pm.INF if want[i] is None else want[i]), i


def test_decompress_inverts_the_librarys_compress(ctx, sbn):
    pts = ol.g1_mul_gen_batch(b"".join(pm.sb(11 * i + 1) for i in range(70)), 1) + pm.INF
    xy, ok = ctx.g1_decompress(sbn.g1_compress(pts))
    assert xy == pts and ok == bytes([1] * 71)
    assert ctx.g1_decompress(b"") == (b"", b"")


@pytest.mark.parametrize("n", [1, 65, 300])
def test_bases_from_compressed_round_trips_and_reports_the_first_bad_index(ctx, sbn, n):
    comp, classes, want = _batch(n)
    good = [i for i in range(n) if want[i] is not None]
    gc = b"".join(comp[32 * i:32 * i + 32] for i in good)
    b = ctx.bases_from_compressed(gc)
    try:
        assert len(b) == len(good)
        assert ctx.bases_download(b, 0, len(good)) == b"".join(want[i] for i in good)
    finally:
        b.free()
    bad = [i for i in range(n) if want[i] is None]
    if bad:
        with pytest.raises(sbn.SbnError) as e:
            ctx.bases_from_compressed(comp)
        assert e.value.bad_index == bad[0]


def test_a_set_from_compressed_bytes_serves_the_msm_with_identities_in_it(ctx):
    """identity points in a resident set are ordinary: zero rows of a commitment (hyrax.rs:245 padding)"""
    n = 40
    pts = [ol.g1_mul_gen_batch(pm.sb(5 * i + 2), 1) if i % 3 else pm.INF for i in range(n)]
    b = ctx.bases_from_compressed(b"".join(ol.g1_compress(p) for p in pts))
    try:
        scal = [pow(3, i + 1, pm.R_MOD) for i in range(n)]
        got, inf = ctx.msm_bases(b, b"".join(pm.sb(s) for s in scal))
        assert got == pm.msm(scal, pts) and not inf
    finally:
        b.free()
