"""GPU: sbn_nizk_* — NIZKGens::new, Instance::new, Instance::is_sat, NIZK::prove and NIZK::verify (snark.rs:162-287) in one call each — against the
literal model of tests/nizk_model.py: the generator sets, the proof's bytes and the transcript's end state on every raw shape whose padding takes another
path and on the two instances only NIZK takes; the digest as opaque bytes of any length; what the verifier refuses, with the transcript untouched — the
comparison of the derived point with the claimed one on its own among it; that the verifier reads its own matrices; what is misuse; the witness check;
the one call against the same work assembled from the calls that existed before it; its launches."""
import collections
import ctypes as C
import random

import pytest

import nizk_model as nm
import oracle_lib as ol
import polyeval_model as pm
import r1cs_model as rm
import r1cs_proof_verify_model as rpvm
from nizk_model import R_MOD, Transcript

pytestmark = pytest.mark.gpu
TR = b"nizk gpu"
DIGEST = bytes(range(100, 132))
_CASES = {}
_HANDLES = []


def _sbs(xs):
    return b"".join(pm.sb(x) for x in xs)


def _mats_bytes(mats):
    return [(r, c, _sbs(v)) for r, c, v in mats]


def case(ctx, key, digest=DIGEST, seed=11):
    """one honest model proof per (raw shape, digest, seed) for the whole module, with the device's generator bundle and instance handle"""
    ck = (key, digest, seed)
    if ck not in _CASES:
        nc, nv, ni, _ = key
        mats, vars_, inputs = nm.instance(key, seed)
        inst = nm.Instance(nc, nv, ni, mats)
        gk = ("gens", inst.nv)
        if gk not in _CASES:
            dg = ctx.nizk_gens_new(nc, nv, ni)
            _HANDLES.append(dg)
            _CASES[gk] = (dg, [ctx.bases_download(b, 0, len(b) + 1) for b in (dg.pc, dg.g3, dg.g4)])
        dg, points = _CASES[gk]
        gens = nm.make_gens(points, inst)
        dinst = ctx.nizk_instance_new(nc, nv, ni, _mats_bytes(mats), digest)
        _HANDLES.append(dinst)
        rnd = nm.random_rnd(inst, 3 + seed)
        tp = Transcript(TR)
        proof = nm.prove(tp, inst, digest, vars_, inputs, gens, rnd)
        _CASES[ck] = dict(key=key, mats=mats, vars=vars_, inputs=inputs, inst=inst, digest=digest, dg=dg, points=points, gens=gens, dinst=dinst, rnd=rnd, proof=proof,
                          data=nm.proof_bytes(proof), state=tp.state())
    return _CASES[ck]


@pytest.fixture(scope="module", autouse=True)
def _free_handles():
    yield
    for h in reversed(_HANDLES):
        h.free()
    del _HANDLES[:]
    _CASES.clear()


def vars_table(ctx, c, length=None):
    """the witness as a table of `length` entries (default: the shortest table that holds it), zeros behind the raw variables"""
    n = nm.sm.npo2(max(len(c["vars"]), 1)) if length is None else length
    return ctx.table_upload(_sbs(nm.pad_vars(c["vars"], n)))


def device_prove(ctx, sbn, c, length=None, dg=None, **kw):
    t = vars_table(ctx, c, length)
    tr = sbn.Transcript(TR)
    try:
        return ctx.nizk_prove(c["dinst"], t, _sbs(c["inputs"]), dg or c["dg"], _sbs(c["rnd"]), tr, **kw), tr.state()
    finally:
        t.free()


def device_verify(ctx, sbn, c, data=None, inputs=None, dinst=None):
    """-> (accepted, the transcript's state behind the call, its state before)"""
    tr = sbn.Transcript(TR)
    before = tr.state()
    ok = ctx.nizk_verify(dinst or c["dinst"], _sbs(c["inputs"] if inputs is None else inputs), c["dg"], c["data"] if data is None else data, tr)
    return ok, tr.state(), before


def model_verify(c, data=None, inputs=None, digest=None, inst=None):
    tv = Transcript(TR)
    ok = nm.verify_bytes(tv, c["data"] if data is None else data, inst or c["inst"], c["digest"] if digest is None else digest, c["inputs"] if inputs is None else inputs, c["gens"])
    return ok, tv.state()


def refused(ctx, sbn, c, **kw):
    ok, state, before = device_verify(ctx, sbn, c, **kw)
    return ok is False and state == before


# ---- 1. the generator bundle --------------------------------------------------------------------------------------------------------

def test_gens_are_the_first_three_sets_of_the_snark_bundle(ctx, sbn):
    key = (5, 3, 2, None)
    c = case(ctx, key)
    want = nm.gens_sizes(5, 3, 2)
    full = ctx.snark_gens_new(5, 3, 2, 16)
    try:
        for k, (n, label), got in zip(("pc", "g3", "g4"), want, c["points"]):
            assert label == b"gens_r1cs_sat" and len(getattr(c["dg"], k)) == n and got == ol.gens_new(n, label)[0], k
            f = getattr(full, k)
            assert ctx.bases_download(f, 0, len(f) + 1) == got, k
        assert c["dg"].ops is None and c["dg"].mem is None and c["dg"].derefs is None
        assert [sbn.lib().sbn_snark_gens_get(c["dg"].h, i) for i in (3, 4, 5, 6, -1)] == [None] * 5
        with pytest.raises(sbn.SbnError, match="rc=-1"):            # SNARK::encode needs the eval sets
            ctx.snark_encode(5, 3, 2, _mats_bytes(c["mats"]), c["dg"])
        assert device_prove(ctx, sbn, c, dg=full) == device_prove(ctx, sbn, c) == (c["data"], c["state"])
    finally:
        full.free()


# ---- 2. prove, byte for byte --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("key", nm.KEYS)
def test_prove_gives_the_models_bytes_and_state(ctx, sbn, key):
    c = case(ctx, key)
    assert nm.sm.is_sat(c["inst"], c["vars"], c["inputs"])[0]
    assert c["dinst"].sizes() == nm.sizes(c["inst"]) == (len(c["rnd"]), len(c["data"]))
    got = device_prove(ctx, sbn, c)
    assert got == (c["data"], c["state"])
    if nm.sm.npo2(max(len(c["vars"]), 1)) != c["inst"].nv:          # the shortest table and the padded one: the same bytes
        assert device_prove(ctx, sbn, c, length=c["inst"].nv) == got
    assert device_prove(ctx, sbn, c, check_sat=True) == got
    assert model_verify(c, data=got[0]) == (True, c["state"])
    assert device_verify(ctx, sbn, c, data=got[0])[:2] == (True, c["state"])


def test_a_table_of_one_variable_is_padded_on_the_device(ctx, sbn):
    c = case(ctx, (2, 1, 3, None))
    assert c["inst"].nv == 4 and len(c["vars"]) == 1
    assert device_prove(ctx, sbn, c, length=1) == device_prove(ctx, sbn, c, length=2) == device_prove(ctx, sbn, c, length=4) == (c["data"], c["state"])


# ---- 3. the digest ------------------------------------------------------------------------------------------------------------------

def test_the_digest_is_absorbed_as_bytes_of_any_length(ctx, sbn):
    key = (4, 4, 1, None)
    digests = [b"", b"\x07", DIGEST, bytes((3 * i + 1) & 0xff for i in range(200))]      # 200 bytes cross STROBE's 166-byte rate inside one message
    cs = [case(ctx, key, digest=d) for d in digests]
    for c in cs:
        assert device_prove(ctx, sbn, c) == (c["data"], c["state"]), len(c["digest"])
        assert device_verify(ctx, sbn, c)[:2] == (True, c["state"]), len(c["digest"])
    assert len({c["data"] for c in cs}) == len(cs) and len({c["state"] for c in cs}) == len(cs)
    a, b = cs[2], cs[3]
    assert model_verify(a, digest=b["digest"])[0] is False
    assert refused(ctx, sbn, a, dinst=b["dinst"]) and refused(ctx, sbn, b, dinst=a["dinst"])      # a verifier holding another digest


# ---- 4. verify ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("key", [(5, 3, 2, None), (4, 4, 1, None)])
def test_verify_refuses_each_tampering(ctx, sbn, key):
    c = case(ctx, key)
    honest = (True, c["state"])
    assert device_verify(ctx, sbn, c)[:2] == honest == model_verify(c)
    t = nm.tamperings(c["data"], c["inst"])
    sat_part = rpvm.tamperings(c["data"][:nm.r_span(c["inst"])["sat"][1]], c["inst"].nc, c["inst"].nv)
    assert set(t) == set(sat_part) | set(nm.R_TAMPERINGS) and len(t) == len(sat_part) + 6
    for name, data in t.items():
        assert model_verify(c, data=data)[0] is False, name
        assert refused(ctx, sbn, c, data=data), name
    wrong = list(c["inputs"]); wrong[-1] = (wrong[-1] + 1) % R_MOD
    assert model_verify(c, inputs=wrong)[0] is False and refused(ctx, sbn, c, inputs=wrong)
    assert device_verify(ctx, sbn, c)[:2] == honest


# ---- 5. the comparison on its own ---------------------------------------------------------------------------------------------------

def test_only_the_comparison_refuses_a_changed_point_on_an_empty_instance(ctx, sbn):
    """A, B, C are 0 at every point of an instance without entries: R1CSProof::verify passes at whatever point the proof claims, returns a point, and the
    point differs from the claim.  A build that forgets the comparison of snark.rs:280-281 accepts this proof."""
    c = case(ctx, nm.ALL_EMPTY)
    inst = c["inst"]
    assert all(len(m[0]) == 0 for m in inst.mats)
    assert device_verify(ctx, sbn, c)[:2] == (True, c["state"])
    rx, ry = c["proof"]["r"]
    claimed = ([(rx[0] + 1) % R_MOD] + rx[1:], ry)
    assert nm.verify(Transcript(TR), dict(sat=c["proof"]["sat"], r=claimed), inst, c["digest"], c["inputs"], c["gens"]) == (True, False)
    data = nm.bump(c["data"], nm.r_span(inst)["rx"][0])
    assert data == nm.proof_bytes(dict(sat=c["proof"]["sat"], r=claimed))
    assert model_verify(c, data=data)[0] is False
    assert refused(ctx, sbn, c, data=data)
    assert refused(ctx, sbn, c, data=nm.bump(c["data"], nm.r_span(inst)["ry"][1] - 32))


# ---- 6. the verifier reads its own matrices -----------------------------------------------------------------------------------------

def test_a_proof_for_one_circuit_is_refused_on_anothers_handle(ctx, sbn):
    a, b = case(ctx, (4, 4, 1, None)), case(ctx, (4, 4, 1, None), seed=12)
    assert a["digest"] == b["digest"] and a["inst"].mats != b["inst"].mats
    for c, other in ((a, b), (b, a)):
        assert device_verify(ctx, sbn, c)[:2] == (True, c["state"])
        assert model_verify(c, inst=other["inst"])[0] is False
        # (the other circuit's own inputs: the statement is the other's in everything but the proof)
        assert refused(ctx, sbn, c, dinst=other["dinst"]) and refused(ctx, sbn, c, dinst=other["dinst"], inputs=other["inputs"])


# ---- 7. the instance ----------------------------------------------------------------------------------------------------------------

def test_instance_new_refuses_each_error_in_the_references_order(ctx, sbn):
    c = case(ctx, (5, 3, 2, None))
    A, B, Cm = c["mats"]

    def with_entry(at, row, col, val):
        rows, cols, vals = list(A[0]), list(A[1]), [pm.sb(v) for v in A[2]]
        rows[at], cols[at], vals[at] = row, col, val
        return [(rows, cols, b"".join(vals)), _mats_bytes([B])[0], _mats_bytes([Cm])[0]]
    one, big = pm.sb(1), R_MOD.to_bytes(32, "little")
    last = len(A[0]) - 1
    for mats, words in ((with_entry(last, 5, 0, one), "entry %d: row 5 >= num_cons 5" % last), (with_entry(1, 0, 6, one), "entry 1: col 6 >= num_vars"),
                        (with_entry(2, 0, 0, big), "entry 2: value >= r"),
                        (with_entry(1, 5, 6, big), "entry 1: row 5"), (with_entry(1, 0, 6, big), "entry 1: col 6")):      # row before col before value
        with pytest.raises(sbn.SbnError, match="rc=-1.*matrix 0 " + words):
            ctx.nizk_instance_new(5, 3, 2, mats, DIGEST)
    ok = ctx.nizk_instance_new(5, 3, 2, with_entry(last, 4, 5, pm.sb(R_MOD - 1)), DIGEST)      # the last row, the last input, the largest value
    ok.free()
    with pytest.raises(sbn.SbnError, match="rc=-1"):                # num_vars_padded = 1
        ctx.nizk_instance_new(2, 1, 0, [([], [], b"")] * 3, DIGEST)
    with pytest.raises(sbn.SbnError, match="rc=-1"):                # flags other than SBN_SCALARS_MONT
        ctx.nizk_instance_new(5, 3, 2, _mats_bytes(c["mats"]), DIGEST, flags=2)


@pytest.mark.parametrize("key", [(5, 3, 2, None), (2, 40, 5, None), nm.ALL_EMPTY])
def test_the_handles_matrices_evaluate_as_the_models(ctx, key):
    c = case(ctx, key)
    inst = c["inst"]
    rng = random.Random(9)
    rx, ry = [rng.randrange(R_MOD) for _ in range(inst.nx)], [rng.randrange(R_MOD) for _ in range(inst.ny)]
    assert (c["dinst"].r1cs.num_cons, c["dinst"].r1cs.num_vars) == (inst.nc, inst.nv)
    assert b"".join(ctx.r1cs_evaluate(c["dinst"].r1cs, _sbs(rx), _sbs(ry))) == _sbs(rm.evaluate(inst.nc, inst.nv, inst.mats, rx, ry))


def _violate(mats, rows):
    """C with the entry of each listed row raised by one: exactly those rows are violated (C holds one entry a row, at index row)"""
    A, B, (cr, cc, cv) = mats
    cv = list(cv)
    for r in rows:
        assert cr[r] == r
        cv[r] = (cv[r] + 1) % R_MOD
    return A, B, (cr, cc, cv)


@pytest.mark.parametrize("key", [(5, 3, 2, None), (2, 1, 3, None), (1, 2, 0, None)])
def test_is_sat_on_raw_shapes_and_short_tables(ctx, sbn, key):
    c = case(ctx, key)
    nc = key[0]
    rows = [0, nc - 1] if nc > 1 else [0]
    bad_mats = _violate(c["mats"], rows)
    want = nm.sm.is_sat(nm.Instance(*key[:3], bad_mats), c["vars"], c["inputs"])
    assert want == (False, len(rows), 0)
    bad = ctx.nizk_instance_new(*key[:3], _mats_bytes(bad_mats), DIGEST)
    tabs = [vars_table(ctx, c), vars_table(ctx, c, c["inst"].nv)]
    try:
        for t in tabs:
            assert ctx.nizk_is_sat(c["dinst"], t, _sbs(c["inputs"])) == (True, 0, 0)
            assert ctx.nizk_is_sat(bad, t, _sbs(c["inputs"])) == want
        with pytest.raises(sbn.SbnError, match="rc=-1"):
            ctx.nizk_is_sat(c["dinst"], tabs[0], _sbs(c["inputs"]) + pm.sb(1))      # one input too many
    finally:
        bad.free()
        for t in tabs:
            t.free()


# ---- 8. misuse ----------------------------------------------------------------------------------------------------------------------

def test_misuse_is_einval_and_launches_nothing(ctx, sbn):
    c = case(ctx, (5, 3, 2, None))
    other = case(ctx, (2, 40, 5, None))                             # another num_vars_padded: gens_pc has another size
    t = vars_table(ctx, c)
    long = ctx.table_upload(_sbs(nm.pad_vars(c["vars"], 8)))
    L = sbn.lib()
    inp, rnd, data = _sbs(c["inputs"]), _sbs(c["rnd"]), c["data"]
    big = R_MOD.to_bytes(32, "little")
    tr = sbn.Transcript(TR)
    before = tr.state()
    p = lambda x: (C.c_uint8 * len(x)).from_buffer_copy(x)          # noqa: E731
    proof = (C.c_uint8 * len(data))(*([0xaa] * len(data)))
    acc = C.c_int(7)
    sat, nb, fb = C.c_int(7), C.c_uint64(7), C.c_uint64(7)
    ni, n = C.c_size_t(2), C.c_size_t(len(data))
    ih, gh = c["dinst"].h, c["dg"].h
    ctx.prof_enable(True)
    try:
        ctx.prof_reset()
        for bad in (data[:-1], data + b"\0", data[:32], other["data"]):                       # a wrong proof_len: one short, one long, others
            with pytest.raises(sbn.SbnError, match="rc=-1"):
                ctx.nizk_verify(c["dinst"], inp, c["dg"], bad, tr)
        with pytest.raises(sbn.SbnError, match="rc=-1"):
            ctx.nizk_verify(c["dinst"], inp[:32], c["dg"], data, tr)                          # a wrong num_inputs
        with pytest.raises(sbn.SbnError, match="rc=-1"):
            ctx.nizk_verify(c["dinst"], inp + inp[:32], c["dg"], data, tr)
        with pytest.raises(sbn.SbnError, match="rc=-1"):
            ctx.nizk_verify(c["dinst"], big + inp[32:], c["dg"], data, tr)                    # an input >= r
        with pytest.raises(sbn.SbnError, match="rc=-1"):
            ctx.nizk_verify(c["dinst"], inp, other["dg"], data, tr)                           # a bundle of another num_vars_padded
        with pytest.raises(sbn.SbnError, match="rc=-1"):
            ctx.nizk_prove(c["dinst"], long, inp, c["dg"], rnd, tr)                           # more variables than num_vars_padded
        with pytest.raises(sbn.SbnError, match="rc=-1"):
            ctx.nizk_prove(c["dinst"], t, inp[:32], c["dg"], rnd, tr)
        with pytest.raises(sbn.SbnError, match="rc=-1"):
            ctx.nizk_prove(c["dinst"], t, inp[:32] + big, c["dg"], rnd, tr)                   # a non-canonical input
        with pytest.raises(sbn.SbnError, match="rc=-1"):
            ctx.nizk_prove(c["dinst"], t, inp, c["dg"], big + rnd[32:], tr)                   # a non-canonical draw: the first, the last
        with pytest.raises(sbn.SbnError, match="rc=-1"):
            ctx.nizk_prove(c["dinst"], t, inp, c["dg"], rnd[:-32] + big, tr)
        with pytest.raises(sbn.SbnError, match="rc=-1"):
            ctx.nizk_prove(c["dinst"], t, inp, other["dg"], rnd, tr)
        with pytest.raises(sbn.SbnError, match="rc=-1"):
            ctx.nizk_is_sat(c["dinst"], long, inp)
        assert L.sbn_nizk_prove(ctx.h, ih, t.h, p(inp), ni, gh, C.c_uint32(2), p(rnd), tr.h, proof) == -1      # an unknown flag
        assert L.sbn_nizk_prove(ctx.h, ih, t.h, p(inp), ni, gh, C.c_uint32(0x80000001), p(rnd), tr.h, proof) == -1
        # each NULL
        prove_args = [ctx.h, ih, t.h, p(inp), ni, gh, C.c_uint32(0), p(rnd), tr.h, proof]
        for k in (0, 1, 2, 3, 5, 7, 8, 9):
            a = list(prove_args); a[k] = None
            assert L.sbn_nizk_prove(*a) == -1, k
        verify_args = [ctx.h, ih, p(inp), ni, gh, p(data), n, tr.h, C.byref(acc)]
        for k in (0, 1, 2, 4, 5, 7, 8):
            a = list(verify_args); a[k] = None
            assert L.sbn_nizk_verify(*a) == -1, k
        sat_args = [ctx.h, ih, t.h, p(inp), ni, C.byref(sat), C.byref(nb), C.byref(fb)]
        for k in (0, 1, 2, 3, 5, 6, 7):
            a = list(sat_args); a[k] = None
            assert L.sbn_nizk_is_sat(*a) == -1, k
        assert ctx.prof_get() == {}, "a refused call launched something"
        assert tr.state() == before and bytes(proof) == b"\xaa" * len(data) and acc.value == 7 and (sat.value, nb.value, fb.value) == (7, 7, 7)
        out = C.c_void_p(7)
        assert L.sbn_nizk_gens_new(ctx.h, C.c_size_t(5), C.c_size_t(3), C.c_size_t(2), None) == -1 and L.sbn_nizk_gens_new(None, C.c_size_t(5), C.c_size_t(3), C.c_size_t(2), C.byref(out)) == -1
        assert L.sbn_nizk_sizes(None, None, None) == -1 and L.sbn_nizk_instance_r1cs(None) is None
        L.sbn_nizk_instance_free(ctx.h, None)
    finally:
        ctx.prof_enable(False)
        t.free(); long.free()
    assert device_verify(ctx, sbn, c)[:2] == (True, c["state"])


# ---- 9. SBN_SNARK_CHECK_SAT ---------------------------------------------------------------------------------------------------------

def test_check_sat_stops_a_bad_witness_before_any_proving_launch(ctx, sbn):
    c = case(ctx, (5, 3, 2, None))
    wrong = dict(c, vars=[(c["vars"][0] + 1) % R_MOD] + c["vars"][1:])
    want = nm.sm.is_sat(c["inst"], wrong["vars"], c["inputs"])
    assert want[0] is False
    t = vars_table(ctx, wrong)
    L = sbn.lib()
    tr = sbn.Transcript(TR)
    before = tr.state()
    proof = (C.c_uint8 * len(c["data"]))(*([0xaa] * len(c["data"])))
    p = lambda x: (C.c_uint8 * len(x)).from_buffer_copy(x)          # noqa: E731
    ctx.prof_enable(True)
    try:
        ctx.prof_reset()
        rc = L.sbn_nizk_prove(ctx.h, c["dinst"].h, t.h, p(_sbs(c["inputs"])), C.c_size_t(len(c["inputs"])), c["dg"].h, C.c_uint32(sbn.SBN_SNARK_CHECK_SAT), p(_sbs(c["rnd"])), tr.h, proof)
        prof = {k: v[1] for k, v in ctx.prof_get().items()}
    finally:
        ctx.prof_enable(False)
    try:
        assert rc == sbn.SBN_EUNSAT == -5
        assert tr.state() == before and bytes(proof) == b"\xaa" * len(c["data"])
        assert prof["k_r1cs_sat_check"] == 1 and set(prof) <= {"k_r1cs_build_z", "k_r1cs_spmv", "k_r1cs_fix", "k_r1cs_sat_check"}, prof
        with pytest.raises(sbn.SbnUnsat, match="%d constraints, the first is row %d" % want[1:]):
            ctx.nizk_prove(c["dinst"], t, _sbs(c["inputs"]), c["dg"], _sbs(c["rnd"]), tr, check_sat=True)
        # without the flag the library proves what it is given, and the verifier refuses the proof
        data = ctx.nizk_prove(c["dinst"], t, _sbs(c["inputs"]), c["dg"], _sbs(c["rnd"]), sbn.Transcript(TR))
        assert model_verify(c, data=data)[0] is False
        assert refused(ctx, sbn, c, data=data)
    finally:
        t.free()
    assert device_prove(ctx, sbn, c, check_sat=True) == (c["data"], c["state"])


# ---- 10. one call equals the sequence ------------------------------------------------------------------------------------------------

def _assembled_prove(ctx, sbn, dinst, digest, vt, inp, dg, rnd):
    tr = sbn.Transcript(TR)
    tr.append_message(b"protocol-name", nm.NAME); tr.append_message(b"R1CSShapeDigest", digest)
    sat, rx, ry = ctx.r1cs_proof_prove(dinst.r1cs, vt, inp, dg.pc, dg.g3, dg.g4, rnd, tr)
    return sat + rx + ry, tr.state()


def _assembled_verify(ctx, sbn, dinst, digest, inp, dg, data):
    """-> (verdict, the transcript's state behind the last call)"""
    nc, nv = dinst.r1cs.num_cons, dinst.r1cs.num_vars
    nx, ny = nc.bit_length() - 1, nv.bit_length()
    n_sat = len(data) - 32 * (nx + ny)
    crx, cry = data[n_sat:n_sat + 32 * nx], data[n_sat + 32 * nx:]
    tr = sbn.Transcript(TR)
    tr.append_message(b"protocol-name", nm.NAME); tr.append_message(b"R1CSShapeDigest", digest)
    evals = b"".join(ctx.r1cs_evaluate(dinst.r1cs, crx, cry))
    got = ctx.r1cs_proof_verify(nc, nv, inp, evals, dg.pc, dg.g3, dg.g4, data[:n_sat], tr)
    return got is not None and got == (crx, cry), tr.state()


def test_one_call_equals_the_assembled_sequence_where_the_sumchecks_take_many_blocks(ctx, sbn):
    """device against device, no model: 2^10 x 2^10 padded, a few thousand entries"""
    nc, nv, ni = 1000, 1000, 5
    mats, vars_, inputs = nm.sm.satisfying_instance(nc, nv, ni, seed=21)
    assert 3000 < sum(len(m[0]) for m in mats) < 8000
    digest = bytes(range(64))
    dinst = ctx.nizk_instance_new(nc, nv, ni, _mats_bytes(mats), digest)
    dg = ctx.nizk_gens_new(nc, nv, ni)
    vt = ctx.table_upload(_sbs(nm.pad_vars(vars_, 1024)))
    try:
        assert (dinst.r1cs.num_cons, dinst.r1cs.num_vars) == (1024, 1024)
        assert ctx.nizk_is_sat(dinst, vt, _sbs(inputs)) == (True, 0, 0)
        rng = random.Random(4)
        rnd = _sbs([rng.randrange(R_MOD) for _ in range(dinst.sizes()[0])])
        inp = _sbs(inputs)
        tr = sbn.Transcript(TR)
        one = ctx.nizk_prove(dinst, vt, inp, dg, rnd, tr), tr.state()
        assert one == _assembled_prove(ctx, sbn, dinst, digest, vt, inp, dg, rnd) and len(one[0]) == dinst.sizes()[1]
        tr = sbn.Transcript(TR)
        assert (ctx.nizk_verify(dinst, inp, dg, one[0], tr), tr.state()) == _assembled_verify(ctx, sbn, dinst, digest, inp, dg, one[0]) == (True, one[1])
        n_sat = len(one[0]) - 32 * 21
        for data in (nm.bump(one[0], n_sat), nm.bump(one[0], len(one[0]) - 32), nm.bump(one[0], n_sat - 32)):      # rx[0], the last of ry, the last scalar of the R1CS proof
            tr = sbn.Transcript(TR)
            before = tr.state()
            assert ctx.nizk_verify(dinst, inp, dg, data, tr) is False and tr.state() == before
            assert _assembled_verify(ctx, sbn, dinst, digest, inp, dg, data)[0] is False
    finally:
        vt.free(); dg.free(); dinst.free()


# ---- 11. launch counts --------------------------------------------------------------------------------------------------------------

def test_launch_counts(ctx, sbn):
    c = case(ctx, (5, 3, 2, None))
    inst = c["inst"]
    inp, rnd = _sbs(c["inputs"]), _sbs(c["rnd"])
    device_prove(ctx, sbn, c)                                       # (the derived sets are built by now)
    t = vars_table(ctx, c, inst.nv)
    sp = nm.r_span(inst)
    crx, cry = c["data"][slice(*sp["rx"])], c["data"][slice(*sp["ry"])]
    evals = b"".join(ctx.r1cs_evaluate(c["dinst"].r1cs, crx, cry))

    def prefixed():
        tr = sbn.Transcript(TR)
        tr.append_message(b"protocol-name", nm.NAME); tr.append_message(b"R1CSShapeDigest", c["digest"])
        return tr
    runs = dict(prove=lambda: ctx.nizk_prove(c["dinst"], t, inp, c["dg"], rnd, sbn.Transcript(TR)),
                sat_prove=lambda: ctx.r1cs_proof_prove(c["dinst"].r1cs, t, inp, c["dg"].pc, c["dg"].g3, c["dg"].g4, rnd, prefixed()),
                verify=lambda: device_verify(ctx, sbn, c)[0],
                evaluate=lambda: ctx.r1cs_evaluate(c["dinst"].r1cs, crx, cry),
                sat_verify=lambda: ctx.r1cs_proof_verify(inst.nc, inst.nv, inp, evals, c["dg"].pc, c["dg"].g3, c["dg"].g4, c["data"][:sp["sat"][1]], prefixed()))
    counts = {}
    ctx.prof_enable(True)
    try:
        for name, run in runs.items():
            ctx.prof_reset()
            assert run()
            counts[name] = collections.Counter({k: v[1] for k, v in ctx.prof_get().items()})
    finally:
        ctx.prof_enable(False)
        t.free()
    assert counts["verify"]["k_r1cs_spmv_eval"] == 1 and "k_r1cs_spmv_eval" not in counts["sat_verify"]
    assert counts["verify"] == counts["evaluate"] + counts["sat_verify"]      # the evaluation, and otherwise the kernels of sbn_r1cs_proof_verify
    assert counts["prove"] == counts["sat_prove"]                   # a prove is the R1CS proof alone
    assert not [k for k in counts["prove"] if k.startswith(("k_dense_", "k_se_", "k_pp_", "k_dk_")) or k in ("k_r1cs_spmv_eval", "k_r1cs_sat_check")], counts["prove"]
