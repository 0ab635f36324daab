"""GPU: sbn_snark_* and sbn_r1cs_is_sat — SNARKGens::new, Instance::new + SNARK::encode, Instance::is_sat, SNARK::prove and SNARK::verify (snark.rs:59-158,
:290-529) in one call each — against the literal model of tests/snark_model.py: the commitment's bytes, the proof's bytes and the transcript's end state
on every raw shape whose padding takes another path, both builds; what the verifier refuses, with the transcript untouched, on a key from encode and on
a key made of the commitment's bytes; what is misuse; the witness check's verdict, count and first row; its launches."""
import ctypes as C
import random

import pytest

from conftest import golden
import oracle_lib as ol
import polyeval_model as pm
import r1cs_model as rm
import snark_model as sm
import sparse_eval_kzg_model as skm
import sparse_eval_model as sem
from snark_model import R_MOD, Transcript

pytestmark = pytest.mark.gpu
TR = b"snark gpu"
# raw (num_cons, num_vars, num_inputs, the matrix left empty): already padded; both padded and the columns shifted; num_inputs + 1 decides num_vars_padded;
# num_cons raised to 2; nx > ny; ny > nx; an empty B
CASES = [(4, 4, 1, None), (5, 3, 2, None), (2, 1, 3, None), (1, 2, 0, None), (40, 4, 2, None), (2, 40, 5, None), (6, 5, 1, 1)]
KZG_CASES = [(5, 3, 2, None), (4, 4, 1, None)]
TAMPER_CASES = [(5, 3, 2, None), (4, 4, 1, None)]
KAT = golden("pairing_kat.json")
TAU = int(KAT["tau"], 16)
_CASES = {}


def _sbs(xs):
    return b"".join(pm.sb(x) for x in xs)


def _mats_bytes(mats):
    return [(r, c, _sbs(v)) for r, c, v in mats]


def _instance(key, seed):
    nc, nv, ni, empty = key
    return sm.satisfying_instance(nc, nv, ni, seed=seed, empty=empty, min_entries=2 if nc == 1 else 1)


def case(ctx, key, seed=11, kzg=False):
    """one honest model proof per (raw shape, seed, build) for the whole module, with the device's generator bundle and key"""
    ck = (key, seed, kzg)
    if ck not in _CASES:
        nc, nv, ni, _ = key
        mats, vars_, inputs = _instance(key, seed)
        inst = sm.Instance(nc, nv, ni, mats)
        nnz = max(len(m[0]) for m in mats)
        assert sm.num_ops(inst) >= 2
        base = case(ctx, key, seed) if kzg else None                # the KZG build shares the bundle and the key with the Hyrax build
        if base is None:
            dg = ctx.snark_gens_new(nc, nv, ni, nnz)
            points = [ctx.bases_download(getattr(dg, k), 0, len(getattr(dg, k)) + 1) for k in dg.KINDS]
            gens = sm.make_gens(points, inst)
            comm = sm.encode(inst, gens)
            dkey = ctx.snark_encode(nc, nv, ni, _mats_bytes(mats), dg)
        else:
            dg, points, gens, comm, dkey = (base[k] for k in ("dg", "points", "gens", "comm", "dkey"))
        shape = sem.Shape(inst.nx, inst.ny, comm["N"], 3)
        srs_n = (1 << shape.ell["derefs"]) + 1
        srs = skm.Srs(TAU, srs_n) if kzg else None
        rnd = sm.random_rnd(comm, 3 + seed, kzg)
        tp = Transcript(TR)
        data = sm.proof_bytes(sm.prove(tp, inst, comm, vars_, inputs, gens, rnd, srs), kzg)
        _CASES[ck] = dict(key=key, mats=mats, vars=vars_, inputs=inputs, inst=inst, nnz=nnz, dg=dg, points=points, gens=gens, comm=comm, dkey=dkey, owner=base is None,
                          srs=srs, srs_n=srs_n, rnd=rnd, data=data, state=tp.state())
    return _CASES[ck]


@pytest.fixture(scope="module", autouse=True)
def _free_handles():
    yield
    for c in _CASES.values():
        if c["owner"]:
            c["dkey"].free(); c["dg"].free()
    _CASES.clear()


@pytest.fixture(scope="module")
def g2h(ctx):
    hs = {k: ctx.g2_prepare(bytes.fromhex(KAT["g2"][k])) for k in ("gen", "tau")}
    yield hs
    for h in hs.values():
        h.free()


def vars_table(ctx, c, length=None):
    """the witness as a table of `length` entries (default: the shortest table that holds it), zeros behind the raw variables"""
    n = sm.npo2(max(len(c["vars"]), 1)) if length is None else length
    return ctx.table_upload(_sbs(sm.pad_vars(c["vars"], n)))


def device_prove(ctx, sbn, c, length=None, **kw):
    t = vars_table(ctx, c, length)
    tr = sbn.Transcript(TR)
    try:
        return ctx.snark_prove(c["dkey"], t, _sbs(c["inputs"]), c["dg"], _sbs(c["rnd"]), tr, **kw), tr.state()
    finally:
        t.free()


def device_verify(ctx, sbn, c, data=None, inputs=None, dkey=None, **kw):
    """-> (accepted, the transcript's state behind the call, its state before)"""
    tr = sbn.Transcript(TR)
    before = tr.state()
    ok = ctx.snark_verify(dkey or c["dkey"], _sbs(c["inputs"] if inputs is None else inputs), c["dg"], c["data"] if data is None else data, tr, **kw)
    return ok, tr.state(), before


def model_verify(c, data=None, inputs=None, comm=None):
    tv = Transcript(TR)
    ok = sm.verify_bytes(tv, c["data"] if data is None else data, comm or c["comm"], c["inputs"] if inputs is None else inputs, c["gens"], c["srs"])
    return ok, tv.state()


# ---- the generator bundle and encode -----------------------------------------------------------------------------------------------

def test_gens_are_the_six_sets_under_the_two_labels(ctx):
    c = case(ctx, (5, 3, 2, None))
    want = sm.gens_sizes(5, 3, 2, c["nnz"])
    assert [lab for _, lab in want] == [b"gens_r1cs_sat"] * 3 + [b"gens_r1cs_eval"] * 3
    for k, (n, label), got in zip(c["dg"].KINDS, want, c["points"]):
        assert len(getattr(c["dg"], k)) == n and got == ol.gens_new(n, label)[0], k


@pytest.mark.parametrize("key", CASES)
def test_encode_gives_the_models_commitment(ctx, key):
    c = case(ctx, key)
    want = sm.comm_bytes(c["comm"])
    assert c["dkey"].comm() == want
    assert c["dkey"].sizes() == sm.sizes(c["comm"]) and c["dkey"].sizes(True) == sm.sizes(c["comm"], True)
    vk = ctx.snark_key_from_comm(want)
    try:
        assert vk.comm() == want and vk.dense is None and vk.sizes() == c["dkey"].sizes()
    finally:
        vk.free()


def test_encode_refuses_each_error_of_instance_new(ctx, sbn):
    c = case(ctx, (5, 3, 2, None))
    A, B, Cm = c["mats"]

    def with_entry(row, col, val):
        """A with its last entry replaced: the number of entries, and with it N, stays"""
        return [(A[0][:-1] + [row], A[1][:-1] + [col], _sbs(A[2][:-1]) + val), _mats_bytes([B])[0], _mats_bytes([Cm])[0]]
    one = pm.sb(1)
    for name, mats in (("row = num_cons", with_entry(5, 0, one)), ("col = num_vars + 1 + num_inputs", with_entry(0, 6, one)), ("value = r", with_entry(0, 0, R_MOD.to_bytes(32, "little")))):
        with pytest.raises(sbn.SbnError, match="rc=-1"):
            ctx.snark_encode(5, 3, 2, mats, c["dg"])
    ok = ctx.snark_encode(5, 3, 2, with_entry(4, 5, pm.sb(R_MOD - 1)), c["dg"])      # the last row, the last input, the largest value
    ok.free()
    other = case(ctx, (4, 4, 1, None))
    with pytest.raises(sbn.SbnError, match="rc=-1"):                # a bundle made for another shape
        ctx.snark_encode(5, 3, 2, _mats_bytes(c["mats"]), other["dg"])
    with pytest.raises(sbn.SbnError, match="rc=-1"):                # num_vars_padded = 1
        ctx.snark_encode(2, 1, 0, _mats_bytes(c["mats"]), c["dg"])


def test_key_from_comm_refuses_malformed_bytes(ctx, sbn):
    c = case(ctx, (5, 3, 2, None))
    good = sm.comm_bytes(c["comm"])

    def field(k, v):
        b = bytearray(good); b[8 * k:8 * k + 8] = v.to_bytes(8, "little")
        return bytes(b)
    x = 1
    while ol.g1_decompress(x.to_bytes(32, "little")) is not None:
        x += 1
    bad_point = good[:48] + x.to_bytes(32, "little") + good[80:]
    trials = [good[:47], good[:-1], good + b"\0", field(0, 6), field(1, 3), field(2, 4), field(3, 2), field(4, 1), field(4, 12), field(5, 16), bad_point, good[:-32] + x.to_bytes(32, "little")]
    for b in trials:
        assert sm.comm_from_bytes(b) is None
        with pytest.raises(sbn.SbnError, match="rc=-1"):
            ctx.snark_key_from_comm(b)


# ---- prove, byte for byte ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("key", CASES)
def test_prove_gives_the_models_bytes_and_state(ctx, sbn, key):
    c = case(ctx, key)
    assert sm.is_sat(c["inst"], c["vars"], c["inputs"])[0]
    got = device_prove(ctx, sbn, c)
    assert got == (c["data"], c["state"])
    assert model_verify(c, data=got[0]) == (True, c["state"])
    if sm.npo2(max(len(c["vars"]), 1)) != c["inst"].nv:              # the shortest table and the padded one: the same bytes
        assert device_prove(ctx, sbn, c, length=c["inst"].nv) == got
    assert device_prove(ctx, sbn, c, check_sat=True) == got
    assert device_verify(ctx, sbn, c, data=got[0])[:2] == (True, c["state"])


def test_a_table_of_one_variable_is_padded_on_the_device(ctx, sbn):
    c = case(ctx, (2, 1, 3, None))
    assert c["inst"].nv == 4 and len(c["vars"]) == 1
    assert device_prove(ctx, sbn, c, length=1) == device_prove(ctx, sbn, c, length=2) == device_prove(ctx, sbn, c, length=4) == (c["data"], c["state"])


@pytest.mark.parametrize("key", KZG_CASES)
def test_the_kzg_build_with_and_without_a_derefs_key(ctx, sbn, g2h, key):
    c = case(ctx, key, kzg=True)
    srs = ctx.kzg_srs_from_tau(_sbs([TAU]), c["srs_n"])
    dk = ctx.derefs_key_build(c["dkey"].dense, srs)
    try:
        for k in (None, dk):
            assert device_prove(ctx, sbn, c, srs=srs, derefs_key=k) == (c["data"], c["state"])
        assert model_verify(c) == (True, c["state"])
        assert device_verify(ctx, sbn, c, g2=g2h["gen"], tau_g2=g2h["tau"])[:2] == (True, c["state"])
        sp = sm.proof_spans(c["comm"], True)
        for name, at in (("comm_derefs", sp["eval"][0]), ("the sat half", sp["sat"][1] - 32), ("the eval half", sp["eval"][1] - 32), ("inst_evals[2]", sp["evals"][0] + 64)):
            b = bytearray(c["data"]); b[at] ^= 1
            assert model_verify(c, data=bytes(b))[0] is False, name
            ok, state, before = device_verify(ctx, sbn, c, data=bytes(b), g2=g2h["gen"], tau_g2=g2h["tau"])
            assert ok is False and state == before, name
        assert device_verify(ctx, sbn, c, g2=g2h["tau"], tau_g2=g2h["gen"])[0] is False
        with pytest.raises(sbn.SbnError, match="rc=-1"):            # the Hyrax build's proof length
            device_verify(ctx, sbn, c, data=case(ctx, key)["data"], g2=g2h["gen"], tau_g2=g2h["tau"])
    finally:
        dk.free(); srs.free()


# ---- verify ------------------------------------------------------------------------------------------------------------------------

def tamperings(c):
    """{name: proof bytes}: one change each"""
    sp = sm.proof_spans(c["comm"])
    out = {}
    for k in range(3):
        b = bytearray(c["data"]); b[sp["evals"][0] + 32 * k] ^= 1
        out["inst_evals[%d]" % k] = bytes(b)
    for half in ("sat", "eval"):
        b = bytearray(c["data"]); b[sp[half][1] - 32] ^= 1          # the last scalar of the half
        out["one byte in the %s half" % half] = bytes(b)
        b = bytearray(c["data"]); b[sp[half][0]] ^= 1               # its first point
        out["the first byte of the %s half" % half] = bytes(b)
    for k in range(3):
        b = bytearray(c["data"]); o = sp["evals"][0] + 32 * k
        b[o:o + 32] = (int.from_bytes(b[o:o + 32], "little") + R_MOD).to_bytes(32, "little") if k else R_MOD.to_bytes(32, "little")
        out["inst_evals[%d] >= r" % k] = bytes(b)
    return out


def other_circuit(ctx, c):
    """another instance of the same padded shape and N: its key fits the same bundle and the same proof length"""
    for seed in range(12, 60):
        mats, _, _ = _instance(c["key"], seed)
        if sm.num_ops(sm.Instance(*c["key"][:3], mats)) == c["comm"]["N"]:
            return case(ctx, c["key"], seed=seed)
    raise AssertionError("no second instance with N = %d" % c["comm"]["N"])


@pytest.mark.parametrize("key", TAMPER_CASES)
def test_verify_refuses_each_tampering_on_both_kinds_of_key(ctx, sbn, key):
    c = case(ctx, key)
    honest = (True, c["state"])
    vk = ctx.snark_key_from_comm(c["dkey"].comm())
    try:
        for dkey in (c["dkey"], vk):
            assert device_verify(ctx, sbn, c, dkey=dkey)[:2] == honest
        t = tamperings(c)
        assert len(t) == 3 + 4 + 3
        for name, data in t.items():
            assert model_verify(c, data=data)[0] is False, name
            for dkey in (c["dkey"], vk):
                ok, state, before = device_verify(ctx, sbn, c, data=data, dkey=dkey)
                assert ok is False and state == before, name
            assert device_verify(ctx, sbn, c, dkey=vk)[:2] == honest, name
        wrong = list(c["inputs"]); wrong[-1] = (wrong[-1] + 1) % R_MOD
        assert model_verify(c, inputs=wrong)[0] is False
        other = other_circuit(ctx, c)
        assert model_verify(c, comm=other["comm"])[0] is False
        for dkey, okey in ((c["dkey"], other["dkey"]), (vk, None)):
            ok, state, before = device_verify(ctx, sbn, c, inputs=wrong, dkey=dkey)
            assert ok is False and state == before
            if okey is not None:
                ok, state, before = device_verify(ctx, sbn, c, dkey=okey)      # the key of another circuit
                assert ok is False and state == before
        assert device_verify(ctx, sbn, c)[:2] == honest
    finally:
        vk.free()


def test_misuse_is_einval_and_launches_nothing(ctx, sbn):
    c = case(ctx, (5, 3, 2, None))
    other = case(ctx, (2, 40, 5, None))                             # another num_vars_padded: gens_pc has another size
    vk = ctx.snark_key_from_comm(c["dkey"].comm())
    t = vars_table(ctx, c)
    long = ctx.table_upload(_sbs(sm.pad_vars(c["vars"], 8)))
    L = sbn.lib()
    inp, rnd = _sbs(c["inputs"]), _sbs(c["rnd"])
    big = R_MOD.to_bytes(32, "little")
    tr = sbn.Transcript(TR)
    before = tr.state()
    ctx.prof_enable(True)
    try:
        ctx.prof_reset()
        for data in (c["data"][:-1], c["data"] + b"\0", c["data"][:32], other["data"]):       # a wrong proof_len
            with pytest.raises(sbn.SbnError, match="rc=-1"):
                ctx.snark_verify(c["dkey"], inp, c["dg"], data, tr)
        with pytest.raises(sbn.SbnError, match="rc=-1"):
            ctx.snark_verify(c["dkey"], inp[:32], c["dg"], c["data"], tr)                     # a wrong num_inputs
        with pytest.raises(sbn.SbnError, match="rc=-1"):
            ctx.snark_verify(c["dkey"], big + inp[32:], c["dg"], c["data"], tr)               # an input >= r
        with pytest.raises(sbn.SbnError, match="rc=-1"):
            ctx.snark_verify(c["dkey"], inp, other["dg"], c["data"], tr)                      # a bundle of another shape
        for k in (vk, ):                                                                      # the prover's calls on a verifier key
            with pytest.raises(sbn.SbnError, match="rc=-1"):
                ctx.snark_prove(k, t, inp, c["dg"], rnd, tr)
            with pytest.raises(sbn.SbnError, match="rc=-1"):
                ctx.snark_is_sat(k, t, inp)
        with pytest.raises(sbn.SbnError, match="rc=-1"):
            ctx.snark_prove(c["dkey"], long, inp, c["dg"], rnd, tr)                           # more variables than num_vars_padded
        with pytest.raises(sbn.SbnError, match="rc=-1"):
            ctx.snark_prove(c["dkey"], t, inp[:32], c["dg"], rnd, tr)
        with pytest.raises(sbn.SbnError, match="rc=-1"):
            ctx.snark_prove(c["dkey"], t, inp, c["dg"], big + rnd[32:], tr)                   # a draw of the sat half >= r
        with pytest.raises(sbn.SbnError, match="rc=-1"):
            ctx.snark_prove(c["dkey"], t, inp, c["dg"], rnd[:-32] + big, tr)                  # and of the eval half
        with pytest.raises(sbn.SbnError, match="rc=-1"):
            ctx.snark_prove(c["dkey"], t, inp, other["dg"], rnd, tr)
        proof = (C.c_uint8 * len(c["data"]))()
        p = lambda x: (C.c_uint8 * len(x)).from_buffer_copy(x)      # noqa: E731
        assert L.sbn_snark_prove(ctx.h, c["dkey"].h, t.h, p(inp), C.c_size_t(2), c["dg"].h, C.c_uint32(2), p(rnd), tr.h, proof) == -1      # an unknown flag
        assert L.sbn_snark_prove(ctx.h, c["dkey"].h, t.h, p(inp), C.c_size_t(2), c["dg"].h, C.c_uint32(0), None, tr.h, proof) == -1
        acc = C.c_int(7)
        assert L.sbn_snark_verify(ctx.h, c["dkey"].h, p(inp), C.c_size_t(2), c["dg"].h, p(c["data"]), C.c_size_t(len(c["data"])), None, C.byref(acc)) == -1
        assert ctx.prof_get() == {}, "a refused call launched something"
        assert tr.state() == before and bytes(proof) == bytes(len(c["data"])) and acc.value == 7
    finally:
        ctx.prof_enable(False)
        vk.free(); t.free(); long.free()
    assert device_verify(ctx, sbn, c)[:2] == (True, c["state"])


# ---- the witness check -------------------------------------------------------------------------------------------------------------

def _violate(mats, rows):
    """C with the entry of each listed row raised by one: exactly those rows are violated (C holds one entry a row, at index row)"""
    A, B, (cr, cc, cv) = mats
    cv = list(cv)
    for r in rows:
        assert cr[r] == r
        cv[r] = (cv[r] + 1) % R_MOD
    return A, B, (cr, cc, cv)


@pytest.mark.parametrize("nc", [2, 1 << 12])
def test_is_sat_counts_the_violated_rows_and_names_the_first(ctx, nc):
    nv, ni = 4, 1                                                   # raw = padded: the columns stay where they are
    mats, vars_, inputs = sm.satisfying_instance(nc, nv, ni, seed=nc)
    t = ctx.table_upload(_sbs(vars_))
    last = nc - 1
    trials = [[], [0], [last]] + ([[255], [256], [255, 256], [3000, 17, 2048, last], list(range(0, nc, 7))] if nc > 2 else [[0, 1]])
    try:
        for rows in trials:
            bad = _violate(mats, rows)
            inst = sm.Instance(nc, nv, ni, bad)
            want = sm.is_sat(inst, vars_, inputs)
            assert want == ((True, 0, None) if not rows else (False, len(rows), min(rows)))
            m = ctx.r1cs_upload(nc, nv, _mats_bytes(bad))
            try:
                sat, nb, fb = ctx.r1cs_is_sat(m, t, _sbs(inputs))
                assert (sat, nb) == want[:2] and (sat or fb == want[2]), rows
            finally:
                m.free()
    finally:
        t.free()


def test_is_sat_where_the_loop_strides_over_the_grid(ctx):
    """2^20 rows: more rows than the grid has lanes, so every lane takes two; almost all rows are empty (0 * 0 = 0 holds)"""
    nc, nv = 1 << 20, 4
    vars_ = [3, 5, 7, 11]
    live = [0, 255, 256, 1 << 19, (1 << 19) + 1, nc - 1]
    A = (live, [0] * len(live), [2] * len(live))                    # Az = 6
    B = (live, [1] * len(live), [1] * len(live))                    # Bz = 5
    t = ctx.table_upload(_sbs(vars_))
    try:
        for rows in ([], [nc - 1], [(1 << 19) + 1, nc - 1], [1 << 19]):
            Cm = (live, [nv] * len(live), [31 if r in rows else 30 for r in live])
            m = ctx.r1cs_upload(nc, nv, _mats_bytes([A, B, Cm]))
            try:
                sat, nb, fb = ctx.r1cs_is_sat(m, t, b"")
                assert (sat, nb) == (not rows, len(rows)) and (sat or fb == min(rows)), rows
            finally:
                m.free()
    finally:
        t.free()


def test_is_sat_reads_any_representative_a_producer_left(ctx):
    """the witness is what sbn_bind_top leaves of a table of twice the length (lazy representatives); the instance is built around its downloaded values"""
    nc, nv, ni = 64, 8, 2
    rng = random.Random(5)
    t = ctx.table_upload(_sbs([rng.choice([0, 1, R_MOD - 1, rng.randrange(R_MOD)]) for _ in range(2 * nv)]))
    try:
        ctx.bind_top(t, pm.sb(rng.randrange(R_MOD)))
        assert len(t) == nv
        vars_ = rm.from_bytes(ctx.table_download(t))
        mats, _, inputs = sm.satisfying_instance(nc, nv, ni, seed=9, vars_=vars_)
        for rows in ([], [63], [5, 9]):
            m = ctx.r1cs_upload(nc, nv, _mats_bytes(_violate(mats, rows)))
            try:
                sat, nb, fb = ctx.r1cs_is_sat(m, t, _sbs(inputs))
                assert (sat, nb) == (not rows, len(rows)) and (sat or fb == min(rows)), rows
            finally:
                m.free()
    finally:
        t.free()


def test_is_sat_with_every_value_at_r_minus_one(ctx):
    nc, nv, ni = 8, 4, 3
    mats, vars_, inputs = sm.satisfying_instance(nc, nv, ni, seed=2, only_vals=[R_MOD - 1])
    assert set(vars_ + inputs) == {R_MOD - 1}
    t = ctx.table_upload(_sbs(vars_))
    try:
        for rows in ([], [7]):
            m = ctx.r1cs_upload(nc, nv, _mats_bytes(_violate(mats, rows)))
            try:
                assert ctx.r1cs_is_sat(m, t, _sbs(inputs))[:2] == (not rows, len(rows))
            finally:
                m.free()
    finally:
        t.free()


@pytest.mark.parametrize("key", [(5, 3, 2, None), (2, 1, 3, None), (1, 2, 0, None)])
def test_snark_is_sat_on_raw_shapes_and_short_tables(ctx, sbn, key):
    c = case(ctx, key)
    nc = key[0]
    bad = ctx.snark_encode(*key[:3], _mats_bytes(_violate(c["mats"], [nc - 1])), c["dg"])
    tabs = [vars_table(ctx, c), vars_table(ctx, c, c["inst"].nv)]
    try:
        for t in tabs:
            assert ctx.snark_is_sat(c["dkey"], t, _sbs(c["inputs"])) == (True, 0, 0)
            sat, nb, fb = ctx.snark_is_sat(bad, t, _sbs(c["inputs"]))
            assert (sat, nb, fb) == (False, 1, nc - 1)
        with pytest.raises(sbn.SbnError, match="rc=-1"):
            ctx.snark_is_sat(c["dkey"], tabs[0], _sbs(c["inputs"]) + pm.sb(1))      # one input too many
    finally:
        bad.free()
        for t in tabs:
            t.free()


def test_check_sat_stops_a_bad_witness_before_any_proving_launch(ctx, sbn):
    c = case(ctx, (5, 3, 2, None))
    wrong = dict(c, vars=[(c["vars"][0] + 1) % R_MOD] + c["vars"][1:])
    want = sm.is_sat(c["inst"], wrong["vars"], c["inputs"])
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
        rc = L.sbn_snark_prove(ctx.h, c["dkey"].h, t.h, p(_sbs(c["inputs"])), C.c_size_t(len(c["inputs"])), c["dg"].h, C.c_uint32(sbn.SBN_SNARK_CHECK_SAT), p(_sbs(c["rnd"])), tr.h, proof)
        prof = {k: v[1] for k, v in ctx.prof_get().items()}
    finally:
        ctx.prof_enable(False)
    try:
        assert rc == sbn.SBN_EUNSAT == -5
        assert tr.state() == before and bytes(proof) == b"\xaa" * len(c["data"])
        assert prof["k_r1cs_sat_check"] == 1 and set(prof) <= {"k_r1cs_build_z", "k_r1cs_spmv", "k_r1cs_fix", "k_r1cs_sat_check"}, prof
        with pytest.raises(sbn.SbnUnsat, match="%d constraints, the first is row %d" % want[1:]):
            ctx.snark_prove(c["dkey"], t, _sbs(c["inputs"]), c["dg"], _sbs(c["rnd"]), tr, check_sat=True)
        # without the flag the library proves what it is given, and the verifier refuses the proof
        data = ctx.snark_prove(c["dkey"], t, _sbs(c["inputs"]), c["dg"], _sbs(c["rnd"]), sbn.Transcript(TR))
        ok, state, was = device_verify(ctx, sbn, c, data=data)
        assert ok is False and state == was
    finally:
        t.free()
    assert device_prove(ctx, sbn, c, check_sat=True) == (c["data"], c["state"])


def test_launch_counts(ctx, sbn):
    c = case(ctx, (5, 3, 2, None))
    device_prove(ctx, sbn, c)                                       # (the derived sets are built by now)
    t = vars_table(ctx, c)
    counts = []
    ctx.prof_enable(True)
    try:
        for run in (lambda: ctx.snark_is_sat(c["dkey"], t, _sbs(c["inputs"])), lambda: device_prove(ctx, sbn, c), lambda: device_prove(ctx, sbn, c, check_sat=True),
                    lambda: device_verify(ctx, sbn, c)):
            ctx.prof_reset()
            run()
            counts.append({k: v[1] for k, v in ctx.prof_get().items()})
    finally:
        ctx.prof_enable(False)
        t.free()
    sat, plain, checked, verify = counts
    assert sat["k_r1cs_sat_check"] == 1 and sat["k_r1cs_build_z"] == 1 and sat["k_r1cs_spmv"] == 1
    assert "k_r1cs_sat_check" not in plain and "k_r1cs_sat_check" not in verify
    assert checked["k_r1cs_sat_check"] == 1 and checked["k_r1cs_build_z"] == plain["k_r1cs_build_z"] + 1
    assert {k: v for k, v in checked.items() if k not in sat} == {k: v for k, v in plain.items() if k not in sat}      # the flag adds the check's launches and nothing else
    assert plain["k_r1cs_spmv_eval"] == 1                           # A, B, C(rx, ry) between the halves
    assert verify["k_g1_decompress"] >= 2 and verify["k_pow2_table"] == 1
