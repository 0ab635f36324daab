"""GPU: sbn_circom_* — circom's .r1cs and .wtns files parsed on the device — against the literal model of tests/circom_model.py (the triplets, the counts, the
refusals) and against the routes that existed before (sbn_r1cs_upload, sbn_snark_encode, sbn_nizk_instance_new on the model's triplets): the handles must be
indistinguishable through every call that reads them.  Device against device wherever a proof is involved: no model proof is computed here."""
import collections
import ctypes as C
import random

import pytest

import circom_model as cm
import nizk_model as nm
import snark_model as sm
from conftest import golden

pytestmark = pytest.mark.gpu
R = cm.R_MOD
TR = b"circom gpu"
DIGEST = bytes(range(7, 71))
H = bytes.fromhex


def _sb(v):
    return int(v).to_bytes(32, "little")


def _sbs(xs):
    return b"".join(_sb(x) for x in xs)


def model_of(data):
    """-> (the model's R1CS, (nc, nv, ni, nc_padded, nv_padded), the three padded triplet lists)"""
    r = cm.read_r1cs(data)
    shp = cm.shape(r)
    return r, shp, cm.to_sparse_matrices_padded(r, shp[4])


def upload_mats(mats):
    """[(row, col, val)] x 3 -> what r1cs_upload takes"""
    return [(rows, cols, _sbs(vals)) for rows, cols, vals in cm.triplet_lists(mats)]


def raw_mats(mats, shp):
    """the padded triplets in the raw numbering snark_encode / nizk_instance_new take (vars | 1 | inputs)"""
    _, nv, _, _, nvp = shp
    return [(rows, [c - nvp + nv if c >= nvp else c for c in cols], _sbs(vals)) for rows, cols, vals in cm.triplet_lists(mats)]


def assert_download_is_the_models(ctx, data):
    r, shp, mats = model_of(data)
    f = ctx.circom_r1cs_load(data)
    try:
        info = f.info()
        want = dict(num_constraints=r["num_constraints"], num_variables=r["num_variables"], num_pub_inputs=r["num_pub_inputs"], num_prv_inputs=r["num_prv_inputs"],
                    num_labels=r["num_labels"], nnz=tuple(len(r[k]) for k in "abc"), dropped=tuple(r["dropped"]), num_vars=shp[1], num_cons_padded=shp[3], num_vars_padded=shp[4])
        assert info == want
        for m in range(3):
            rows, cols, vals = f.download(m)
            assert list(zip(rows, cols, vals)) == [(a, b, _sb(v)) for a, b, v in mats[m]], m
    finally:
        f.free()
    return r, shp, mats


# ---- 1. download ----------------------------------------------------------------------------------------------------------------------

def _shape(n_wires, n_pub, labels=None):
    return dict(n_wires=n_wires, n_pub_out=n_pub // 2, n_pub_in=n_pub - n_pub // 2, n_prv_in=1, n_labels=labels or 3 * n_wires)


def _download_files():
    rng = random.Random(5)
    v = lambda: rng.choice([1, R - 1, rng.randrange(R)])            # noqa: E731
    yield "golden", H(golden("circom_kat.json")["r1cs"])
    yield "no_public_columns", cm.write_r1cs(_shape(5, 0), [([(0, v()), (1, v())], [(4, v())], [(2, v())]), ([(3, v())], [(0, v())], [(1, v()), (4, v())])])
    # num_vars = 1 < n_pub + 1 = 5: num_vars_padded = 8 comes from the inputs
    yield "padding_from_the_inputs", cm.write_r1cs(_shape(6, 4), [([(5, v()), (4, v())], [(0, v())], [(1, v())]), ([(2, v())], [(3, v()), (5, v())], [(0, v())])])
    # wires exactly 0, n_pub, n_pub + 1, nWires - 1
    yield "remap_boundaries", cm.write_r1cs(_shape(9, 3), [([(0, v()), (3, v()), (4, v()), (8, v())], [(8, v()), (4, v())], [(3, v()), (0, v())])] * 2, section_order=(9, 2, 1),
                                            extra_sections={9: b"\x05"})
    yield "a_run_of_300_entries", cm.write_r1cs(_shape(40, 2), [([(1, v())], [(2, v())], []), ([(j % 40, v()) for j in range(300)], [(5, v())], [(6, v())]), ([], [(7, v())], [(0, v())])])
    yield "2200_entries_in_one_matrix", cm.write_r1cs(_shape(50, 5), [([(3, v())], [((7 * i + j) % 50, v()) for j in range(220)], [(i % 50, v())]) for i in range(10)])
    yield "all_empty", cm.write_r1cs(_shape(6, 1), [([], [], [])] * 5)
    yield "no_constraints", cm.write_r1cs(_shape(6, 1), [])
    yield "empty_first_and_last_runs", cm.write_r1cs(_shape(8, 2), [([], [(1, v())], [(2, v())]), ([], [], []), ([(3, v()), (4, v())], [], []), ([(5, v())], [(6, v())], [])])


DOWNLOAD = dict(_download_files())


@pytest.mark.parametrize("name", list(DOWNLOAD))
def test_download_and_info_are_the_models(ctx, name):
    r, shp, mats = assert_download_is_the_models(ctx, DOWNLOAD[name])
    if name == "golden":
        g = golden("circom_kat.json")
        assert [[(a, b, str(v)) for a, b, v in m] for m in mats] == [[tuple(t) for t in g["padded"][k]] for k in "ABC"]
    if name == "a_run_of_300_entries":
        assert max(r["counts"]) == 300
    if name == "2200_entries_in_one_matrix":
        assert len(r["b"]) == 2200


# ---- 2. dropped values ----------------------------------------------------------------------------------------------------------------

def _with_values(cons, where):
    """constraints with the value of each listed (constraint, matrix, entry) replaced by one >= r"""
    big = [R, R + 1, 2**256 - 1, R + (1 << 200)]
    out = [tuple(list(run) for run in abc) for abc in cons]
    for n, (i, m, e) in enumerate(where):
        out[i][m][e] = (out[i][m][e][0], big[n % len(big)])
    return out


def _drop_files():
    rng = random.Random(6)
    cons = [([(rng.randrange(12), rng.randrange(R)) for _ in range(3)], [(rng.randrange(12), rng.randrange(R)) for _ in range(2)], [(rng.randrange(12), rng.randrange(R))]) for _ in range(6)]
    shape = _shape(12, 3)
    yield "first_entry", cm.write_r1cs(shape, _with_values(cons, [(0, 0, 0)]))
    yield "last_entry", cm.write_r1cs(shape, _with_values(cons, [(5, 2, 0)]))
    yield "a_middle_entry", cm.write_r1cs(shape, _with_values(cons, [(2, 0, 1), (3, 1, 0)]))
    yield "every_entry_of_B", cm.write_r1cs(shape, _with_values(cons, [(i, 1, e) for i in range(6) for e in range(2)]))
    yield "first_last_and_all_of_C", cm.write_r1cs(shape, _with_values(cons, [(0, 0, 0), (5, 1, 1)] + [(i, 2, 0) for i in range(6)]))
    many = [([(j % 30, rng.randrange(R)) for j in range(500)], [(1, 1)], [(2, 1)]) for _ in range(6)]      # the scan over more than one chunk of 2048
    yield "across_scan_chunks", cm.write_r1cs(_shape(30, 2), _with_values(many, [(i, 0, e) for i in range(6) for e in (0, 255, 256, 499)]))


DROPS = dict(_drop_files())


@pytest.mark.parametrize("name", list(DROPS))
def test_values_not_below_r_are_dropped_in_order(ctx, name):
    r, shp, mats = assert_download_is_the_models(ctx, DROPS[name])
    assert sum(r["dropped"]) > 0 and max(len(m) for m in mats) >= 2      # encode needs N >= 2
    if name == "every_entry_of_B":
        assert r["dropped"] == [0, 12, 0] and mats[1] == []


# ---- 3. a wire that does not exist ----------------------------------------------------------------------------------------------------

def test_a_wire_past_nwires_is_refused_and_names_the_entry(ctx, sbn):
    cons = [([(1, 2), (2, 3)], [(3, 4)], [(4, 5)]), ([(5, 6)], [(1, 7), (6, 8)], [(0, 9)]), ([(2, 1)], [(3, 1)], [(9, 1)])]
    shape = _shape(6, 2)
    r = cm.read_r1cs(cm.write_r1cs(shape, cons))
    assert cm.first_bad_wire(r) == 6                                  # entry 6 in file order: matrix B of constraint 1, its second entry
    with pytest.raises(sbn.SbnError, match=r"rc=-1.*entry 6 of the file \(matrix B, constraint 1, entry 1 of its run\)"):
        ctx.circom_r1cs_load(cm.write_r1cs(shape, cons))
    # the same wire under a value >= r is dropped before anyone looks at it; the next bad one is named
    cons[1][1][1] = (6, R)
    data = cm.write_r1cs(shape, cons)
    assert cm.first_bad_wire(cm.read_r1cs(data)) == 10
    with pytest.raises(sbn.SbnError, match=r"rc=-1.*entry 10 of the file \(matrix C, constraint 2, entry 0"):
        ctx.circom_r1cs_load(data)
    out = C.c_void_p(7)
    buf = (C.c_uint8 * len(data)).from_buffer_copy(data)
    assert sbn.lib().sbn_circom_r1cs_load(ctx.h, buf, C.c_size_t(len(data)), C.byref(out)) == -1 and out.value is None
    for why, f in (("magic", b"r1cx" + data[4:]), ("prime", data.replace(_sb(R), _sb(R + 2))), ("end of the file", cm.write_r1cs(shape, cons, section_order=(1, 2))[:-1]), ("end of section 2", cm.write_r1cs(shape, cons, num_constraints=4))):
        with pytest.raises(sbn.SbnError, match="rc=-1.*refused.*" + why):
            ctx.circom_r1cs_load(f)


# ---- 4. the matrices handle -----------------------------------------------------------------------------------------------------------

def _big_circuit(num_vars, ni, num_cons, seed):
    """wire 0 in every run (a column-major row of more than 2048 entries), duplicates of one (row, column), wires over the whole range"""
    rng = random.Random(seed)
    nw = 1 + ni + num_vars
    cons = []
    for i in range(num_cons):
        w = rng.randrange(nw)
        cons.append(([(0, rng.randrange(R)), (w, 1), (w, R - 1), (rng.randrange(nw), rng.randrange(R))], [(0, 1), (rng.randrange(1, ni + 1), rng.randrange(R))],
                     [(0, rng.randrange(R)), (nw - 1 - (i % 3), 5)]))
    return cm.write_r1cs(_shape(nw, ni), cons)


def _handle_files():
    for key in nm.SNARK_KEYS:
        nc, nv, ni, _ = key
        mats, vars_, inputs = nm.instance(key)
        yield "raw_%d_%d_%d" % key[:3], cm.raw_to_circom(nc, nv, ni, mats, vars_, inputs)[0]
    yield "nv_64_one_pass", _big_circuit(60, 3, 1100, 1)
    yield "nv_512_two_passes", _big_circuit(500, 7, 1100, 2)
    yield "nv_65536_three_passes", _big_circuit(40000, 2, 1100, 3)
    yield "dropped_entries", DROPS["first_last_and_all_of_C"]
    yield "all_empty", DOWNLOAD["all_empty"]


HANDLES = dict(_handle_files())


@pytest.mark.parametrize("name", list(HANDLES))
def test_from_circom_is_indistinguishable_from_upload(ctx, name):
    data = HANDLES[name]
    r, (nc, nv, ni, ncp, nvp), mats = model_of(data)
    if name.startswith("nv_"):
        assert nvp == int(name.split("_")[1]) and sum(1 for t in mats[0] + mats[1] + mats[2] if t[1] == nvp) > 2048
    f = ctx.circom_r1cs_load(data)
    a = ctx.r1cs_from_circom(f)
    f.free()                                                          # the handle keeps nothing of the parsed circuit
    b = ctx.r1cs_upload(ncp, nvp, upload_mats(mats))
    rng = random.Random(8)
    nx, ny = ncp.bit_length() - 1, nvp.bit_length()
    z = ctx.table_upload(_sbs(rng.randrange(R) for _ in range(2 * nvp)))
    rx, ry = _sbs(rng.randrange(R) for _ in range(nx)), _sbs(rng.randrange(R) for _ in range(ny))
    rabc = [_sb(rng.randrange(R)) for _ in range(3)]
    try:
        assert (a.num_cons, a.num_vars) == (ncp, nvp)
        got = []
        for h in (a, b):
            tabs = ctx.r1cs_multiply(h, z)
            et = ctx.r1cs_eval_table(h, rx, *rabc)
            got.append(([ctx.table_download(t) for t in tabs], ctx.table_download(et), ctx.r1cs_evaluate(h, rx, ry)))
            for t in tabs + (et,):
                t.free()
        assert got[0] == got[1]
        if sum(len(m) for m in mats):
            assert any(x != bytes(len(x)) for x in got[0][0])         # (not an equality of two zero results)
    finally:
        z.free(); a.free(); b.free()


# ---- 5. SNARK::encode ------------------------------------------------------------------------------------------------------------------

def _satisfied_with_drops(key, seed):
    """a satisfied raw circuit as a file with entries of value >= r among its own: the reader drops them, the circuit is the one it was"""
    nc, nv, ni, _ = key
    mats, vars_, inputs = nm.instance(key, seed)
    r1cs, wtns = cm.raw_to_circom(nc, nv, ni, mats, vars_, inputs)
    r = cm.read_r1cs(r1cs)
    cons = [([], [], []) for _ in range(nc)]
    for m, row, wire, val in r["file_order"]:
        cons[row][m].append((wire, val))
    cons[0][0].insert(0, (1, R)); cons[nc - 1][2].append((2, 2**256 - 1)); cons[nc // 2][1].insert(1, (0, R + 7))
    shape = dict(n_wires=1 + ni + nv, n_pub_out=0, n_pub_in=ni, n_prv_in=0, n_labels=9)
    return cm.write_r1cs(shape, cons), wtns


def _rnd(n, seed):
    rng = random.Random(seed)
    return _sbs(rng.randrange(R) for _ in range(n))


@pytest.mark.parametrize("drops", [False, True])
def test_encode_gives_the_key_of_the_raw_route(ctx, sbn, drops):
    key = (5, 3, 2, None) if not drops else (6, 5, 1, None)
    if drops:
        r1cs, wtns = _satisfied_with_drops(key, 12)
    else:
        mats0, vars0, inputs0 = nm.instance(key)
        r1cs, wtns = cm.raw_to_circom(*key[:3], mats0, vars0, inputs0)
    r, shp, mats = model_of(r1cs)
    nc, nv, ni, ncp, nvp = shp
    assert (sum(r["dropped"]) > 0) == drops
    f = ctx.circom_r1cs_load(r1cs)
    nnz = max(f.info()["nnz"])
    dg = ctx.snark_gens_new(nc, nv, ni, nnz)
    ka = ctx.snark_encode_circom(f, dg)
    f.free()
    kb = ctx.snark_encode(nc, nv, ni, raw_mats(mats, shp), dg)
    vt, inp, count = ctx.circom_wtns_load(wtns, ni)
    try:
        assert ka.comm() == kb.comm() and ka.sizes() == kb.sizes() and count == 1 + ni + nv
        assert ctx.snark_is_sat(ka, vt, inp) == ctx.snark_is_sat(kb, vt, inp) == (True, 0, 0)
        rnd = _rnd(ka.sizes()[0], 3)
        proofs = []
        for k in (ka, kb):
            tr = sbn.Transcript(TR)
            proofs.append((ctx.snark_prove(k, vt, inp, dg, rnd, tr), tr.state()))
        assert proofs[0] == proofs[1]
        for k in (ka, kb):                                            # a proof from one key verifies on the other
            tr = sbn.Transcript(TR)
            assert ctx.snark_verify(k, inp, dg, proofs[0][0], tr) is True and tr.state() == proofs[0][1]
        bad = bytearray(proofs[0][0]); bad[40] ^= 1
        assert ctx.snark_verify(ka, inp, dg, bytes(bad), sbn.Transcript(TR)) is False
    finally:
        vt.free(); ka.free(); kb.free(); dg.free()


# ---- 6. NIZK ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("key", [(5, 3, 2, None), (2, 40, 5, None), nm.ALL_EMPTY])
def test_nizk_instance_gives_the_proof_of_the_raw_route(ctx, sbn, key):
    nc, nv, ni, _ = key
    mats0, vars0, inputs0 = nm.instance(key)
    r1cs, wtns = cm.raw_to_circom(nc, nv, ni, mats0, vars0, inputs0)
    r, shp, mats = model_of(r1cs)
    f = ctx.circom_r1cs_load(r1cs)
    ia = ctx.nizk_instance_from_circom(f, DIGEST)
    f.free()                                                          # before proving: harmless
    ib = ctx.nizk_instance_new(nc, nv, ni, raw_mats(mats, shp), DIGEST)
    dg = ctx.nizk_gens_new(nc, nv, ni)
    vt, inp, _ = ctx.circom_wtns_load(wtns, ni)
    try:
        assert ia.sizes() == ib.sizes() and (ia.r1cs.num_cons, ia.r1cs.num_vars) == (shp[3], shp[4])
        assert ctx.nizk_is_sat(ia, vt, inp) == ctx.nizk_is_sat(ib, vt, inp) == (True, 0, 0)
        rnd = _rnd(ia.sizes()[0], 4)
        proofs = []
        for k in (ia, ib):
            tr = sbn.Transcript(TR)
            proofs.append((ctx.nizk_prove(k, vt, inp, dg, rnd, tr, check_sat=True), tr.state()))
        assert proofs[0] == proofs[1]
        for k in (ia, ib):
            tr = sbn.Transcript(TR)
            assert ctx.nizk_verify(k, inp, dg, proofs[0][0], tr) is True and tr.state() == proofs[0][1]
        bad = bytearray(proofs[0][0]); bad[-1] ^= 1
        assert ctx.nizk_verify(ia, inp, dg, bytes(bad), sbn.Transcript(TR)) is False
    finally:
        vt.free(); ia.free(); ib.free(); dg.free()


# ---- 7. the witness --------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("key", [(5, 3, 2, None), (2, 1, 3, None), (40, 4, 2, None), (1, 2, 0, None)])
def test_witness_is_the_models_and_satisfies_the_circuit(ctx, sbn, key):
    nc, nv, ni, _ = key
    mats0, vars0, inputs0 = nm.instance(key)
    r1cs, wtns = cm.raw_to_circom(nc, nv, ni, mats0, vars0, inputs0)
    values, _ = cm.read_wtns(wtns)
    want_in, want_tab = cm.split_witness(values, ni)
    f = ctx.circom_r1cs_load(r1cs)
    inst = ctx.nizk_instance_from_circom(f, DIGEST)
    f.free()
    vt, inp, count = ctx.circom_wtns_load(wtns, ni)
    # one variable changed: the last one the circuit reads (a random circuit this small may leave a variable unused), found on the model
    model = sm.Instance(nc, nv, ni, mats0)
    j = next(j for j in reversed(range(nv)) if not sm.is_sat(model, vars0[:j] + [(vars0[j] + 1) % R] + vars0[j + 1:], inputs0)[0])
    changed = list(values); changed[1 + ni + j] = (changed[1 + ni + j] + 1) % R
    vt2, inp2, _ = ctx.circom_wtns_load(cm.write_wtns(changed, sections=[(9, b"abc"), (2, _sbs(changed))]), ni)      # the values unaligned in the file
    try:
        assert (inp, ctx.table_download(vt), count, len(vt)) == (_sbs(want_in), _sbs(want_tab), len(values), len(want_tab))
        assert want_in == inputs0 and want_tab[:nv] == vars0
        assert ctx.nizk_is_sat(inst, vt, inp) == (True, 0, 0)
        assert ctx.nizk_is_sat(inst, vt2, inp2)[0] is False
    finally:
        vt.free(); vt2.free(); inst.free()


def test_witness_refusals_give_no_table(ctx, sbn):
    values = [1, 5, 6, 7, 8, 9]
    body = _sbs(values)
    cases = [("value 4 is >= r", cm.write_wtns(values[:4] + [R, R + 1]), 2), ("value 0 is >= r", cm.write_wtns([R] + values[1:]), 2), ("value 2 is >= r", cm.write_wtns([1, 2, 2**256 - 1, 4]), 2),
             ("3 values.*need 4", cm.write_wtns(values[:3]), 3), ("second witness section", cm.write_wtns(values, sections=[(2, body), (2, body)]), 2),
             ("end of the file", cm.write_wtns(values)[:-1], 2), ("no multiple of 32", cm.write_wtns(values, sections=[(2, body + b"\0")]), 2), ("magic", b"wtnz" + cm.write_wtns(values)[4:], 2)]
    for why, data, ni in cases:
        with pytest.raises(sbn.SbnError, match="rc=-1.*" + why):
            ctx.circom_wtns_load(data, ni)
        t, n = C.c_void_p(7), C.c_size_t(7)
        inp = (C.c_uint8 * 96)(*([0xaa] * 96))
        buf = (C.c_uint8 * len(data)).from_buffer_copy(data)
        assert sbn.lib().sbn_circom_wtns_load(ctx.h, buf, C.c_size_t(len(data)), C.c_size_t(ni), C.byref(t), inp, C.byref(n)) == -1
        assert t.value is None and n.value == 7 and bytes(inp) == b"\xaa" * 96, why
    vt, inp, n = ctx.circom_wtns_load(cm.write_wtns(values[:3] + [R - 1]), 3)      # exactly 1 + num_inputs values: no variable, a table of num_inputs + 1 zeros
    assert (inp, n, ctx.table_download(vt)) == (_sbs([5, 6, R - 1]), 4, bytes(32 * 4))
    vt.free()


# ---- 8. misuse -------------------------------------------------------------------------------------------------------------------------

def test_misuse_is_einval_and_launches_nothing(ctx, sbn):
    L = sbn.lib()
    data = H(golden("circom_kat.json")["r1cs"])
    wt = H(golden("circom_kat.json")["wtns"])
    f = ctx.circom_r1cs_load(data)
    other = ctx.snark_gens_new(3, 40, 2, 5)                           # another num_vars_padded
    small = ctx.snark_gens_new(3, 3, 2, 2)                            # the shape, but N = 2 where the file's largest matrix holds 5 entries
    nz = ctx.nizk_gens_new(3, 3, 2)                                   # no eval sets
    buf = (C.c_uint8 * len(data)).from_buffer_copy(data)
    wbuf = (C.c_uint8 * len(wt)).from_buffer_copy(wt)
    out, n = C.c_void_p(7), C.c_size_t(7)
    rows, cols, vals = (C.c_uint32 * 8)(), (C.c_uint32 * 8)(), (C.c_uint8 * 256)()
    inp = (C.c_uint8 * 64)()
    ctx.prof_enable(True)
    try:
        ctx.prof_reset()
        for gens in (other, small, nz):
            with pytest.raises(sbn.SbnError, match="rc=-1"):
                ctx.snark_encode_circom(f, gens)
        for m in (-1, 3, 1 << 20):
            assert L.sbn_circom_r1cs_download(ctx.h, f.h, m, rows, cols, vals) == -1
        assert L.sbn_circom_r1cs_download(ctx.h, f.h, 0, None, cols, vals) == -1 and L.sbn_circom_r1cs_download(None, f.h, 0, rows, cols, vals) == -1
        assert L.sbn_circom_r1cs_download(ctx.h, None, 0, rows, cols, vals) == -1
        load = [ctx.h, buf, C.c_size_t(len(data)), C.byref(out)]
        for k in (0, 1, 3):
            a = list(load); a[k] = None
            assert L.sbn_circom_r1cs_load(*a) == -1, k
        assert L.sbn_circom_r1cs_info(None, C.byref(out)) == -1 and L.sbn_circom_r1cs_info(f.h, None) == -1
        for fn, args, nulls in ((L.sbn_r1cs_from_circom, [ctx.h, f.h, C.byref(out)], (0, 1, 2)), (L.sbn_snark_encode_circom, [ctx.h, f.h, small.h, C.byref(out)], (0, 1, 2, 3)),
                                (L.sbn_nizk_instance_from_circom, [ctx.h, f.h, None, C.c_size_t(0), C.byref(out)], (0, 1, 4)),
                                (L.sbn_nizk_instance_from_circom, [ctx.h, f.h, None, C.c_size_t(5), C.byref(out)], ()),      # a NULL digest with a length
                                (L.sbn_circom_wtns_load, [ctx.h, wbuf, C.c_size_t(len(wt)), C.c_size_t(2), C.byref(out), inp, C.byref(n)], (0, 1, 4, 5, 6))):
            if not nulls:
                assert fn(*args) == -1
            for k in nulls:
                a = list(args); a[k] = None
                assert fn(*a) == -1, (fn.__name__, k)
        L.sbn_circom_r1cs_free(ctx.h, None)
        assert ctx.prof_get() == {}, "a refused call launched something"
        assert n.value == 7
    finally:
        ctx.prof_enable(False)
        f.free(); other.free(); small.free(); nz.free()


# ---- 9. launch counts ------------------------------------------------------------------------------------------------------------------

def _counts(ctx, run):
    ctx.prof_reset()
    out = run()
    return out, collections.Counter({k: v[1] for k, v in ctx.prof_get().items()})


def test_launch_counts(ctx, sbn):
    key = (5, 3, 2, None)
    mats0, vars0, inputs0 = nm.instance(key)
    r1cs, wtns = cm.raw_to_circom(*key[:3], mats0, vars0, inputs0)
    r, shp, mats = model_of(r1cs)
    nc, nv, ni, ncp, nvp = shp
    dg = ctx.snark_gens_new(nc, nv, ni, max(len(m) for m in mats))
    warm = ctx.snark_encode(nc, nv, ni, raw_mats(mats, shp), dg)      # (the derived generator sets are built by now)
    warm.free()
    held = []
    ctx.prof_enable(True)
    try:
        f, load = _counts(ctx, lambda: ctx.circom_r1cs_load(r1cs))
        fd, load_drops = _counts(ctx, lambda: ctx.circom_r1cs_load(DROPS["a_middle_entry"]))
        f512, _ = _counts(ctx, lambda: ctx.circom_r1cs_load(HANDLES["nv_512_two_passes"]))
        held += [f, fd, f512]
        h, from_circom = _counts(ctx, lambda: ctx.r1cs_from_circom(f))
        h512, from_512 = _counts(ctx, lambda: ctx.r1cs_from_circom(f512))
        up, upload = _counts(ctx, lambda: ctx.r1cs_upload(ncp, nvp, upload_mats(mats)))
        ka, enc_circom = _counts(ctx, lambda: ctx.snark_encode_circom(f, dg))
        kb, enc_raw = _counts(ctx, lambda: ctx.snark_encode(nc, nv, ni, raw_mats(mats, shp), dg))
        ia, nizk = _counts(ctx, lambda: ctx.nizk_instance_from_circom(f, DIGEST))
        vt, wt = _counts(ctx, lambda: ctx.circom_wtns_load(wtns, ni)[0])
        held += [h, h512, up, ka, kb, ia, vt]
    finally:
        ctx.prof_enable(False)
        for x in held:
            x.free()
        dg.free()
    tail = collections.Counter(k_fr_to_mont=2, k_r1cs_partition=2)    # the end both routes share, once per compressed copy
    assert load == collections.Counter(k_circom_entries=1)
    assert load_drops == load + collections.Counter(k_dense_scan=1, k_dense_scan_top=1, k_circom_compact=1)
    assert upload == tail

    def staged(passes):                                              # the sort passes are the column-major copy's alone: the row-major copy shows none
        return tail + collections.Counter(k_circom_gkeys=1, k_circom_ends=2, k_circom_gather=1, k_dense_hist=passes, k_dense_scan=passes, k_dense_scan_top=passes, k_dense_scatter=passes)
    assert nvp == 4 and from_circom == staged(1) == nizk              # 2 num_vars_padded = 8 columns: 3 bits, one pass
    assert from_512 == staged(2)                                      # 1024 columns: 10 bits, two passes of 5
    assert enc_circom - from_circom == enc_raw - upload and enc_circom == from_circom + (enc_raw - upload)      # encode: the same kernels behind the matrices
    assert enc_raw["k_dense_tables"] == 1 and enc_circom["k_dense_expand"] == 1
    assert wt == collections.Counter(k_circom_wtns=1)
