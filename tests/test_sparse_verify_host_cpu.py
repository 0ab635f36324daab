"""CPU: the field and transcript half of the sparse evaluation check (csrc/sparse_verify_host.hpp) against the literal verifier of
tests/sparse_eval_model.py.  tests/sparse_verify_host_check.cpp includes the header alone and is built with g++ under ASan + UBSan as a
stand-alone program, exactly as tests/test_proof_host_cpu.py builds proof_host_check.cpp; it is fed the model's proofs as hex lines.  Over all
of sem.SHAPES the product-layer check's claims, rand_ops, rand_mem and the 203-byte transcript state behind it, the hash layer's field verdict
and the three padded evaluation vectors equal the model's; every refusal is asserted on the model's side as well."""
import copy
import os
import subprocess

import pytest

import dense_model as dm
import sparse_eval_model as sem
import sparse_eval_verify_model as sevm
from conftest import ROOT
from sparse_eval_model import R, Transcript

LABEL = b"gens_sparse_verify_host"
TR_LABEL = b"sparse verify host"
TAMPER_SHAPES = [(2, 3, (3, 4, 1)), (2, 2, (4, 4, 4, 4))]
PROD = ("prod.eval_row", "prod.eval_col", "prod.eval_val", "prod.proof_mem", "prod.proof_ops")
HASH = ("hash.eval_row", "hash.eval_col", "hash.eval_val", "hash.eval_derefs")
_CACHE = {}


@pytest.fixture(scope="module")
def check(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("sparse_verify_host") / "sparse_verify_host_check")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        os.path.join(ROOT, "tests", "sparse_verify_host_check.cpp"), "-o", exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr

    def run(cases):
        def word(w):
            return str(w) if isinstance(w, (int, str)) else (bytes(w).hex() or "-")
        text = "".join(" ".join(word(w) for w in case) + "\n" for case in cases)
        r = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
        lines = r.stdout.splitlines()
        assert lines[-1] == "SPARSE VERIFY HOST CHECK DONE" and len(lines) == len(cases) + 1
        return [ln.split() for ln in lines[:-1]]
    return run


def sbs(xs):
    return b"".join(int(x).to_bytes(32, "little") for x in xs)


def unhex(w):
    return b"" if w == "-" else bytes.fromhex(w)


def proved(ol, shape_key):
    """one honest proof per shape for the whole module: everything the verifier holds, and the proof as bytes"""
    if shape_key not in _CACHE:
        nx, ny, _ = shape_key
        mats, rx, ry, evals, rnd = sem.instance(shape_key)
        dense = dm.Dense(nx, ny, mats)
        shape = sem.Shape(nx, ny, dense.N, dense.batch)
        gens = sem.make_gens({k: ol.gens_new(shape.R(k) + 1, LABEL + b"_" + k.encode())[0] for k in ("ops", "mem", "derefs")}, shape)
        proof = sem.prove(Transcript(TR_LABEL), nx, ny, mats, rx, ry, evals, gens, rnd)
        _CACHE[shape_key] = dict(rx=rx, ry=ry, evals=evals, shape=shape, gens=gens, comm=sem.commit_dense(dense, gens, shape), data=sem.proof_bytes(proof))
    return _CACHE[shape_key]


def fields_of(data, shape):
    return {f: data[lo:hi] for f, (lo, hi) in sem.field_spans(shape).items()}


def model_field_half(data, c, evals=None):
    """the model on bytes -> (state before the product layer, product-layer result or None, hash-layer field result or None)"""
    shape = c["shape"]
    evals = c["evals"] if evals is None else evals
    proof = sem.proof_from_bytes(data, shape)
    tr = Transcript(TR_LABEL)
    r_hash, r_multiset = sevm.begin(tr, proof["comm_derefs"])
    state0 = tr.state()
    got = sem.product_layer_verify(tr, proof["prod"], shape.N, shape.cells, evals)
    if got is None:
        return state0, None, None, (r_hash, r_multiset)
    claims_mem, rand_mem, claims_ops, claims_dotp, rand_ops = got
    rx_ext, ry_ext = sem.equalize(c["rx"], c["ry"])
    h = sevm.hash_layer_field(proof["hash"], shape.b, rand_mem, claims_mem, claims_ops, claims_dotp, rx_ext, ry_ext, r_hash, r_multiset)
    return state0, got + (tr.state(),), h, (r_hash, r_multiset)


def product_case(f, shape, state0, evals, num_ops=None, num_cells=None):
    return ["product", state0, shape.N if num_ops is None else num_ops, shape.cells if num_cells is None else num_cells, sbs(evals)] + [f[k] for k in PROD]


def hash_case(f, b, claims_mem, rand_mem, claims_ops, claims_dotp, c, rh):
    rx_ext, ry_ext = sem.equalize(c["rx"], c["ry"])
    return ["hash", b] + [f[k] for k in HASH] + [sbs(claims_mem), sbs(rand_mem), sbs(claims_ops), sbs(claims_dotp), sbs(rx_ext), sbs(ry_ext), sbs([rh[0]]), sbs([rh[1]])]


def header_field_half(check, data, c, evals=None):
    """the header on the same bytes: the product layer, then the hash layer on what it returned -> (accepted, product words, hash words)"""
    shape = c["shape"]
    evals = c["evals"] if evals is None else evals
    f = fields_of(data, shape)
    tr = Transcript(TR_LABEL)
    rh = sevm.begin(tr, sem.proof_from_bytes(data, shape)["comm_derefs"])
    p = check([product_case(f, shape, tr.state(), evals)])[0]
    if p[0] != "1":
        return False, p, None
    ints = lambda w: [int.from_bytes(unhex(w)[i:i + 32], "little") for i in range(0, len(unhex(w)), 32)]      # noqa: E731
    h = check([hash_case(f, shape.b, ints(p[1]), ints(p[2]), ints(p[3]), ints(p[4]), c, rh)])[0]
    return h[0] == "1", p, h


@pytest.mark.parametrize("shape_key", sem.SHAPES)
def test_the_header_computes_what_the_model_computes(check, ol, shape_key):
    c = proved(ol, shape_key)
    shape, data = c["shape"], c["data"]
    nx, ny, nnz = shape_key
    lay, canon = check([["layout", nx, ny, shape.N, shape.b], ["canon", nx, ny, shape.N, shape.b, data]])
    sp = sem.field_spans(shape)
    assert lay == ["1"] + [str(sp[f][0]) for f in sem.FIELDS] + [str(len(data))]
    assert canon == ["1"] and sevm.scalars_canonical(data, shape)
    state0, prod, hashr, _ = model_field_half(data, c)
    assert prod is not None and hashr is not None
    ok, p, h = header_field_half(check, data, c)
    assert ok
    claims_mem, rand_mem, claims_ops, claims_dotp, rand_ops, state1 = prod
    assert [unhex(w) for w in p[1:]] == [sbs(claims_mem), sbs(rand_mem), sbs(claims_ops), sbs(claims_dotp), sbs(rand_ops), state1]
    assert len(state1) == 203 and state1 != state0
    assert [unhex(w) for w in h[1:]] == [sbs(v) for v in hashr]
    # and the model's whole verifier accepts these bytes
    assert sevm.verify_bytes(Transcript(TR_LABEL), data, shape, c["comm"], c["rx"], c["ry"], c["evals"], c["gens"])


def model_refuses(data, c, evals=None):
    """the literal verdict on bytes is a refusal, and so is the model's field half (the openings are not what refuses)"""
    whole = sevm.verify_bytes(Transcript(TR_LABEL), data, c["shape"], c["comm"], c["rx"], c["ry"], c["evals"] if evals is None else evals, c["gens"])
    if not sevm.scalars_canonical(data, c["shape"]):
        return not whole
    _, prod, hashr, _ = model_field_half(data, c, evals)
    return not whole and (prod is None or hashr is None)


@pytest.mark.parametrize("shape_key", TAMPER_SHAPES)
@pytest.mark.parametrize("field", sevm.SCALAR_FIELDS)
def test_a_flipped_byte_in_each_scalar_field_is_refused(check, ol, shape_key, field):
    c = proved(ol, shape_key)
    lo, hi = sem.field_spans(c["shape"])[field]
    for at in (lo, hi - 32):                                         # the field's first and last scalar
        b = bytearray(c["data"]); b[at] ^= 1
        assert model_refuses(bytes(b), c), (field, at - lo)
        assert not header_field_half(check, bytes(b), c)[0], (field, at - lo)


@pytest.mark.parametrize("shape_key", TAMPER_SHAPES)
@pytest.mark.parametrize("field", ["prod.proof_ops", "hash.eval_row", "hash.proof_mem"])
def test_a_scalar_not_below_r_is_refused(check, ol, shape_key, field):
    c = proved(ol, shape_key)
    shape = c["shape"]
    nx, ny, _ = shape_key
    lo, hi = sem.field_spans(shape)[field]
    for v in (R, (1 << 256) - 1):
        b = bytearray(c["data"]); b[hi - 32:hi] = v.to_bytes(32, "little")
        assert not sevm.scalars_canonical(bytes(b), shape) and model_refuses(bytes(b), c)
        assert check([["canon", nx, ny, shape.N, shape.b, bytes(b)]])[0] == ["0"]
        if field in sevm.SCALAR_FIELDS:                              # (an opening's z1, z2 are read by the canonical check alone)
            assert not header_field_half(check, bytes(b), c)[0]


@pytest.mark.parametrize("shape_key", TAMPER_SHAPES)
def test_wrong_evals_are_refused(check, ol, shape_key):
    c = proved(ol, shape_key)
    for i in range(c["shape"].b):
        wrong = list(c["evals"]); wrong[i] = (wrong[i] + 1) % R
        assert model_refuses(c["data"], c, wrong)
        assert not header_field_half(check, c["data"], c, wrong)[0]


def _model_raises_or_refuses(fn):
    try:
        return fn() is None
    except (IndexError, ValueError, AssertionError, TypeError):      # the reference's verifier panics on these lengths
        return True


@pytest.mark.parametrize("shape_key", TAMPER_SHAPES)
def test_every_wrong_length_is_refused(check, ol, shape_key):
    c = proved(ol, shape_key)
    shape, data = c["shape"], c["data"]
    nx, ny, _ = shape_key
    f = fields_of(data, shape)
    state0, prod, hashr, rh = model_field_half(data, c)
    claims_mem, rand_mem, claims_ops, claims_dotp, rand_ops, _ = prod
    cases = []
    for k in PROD:                                                   # one scalar short, one scalar long
        for g in (f[k][:-32], f[k] + bytes(32)):
            cases.append(product_case(dict(f, **{k: g}), shape, state0, c["evals"]))
    cases.append(product_case(f, shape, state0, c["evals"], num_ops=2 * shape.N))
    cases.append(product_case(f, shape, state0, c["evals"], num_cells=2 * shape.cells))
    cases.append(product_case(f, shape, state0, c["evals"], num_ops=3))
    cases.append(product_case(f, shape, state0, list(c["evals"]) + [0]))
    cases.append(product_case(f, shape, state0, []))
    for k in HASH:
        for g in (f[k][:-32], f[k] + bytes(32)):
            cases.append(hash_case(dict(f, **{k: g}), shape.b, claims_mem, rand_mem, claims_ops, claims_dotp, c, rh))
    cases.append(hash_case(f, shape.b, claims_mem[:3], rand_mem, claims_ops, claims_dotp, c, rh))
    cases.append(hash_case(f, shape.b, claims_mem, rand_mem, claims_ops[:-1], claims_dotp, c, rh))
    cases.append(hash_case(f, shape.b, claims_mem, rand_mem, claims_ops, claims_dotp[:-1], c, rh))
    cases.append(hash_case(f, shape.b + 1, claims_mem, rand_mem, claims_ops, claims_dotp, c, rh))
    cases += [["canon", nx, ny, shape.N, shape.b, data[:-32]], ["canon", nx, ny, shape.N, shape.b, data + bytes(32)],
              ["layout", nx, ny, 3, shape.b], ["layout", nx, ny, 1, shape.b], ["layout", nx, ny, shape.N, 0], ["layout", 0, 0, shape.N, shape.b]]
    got = check(cases)
    assert all(g == ["0"] for g in got), [i for i, g in enumerate(got) if g != ["0"]]
    # the model on the same malformed structures
    proof = sem.proof_from_bytes(data, shape)
    tr0 = lambda: (lambda t: (sevm.begin(t, proof["comm_derefs"]), t)[1])(Transcript(TR_LABEL))      # noqa: E731
    for key in ("eval_row", "eval_col"):
        bad = copy.deepcopy(proof["prod"]); t = bad[key]; bad[key] = (t[0], t[1][:-1], t[2], t[3])
        assert _model_raises_or_refuses(lambda: sem.product_layer_verify(tr0(), bad, shape.N, shape.cells, c["evals"]))
    for key in ("proof_mem", "proof_ops"):
        bad = copy.deepcopy(proof["prod"]); bad[key]["polys"] = bad[key]["polys"][:-1]
        assert _model_raises_or_refuses(lambda: sem.product_layer_verify(tr0(), bad, shape.N, shape.cells, c["evals"]))
    assert _model_raises_or_refuses(lambda: sem.product_layer_verify(tr0(), proof["prod"], 2 * shape.N, shape.cells, c["evals"]))
    assert _model_raises_or_refuses(lambda: sem.product_layer_verify(tr0(), proof["prod"], shape.N, 2 * shape.cells, c["evals"]))
    assert _model_raises_or_refuses(lambda: sem.product_layer_verify(tr0(), proof["prod"], shape.N, shape.cells, list(c["evals"]) + [0]))
    rx_ext, ry_ext = sem.equalize(c["rx"], c["ry"])
    for cm, co, cd in ((claims_mem[:3], claims_ops, claims_dotp), (claims_mem, claims_ops[:-1], claims_dotp), (claims_mem, claims_ops, claims_dotp[:-1])):
        assert _model_raises_or_refuses(lambda: sevm.hash_layer_field(proof["hash"], shape.b, rand_mem, cm, co, cd, rx_ext, ry_ext, *rh))


def test_the_library_exports_the_one_call_check_and_refuses_it_without_a_context(sbn):
    """no device here: the symbol exists, and a call without a context is SBN_EINVAL with the transcript and the verdict word as they were"""
    import ctypes as C
    L = sbn.lib()
    assert hasattr(L, "sbn_sparse_eval_verify") and "sbn_sparse_eval_verify" in sbn.EXPORTED_SYMBOLS
    tr = sbn.Transcript(TR_LABEL)
    before = tr.state()
    buf = lambda k: (C.c_uint8 * k)()                      # noqa: E731
    acc, fake = C.c_int(7), C.c_void_p(0)
    n_proof = sbn.sparse_eval_sizes(2, 2, 4, 1)[1]
    rc = L.sbn_sparse_eval_verify(None, C.c_size_t(2), C.c_size_t(2), C.c_size_t(4), C.c_size_t(4), C.c_size_t(1), fake, fake, buf(64), buf(64), buf(32), fake, fake, fake,
                                  buf(n_proof), tr.h, C.byref(acc))
    assert rc == -1 and acc.value == 7 and tr.state() == before
