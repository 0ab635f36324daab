"""CPU: tests/snark_model.py — the literal restatement of Instance::new, SNARK::encode, Instance::is_sat, SNARK::prove and SNARK::verify (snark.rs:59-158,
:290-529) that sbn_snark_* is checked against.  The model's prover and verifier must agree with each other (completeness and the same transcript, both
builds), the verifier must refuse what it should, and the lines in front of R1CSProof must be the hand-written Merlin script."""
import pytest

import snark_model as sm
import sparse_eval_kzg_model as skm
from snark_model import R_MOD, Transcript

TR = b"snark cpu"
SHAPES = [(4, 4, 1), (5, 3, 2), (2, 1, 3), (1, 2, 0)]
TAU = 0x1234567890abcdef1234567890abcdef
_CACHE = {}


def _case(ol, shape, kzg=False):
    """one honest proof per (shape, build) for the whole module"""
    key = (shape, kzg)
    if key not in _CACHE:
        mats, vars_, inputs = sm.satisfying_instance(*shape, seed=11, min_entries=2 if shape[0] == 1 else 1)
        inst = sm.Instance(*shape, mats)
        assert sm.num_ops(inst) >= 2
        gk = tuple(sm.gens_sizes(*shape, sm.num_ops(inst)))
        if gk not in _CACHE:
            _CACHE[gk] = [ol.gens_new(n, label)[0] for n, label in gk]
        gens = sm.make_gens(_CACHE[gk], inst)
        comm = sm.encode(inst, gens)
        srs = skm.Srs(TAU, 2 * 4 * comm["N"] + 1) if kzg else None
        tp = Transcript(TR)
        proof = sm.prove(tp, inst, comm, vars_, inputs, gens, sm.random_rnd(comm, 3, kzg), srs)
        _CACHE[key] = dict(inst=inst, vars=vars_, inputs=inputs, gens=gens, comm=comm, srs=srs, proof=proof, data=sm.proof_bytes(proof, kzg), state=tp.state())
    return _CACHE[key]


def _verdict(c, data=None, inputs=None, comm=None):
    tv = Transcript(TR)
    before = tv.state()
    ok = sm.verify_bytes(tv, c["data"] if data is None else data, comm or c["comm"], c["inputs"] if inputs is None else inputs, c["gens"], c["srs"])
    assert ok or tv.state() == before
    return ok, tv.state()


@pytest.mark.parametrize("shape", SHAPES)
def test_prove_then_verify_accepts_and_ends_in_the_same_state(ol, shape):
    c = _case(ol, shape)
    assert sm.is_sat(c["inst"], c["vars"], c["inputs"]) == (True, 0, None)
    assert len(c["data"]) == sm.sizes(c["comm"])[1]
    assert _verdict(c) == (True, c["state"])
    cb = sm.comm_bytes(c["comm"])
    assert sm.comm_bytes(sm.comm_from_bytes(cb)) == cb


def test_the_kzg_build(ol):
    c = _case(ol, (5, 3, 2), kzg=True)
    assert len(c["data"]) == sm.sizes(c["comm"], True)[1]
    assert _verdict(c) == (True, c["state"])
    lo = sm.proof_spans(c["comm"], True)["eval"][0]
    bad = bytearray(c["data"]); bad[lo] ^= 1                # comm_derefs
    assert _verdict(c, data=bytes(bad))[0] is False


def test_padded_and_raw_vars_give_the_same_proof(ol):
    c = _case(ol, (5, 3, 2))
    tp = Transcript(TR)
    again = sm.prove(tp, c["inst"], c["comm"], sm.pad_vars(c["vars"], c["inst"].nv), c["inputs"], c["gens"], sm.random_rnd(c["comm"], 3))
    assert sm.proof_bytes(again) == c["data"] and tp.state() == c["state"]


def tamperings(c, kzg=False):
    """{name: proof bytes}: what SNARK::verify must refuse, one change each"""
    sp = sm.proof_spans(c["comm"], kzg)
    out = {}
    for k in range(3):
        b = bytearray(c["data"]); b[sp["evals"][0] + 32 * k] ^= 1
        out["inst_evals[%d]" % k] = bytes(b)
    for half in ("sat", "eval"):
        b = bytearray(c["data"]); b[sp[half][1] - 32] ^= 1  # the last scalar of the half
        out["one byte in the %s half" % half] = bytes(b)
    b = bytearray(c["data"]); b[sp["evals"][0] + 32:sp["evals"][0] + 64] = R_MOD.to_bytes(32, "little")
    out["inst_evals[1] = r"] = bytes(b)
    return out


@pytest.mark.parametrize("shape", [(4, 4, 1), (5, 3, 2)])
def test_verifier_refuses_each_tampering(ol, shape):
    c = _case(ol, shape)
    t = tamperings(c)
    assert len(t) == 6
    for name, data in t.items():
        assert _verdict(c, data=data)[0] is False, name
    wrong = list(c["inputs"]); wrong[0] = (wrong[0] + 1) % R_MOD
    assert _verdict(c, inputs=wrong)[0] is False
    for seed in range(12, 60):                              # the key of another circuit of the same padded shape and N
        inst2 = sm.Instance(*shape, sm.satisfying_instance(*shape, seed=seed)[0])
        if sm.num_ops(inst2) == c["comm"]["N"]:
            break
    other = sm.encode(inst2, c["gens"])
    assert other != c["comm"] and sm.sizes(other) == sm.sizes(c["comm"])
    assert _verdict(c, comm=other)[0] is False


def test_prefix_is_the_hand_written_script(ol):
    c = _case(ol, (5, 3, 2))
    comm = c["comm"]
    assert (comm["nc"], comm["nv"], comm["ni"], comm["batch"], comm["cells"]) == (8, 4, 2, 3, 8)
    want = Transcript(TR)
    want.append_message(b"protocol-name", b"Spartan SNARK proof")
    for label, x in ((b"num_cons", 8), (b"num_vars", 4), (b"num_inputs", 2), (b"batch_size", 3), (b"num_ops", comm["N"]), (b"num_mem_cells", 8)):
        want.append_message(label, x.to_bytes(8, "little"))
    for label, pts in ((b"comm_comb_ops", comm["ops"]), (b"comm_comb_mem", comm["mem"])):
        want.append_message(label, b"poly_commitment_begin")
        for p in pts:
            want.append_message(b"poly_commitment_share", ol.g1_compress(p))
        want.append_message(label, b"poly_commitment_end")
    got = Transcript(TR)
    sm.append_commitment(got, comm)
    assert got.state() == want.state()
    assert (len(comm["ops"]), len(comm["mem"])) == sm.comm_lens(comm["nc"], comm["nv"], comm["N"])


def test_instance_new_shifts_columns_and_refuses_bad_entries():
    mats = (([0, 4], [0, 3], [1, 2]), ([1], [4], [3]), ([2], [5], [R_MOD - 1]))          # (5, 3, 2): vars 0..2, the constant 3, inputs 4, 5
    inst = sm.Instance(5, 3, 2, mats)
    assert (inst.nc, inst.nv, inst.nx, inst.ny) == (8, 4, 3, 3)
    assert [m[1] for m in inst.mats] == [[0, 4], [5], [6]] and [m[0] for m in inst.mats] == [[0, 4], [1], [2]]
    for bad, why in (((([5], [0], [1]), ([], [], []), ([], [], [])), "row"), ((([0], [6], [1]), ([], [], []), ([], [], [])), "col"),
                     ((([], [], []), ([], [], []), ([0], [0], [R_MOD])), "val")):
        with pytest.raises(sm.InstanceError) as e:
            sm.Instance(5, 3, 2, bad)
        assert e.value.args[0] == why
    assert sm.pad_shape(1, 2, 0) == (2, 2, 1, 2) and sm.pad_shape(2, 1, 3) == (2, 4, 1, 3) and sm.pad_shape(40, 4, 2) == (64, 4, 6, 3) and sm.pad_shape(2, 40, 5) == (2, 64, 1, 7)


def test_is_sat_names_the_violated_rows(ol):
    c = _case(ol, (5, 3, 2))
    inst = c["inst"]
    A, B, (cr, cc, cv) = inst.mats
    for rows in ([0], [4], [1, 3], [0, 1, 2, 3, 4]):
        cv2 = list(cv)
        for r in rows:
            cv2[r] = (cv2[r] + 1) % R_MOD
        bad = sm.Instance.__new__(sm.Instance)
        bad.__dict__.update(inst.__dict__); bad.mats = (A, B, (cr, cc, cv2))
        assert sm.is_sat(bad, c["vars"], c["inputs"]) == (False, len(rows), rows[0])


def test_comm_bytes_are_refused_field_by_field(ol):
    c = _case(ol, (5, 3, 2))
    cb = sm.comm_bytes(c["comm"])
    assert sm.comm_from_bytes(cb) is not None
    assert sm.comm_from_bytes(cb[:-1]) is None and sm.comm_from_bytes(cb + b"\0") is None and sm.comm_from_bytes(cb[:47]) is None
    for k, v in ((0, 6), (0, 1), (1, 3), (2, 4), (3, 2), (4, 1), (4, 3), (5, 16)):
        b = bytearray(cb); b[8 * k:8 * k + 8] = v.to_bytes(8, "little")
        assert sm.comm_from_bytes(bytes(b)) is None, (k, v)
