"""CPU: tests/nizk_model.py — the literal restatement of NIZKGens::new, NIZK::prove and NIZK::verify (snark.rs:162-287) that sbn_nizk_* is checked
against.  The model's prover and verifier must agree with each other on every raw shape (completeness and the same transcript), the two lines in front of
R1CSProof must be the hand-written Merlin script, and the verifier must refuse what it should: every tampering of the R1CS part, a claimed scalar = r, a
claimed point off by one coordinate, wrong inputs, another digest, another circuit under the same digest — and, on an instance whose matrices are empty,
a changed claimed point that the R1CS proof check itself lets through, so that only the comparison of snark.rs:280-281 refuses it."""
import pytest

import nizk_model as nm
import r1cs_proof_model as rpm
import r1cs_proof_verify_model as rpvm
from nizk_model import R_MOD, Transcript

TR = b"nizk cpu"
DIGEST = bytes(range(32))
_CACHE = {}


def _gens(ol, key):
    gk = tuple(nm.gens_sizes(*key[:3]))
    if gk not in _CACHE:
        _CACHE[gk] = [ol.gens_new(n, label)[0] for n, label in gk]
    return _CACHE[gk]


def _case(ol, key, digest=DIGEST, seed=11):
    """one honest proof per (raw shape, digest, seed) for the whole module"""
    ck = (key, digest, seed)
    if ck not in _CACHE:
        mats, vars_, inputs = nm.instance(key, seed)
        inst = nm.Instance(*key[:3], mats)
        gens = nm.make_gens(_gens(ol, key), inst)
        tp = Transcript(TR)
        proof = nm.prove(tp, inst, digest, vars_, inputs, gens, nm.random_rnd(inst, 3))
        _CACHE[ck] = dict(inst=inst, digest=digest, vars=vars_, inputs=inputs, gens=gens, proof=proof, data=nm.proof_bytes(proof), state=tp.state())
    return _CACHE[ck]


def _verdict(c, data=None, inputs=None, digest=None, inst=None):
    tv = Transcript(TR)
    before = tv.state()
    ok = nm.verify_bytes(tv, c["data"] if data is None else data, inst or c["inst"], c["digest"] if digest is None else digest, c["inputs"] if inputs is None else inputs, c["gens"])
    assert ok or tv.state() == before
    return ok, tv.state()


@pytest.mark.parametrize("key", nm.KEYS)
def test_prove_then_verify_accepts_and_ends_in_the_same_state(ol, key):
    c = _case(ol, key)
    assert nm.sm.is_sat(c["inst"], c["vars"], c["inputs"]) == (True, 0, None)
    assert len(c["data"]) == nm.sizes(c["inst"])[1] == rpm.sizes(c["inst"].nc, c["inst"].nv)[1] + 32 * (c["inst"].nx + c["inst"].ny)
    assert _verdict(c) == (True, c["state"])
    sp = nm.r_span(c["inst"])
    assert c["data"][sp["rx"][0]:sp["ry"][1]] == b"".join(x.to_bytes(32, "little") for x in c["proof"]["r"][0] + c["proof"]["r"][1])


def test_the_two_instances_only_nizk_takes_have_fewer_than_two_ops(ol):
    for key in (nm.ALL_EMPTY, nm.SINGLE):
        assert nm.sm.num_ops(_case(ol, key)["inst"]) < 2             # SNARK::encode's dot-product circuits cannot be split (product_tree.rs:89)
    assert all(nm.sm.num_ops(_case(ol, key)["inst"]) >= 2 for key in nm.SNARK_KEYS[:4])


def test_padded_and_raw_vars_give_the_same_proof(ol):
    c = _case(ol, (5, 3, 2, None))
    tp = Transcript(TR)
    again = nm.prove(tp, c["inst"], DIGEST, nm.pad_vars(c["vars"], c["inst"].nv), c["inputs"], c["gens"], nm.random_rnd(c["inst"], 3))
    assert nm.proof_bytes(again) == c["data"] and tp.state() == c["state"]


@pytest.mark.parametrize("digest", [b"", b"\x07", DIGEST, bytes(range(200))])
def test_prefix_is_the_hand_written_script(digest):
    want = Transcript(TR)
    want.append_message(b"protocol-name", b"Spartan NIZK proof")
    want.append_message(b"R1CSShapeDigest", digest)
    got = Transcript(TR)
    nm.append_prefix(got, digest)
    assert got.state() == want.state()
    other = Transcript(TR)
    nm.append_prefix(other, digest + b"\0")                          # the length is part of the message
    assert other.state() != want.state()


def test_gens_are_the_sat_half_of_the_snark_bundle():
    for shape in [(4, 4, 1), (5, 3, 2), (2, 40, 5), (1000, 900, 30)]:
        assert nm.gens_sizes(*shape) == nm.sm.gens_sizes(*shape, 64)[:3]


@pytest.mark.parametrize("key", [(4, 4, 1, None), (5, 3, 2, None)])
def test_verifier_refuses_each_tampering(ol, key):
    c = _case(ol, key)
    t = nm.tamperings(c["data"], c["inst"])
    sat_part = rpvm.tamperings(c["data"][:nm.r_span(c["inst"])["sat"][1]], c["inst"].nc, c["inst"].nv)
    assert set(t) == set(sat_part) | set(nm.R_TAMPERINGS) and len(t) == len(sat_part) + 6
    for name, data in t.items():
        assert _verdict(c, data=data)[0] is False, name
    wrong = list(c["inputs"]); wrong[-1] = (wrong[-1] + 1) % R_MOD
    assert _verdict(c, inputs=wrong)[0] is False
    assert _verdict(c, digest=DIGEST[:-1] + b"\xff")[0] is False and _verdict(c, digest=b"")[0] is False
    assert _verdict(c) == (True, c["state"])


def test_two_digests_give_two_proofs(ol):
    a, b = _case(ol, (4, 4, 1, None)), _case(ol, (4, 4, 1, None), digest=bytes(range(200)))
    assert a["data"] != b["data"] and a["state"] != b["state"]
    assert _verdict(b) == (True, b["state"]) and _verdict(b, digest=DIGEST)[0] is False


def test_the_verifier_reads_its_own_matrices(ol):
    """two circuits of one shape under the same digest bytes: the digest is not what binds the proof to the matrices, the evaluation is"""
    a, b = _case(ol, (4, 4, 1, None)), _case(ol, (4, 4, 1, None), seed=12)
    assert a["inst"].mats != b["inst"].mats and a["digest"] == b["digest"]
    assert _verdict(a) == (True, a["state"]) and _verdict(b) == (True, b["state"])
    assert _verdict(a, inst=b["inst"])[0] is False and _verdict(b, inputs=b["inputs"], inst=a["inst"])[0] is False


@pytest.mark.parametrize("key", [nm.ALL_EMPTY, (2, 2, 0, "empty")])
def test_the_comparison_on_its_own(ol, key):
    """A, B, C are 0 at every point of an instance without entries, so R1CSProof::verify passes whatever point the proof claims: it returns a point, and
    the point differs from the claim.  Only the comparison of snark.rs:280-281 stands between this proof and acceptance."""
    c = _case(ol, key)
    inst = c["inst"]
    assert all(len(m[0]) == 0 for m in inst.mats)
    rx, ry = c["proof"]["r"]
    for claimed in (([(rx[0] + 1) % R_MOD] + rx[1:], ry), (rx, ry[:-1] + [(ry[-1] + 1) % R_MOD])):
        tv = Transcript(TR)
        got = nm.verify(tv, dict(sat=c["proof"]["sat"], r=claimed), inst, c["digest"], c["inputs"], c["gens"])
        assert got == (True, False)                                  # the R1CS proof holds; the derived point is not the claimed one
        assert tv.state() == c["state"]                              # (the literal verifier has moved its transcript to the prover's end by then)
    data = nm.bump(c["data"], nm.r_span(inst)["rx"][0])
    assert _verdict(c, data=data)[0] is False and _verdict(c) == (True, c["state"])
