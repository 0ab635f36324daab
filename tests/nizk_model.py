"""NIZKGens::new, NIZK::prove and NIZK::verify in plain Python: a literal restatement of the reference's NIZK mode (snark.rs:162-287) composed of the
models of its parts — the checker of sbn_nizk_gens_new, sbn_nizk_prove and sbn_nizk_verify.

    gens_sizes           the three generator sets of NIZKGens::new                     (snark.rs:169-180, r1csproof.rs:177-182)
    append_prefix        protocol name + the digest bytes                               (:212-213, :252-253)
    prove / verify       NIZK::prove / ::verify                                         (:202-240, :243-286)
    sizes / proof_bytes / verify_bytes   the layout of include/sbn254.h and the literal verdict on bytes

Instance and pad_vars are snark_model's (Instance::new and Assignment::pad are shared by the two modes).  The digest is what it is to the reference's
prover and verifier: bytes that are appended (R1CSShape::get_digest computes them once, in Instance::new; nothing here does).  Built on r1cs_proof_model.py,
r1cs_model.py and snark_model.py, on the same footing as they are.  Scalars are Python integers mod r."""
import polyeval_model as pm
import r1cs_model as rm
import r1cs_proof_model as rpm
import snark_model as sm
from transcript_model import R_MOD, Transcript  # noqa: F401

NAME = b"Spartan NIZK proof"
Instance, pad_vars, pad_shape, log2 = sm.Instance, sm.pad_vars, sm.pad_shape, rpm.log2


def gens_sizes(num_cons, num_vars, num_inputs):
    """-> [(generators without h, label)] of pc, g3, g4: R1CSGens::new(b"gens_r1cs_sat", num_cons, num_vars_padded), snark.rs:178"""
    nv = pad_shape(num_cons, num_vars, num_inputs)[1]                                            # :170-176
    Rpc = 1 << pm.factored_lens(log2(nv))[1]
    return [(Rpc + 1, b"gens_r1cs_sat"), (3, b"gens_r1cs_sat"), (4, b"gens_r1cs_sat")]


def make_gens(points, inst):
    """points: the three point strings sbn_gens_new returns (n + 1 points each), in gens_sizes' order -> the gens dict of r1cs_proof_model"""
    return rpm.make_gens(points[0], 1 << pm.factored_lens(log2(inst.nv))[1], points[1], points[2])


def append_prefix(tr, digest):
    tr.append_message(b"protocol-name", NAME)                                                    # snark.rs:212, :252
    tr.append_message(b"R1CSShapeDigest", digest)                                                # :213, :253


def sizes(inst):
    """(scalars of rnd, bytes of the proof); rnd = R1CSProof::prove's draws, proof = r1cs_sat_proof | rx | ry (snark.rs:191-194)"""
    a = rpm.sizes(inst.nc, inst.nv)
    return a[0], a[1] + 32 * (inst.nx + inst.ny)


def prove(tr, inst, digest, vars_, inputs, gens, rnd):
    """NIZK::prove -> dict(sat=R1CSProof, r=(rx, ry))"""
    append_prefix(tr, digest)
    padded = pad_vars(vars_, inst.nv)                                                            # snark.rs:216-223
    sat, rx, ry = rpm.prove(tr, inst.nc, inst.nv, inst.mats, padded, inputs, gens, list(rnd))    # :225-232
    return dict(sat=sat, r=(list(rx), list(ry)))                                                 # :236-239


def proof_bytes(proof):
    return rpm.proof_bytes(proof["sat"]) + b"".join(pm.sb(x) for x in proof["r"][0] + proof["r"][1])


def verify(tr, proof, inst, digest, inputs, gens):
    """NIZK::verify on a parsed proof -> (the R1CS proof holds, the derived point is the claimed one).  The reference returns Err for a False first
    half and panics for a False second one (assert_eq!, snark.rs:280-281); `tr` moves as the reference's verifier moves it"""
    append_prefix(tr, digest)
    claimed_rx, claimed_ry = proof["r"]                                                          # :257
    evals = rm.evaluate(inst.nc, inst.nv, inst.mats, claimed_rx, claimed_ry)                     # :258
    assert len(inputs) == inst.ni                                                                # :262
    got = rpm.verify(tr, proof["sat"], inst.nv, inst.nc, inputs, tuple(evals), gens)             # :263-270
    if got is None:
        return False, None                                                                       # :271-277
    rx, ry = got
    return True, (list(rx), list(ry)) == (list(claimed_rx), list(claimed_ry))                    # :280-281


def verify_bytes(tr, data, inst, digest, inputs, gens):
    """the literal verdict on bytes -> bool, the comparison of snark.rs:280-281 as a refusal; `tr` moves on only behind an accepted proof"""
    n_sat = rpm.sizes(inst.nc, inst.nv)[1]
    assert len(data) == sizes(inst)[1]
    r = [int.from_bytes(data[o:o + 32], "little") for o in range(n_sat, len(data), 32)]
    if any(x >= R_MOD for x in r):                                                               # Scalar::from_bytes fails
        return False
    sat = rpm.proof_from_bytes(data[:n_sat], inst.nc, inst.nv)
    if sat is None:
        return False
    t = tr.clone()
    if verify(t, dict(sat=sat, r=(r[:inst.nx], r[inst.nx:])), inst, digest, inputs, gens) != (True, True):
        return False
    tr.s = t.s
    return True


# ---- instances ------------------------------------------------------------------------------------------------------------------

# raw (num_cons, num_vars, num_inputs, kind).  kind None / 0 / 1: snark_model.satisfying_instance with that matrix left empty — the seven shapes of
# tests/test_gpu_snark.py; "empty": three matrices without entries; "single": no matrix has more than one entry (SNARK::encode refuses both: N < 2)
SNARK_KEYS = [(4, 4, 1, None), (5, 3, 2, None), (2, 1, 3, None), (1, 2, 0, None), (40, 4, 2, None), (2, 40, 5, None), (6, 5, 1, 1)]
ALL_EMPTY = (4, 4, 1, "empty")
SINGLE = (2, 2, 0, "single")
KEYS = SNARK_KEYS + [ALL_EMPTY, SINGLE]


def instance(key, seed=11):
    """-> (mats, vars, inputs) of a satisfied raw circuit"""
    import random
    nc, nv, ni, kind = key
    if kind in ("empty", "single"):
        rng = random.Random(seed)
        vars_ = [rng.randrange(R_MOD) for _ in range(nv)]
        inputs = [rng.randrange(R_MOD) for _ in range(ni)]
        if kind == "empty":
            return (([], [], []),) * 3, vars_, inputs
        a = rng.randrange(1, R_MOD)                                                              # row 0: (a v0) (v1) = a v0 v1 at the constant column
        return (([0], [0], [a]), ([0], [1], [1]), ([0], [nv], [a * vars_[0] * vars_[1] % R_MOD])), vars_, inputs
    return sm.satisfying_instance(nc, nv, ni, seed=seed, empty=kind, min_entries=2 if nc == 1 else 1)


def random_rnd(inst, seed):
    return rpm.random_rnd(inst.nc, inst.nv, seed)


def r_span(inst):
    """{"sat" | "rx" | "ry": (first byte, end)}"""
    a = rpm.sizes(inst.nc, inst.nv)[1]
    return dict(sat=(0, a), rx=(a, a + 32 * inst.nx), ry=(a + 32 * inst.nx, a + 32 * (inst.nx + inst.ny)))


def with_scalar(data, at, value):
    """the proof with the 32 bytes at `at` replaced by `value`"""
    return data[:at] + int(value).to_bytes(32, "little") + data[at + 32:]


def bump(data, at):
    """the proof with the scalar at `at` raised by one (mod r): another canonical value"""
    return with_scalar(data, at, (int.from_bytes(data[at:at + 32], "little") + 1) % R_MOD)


R_TAMPERINGS = ("rx[0] = r", "the last of ry is itself + r", "rx[0] + 1", "the last of rx + 1", "ry[0] + 1", "the last of ry + 1")


def tamperings(data, inst):
    """{name: proof bytes}: what NIZK::verify must refuse, one change each — every entry of r1cs_proof_verify_model.tamperings on the R1CS part, a
    claimed scalar >= r, one coordinate of the claimed rx or ry changed"""
    import r1cs_proof_verify_model as rpvm
    sp = r_span(inst)
    out = {name: sat + data[sp["sat"][1]:] for name, sat in rpvm.tamperings(data[:sp["sat"][1]], inst.nc, inst.nv).items()}
    out["rx[0] = r"] = with_scalar(data, sp["rx"][0], R_MOD)
    out["the last of ry is itself + r"] = with_scalar(data, sp["ry"][1] - 32, int.from_bytes(data[-32:], "little") + R_MOD)
    out["rx[0] + 1"] = bump(data, sp["rx"][0])
    out["the last of rx + 1"] = bump(data, sp["rx"][1] - 32)
    out["ry[0] + 1"] = bump(data, sp["ry"][0])
    out["the last of ry + 1"] = bump(data, sp["ry"][1] - 32)
    assert len(out) == len(rpm.FIELDS) + 4 + len(R_TAMPERINGS)
    return out
