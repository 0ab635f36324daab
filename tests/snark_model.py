"""SNARK::encode / prove / verify and Instance::new / ::is_sat in plain Python: a literal restatement of the reference's public surface (snark.rs:59-158,
:290-529) composed of the models of its parts — the checker of sbn_snark_encode, sbn_snark_is_sat, sbn_snark_prove and sbn_snark_verify, both builds.

    pad_shape            Instance::new's and SNARKGens::new's padding                 (snark.rs:74-90, :306-319)
    Instance             Instance::new: the three errors and the column shift          (:92-110)
    is_sat               Instance::is_sat -> R1CSShape::is_sat                          (:137-158, r1cs.rs:105-123), with the violated rows
    gens_sizes           the six generator sets of SNARKGens::new                       (:321-322, r1csproof.rs:177-182, sparse_mlpoly_full.rs:612-630)
    encode               SNARK::encode -> R1CSShape::commit                             (:417-425, r1cs.rs:375-400)
    append_commitment    protocol name + R1CSCommitment::append_to_transcript           (:440-442, r1cs.rs:355-362, sparse_mlpoly_full.rs:710-717)
    prove / verify       SNARK::prove / ::verify                                        (:428-484, :487-528); srs given: the KZG build
    comm_bytes / proof_bytes / verify_bytes   the layouts of include/sbn254.h and the literal verdict on bytes

Built on r1cs_proof_model.py, r1cs_model.py, dense_model.py, sparse_eval_model.py, sparse_eval_kzg_model.py and transcript_model.py, on the same
footing as they are.  Scalars are Python integers mod r; points are 64-byte canonical affine x || y."""
import random

import dense_model as dm
import oracle_lib as ol
import polyeval_model as pm
import r1cs_model as rm
import r1cs_proof_model as rpm
import sparse_eval_kzg_model as skm
import sparse_eval_model as sem
import sparse_eval_verify_model as sevm
from transcript_model import R_MOD, Transcript  # noqa: F401

NAME = b"Spartan SNARK proof"
BATCH = 3
npo2, log2 = dm.next_power_of_two, rpm.log2


def pad_shape(num_cons, num_vars, num_inputs):
    """-> (num_cons_padded, num_vars_padded, nx, ny)"""
    nv = npo2(max(num_vars, num_inputs + 1))
    nc = npo2(max(num_cons, 2))
    return nc, nv, log2(nc), log2(2 * nv)


class InstanceError(ValueError):
    """R1CSError::InvalidIndex / InvalidScalar of Instance::new; args[0] is "row", "col" or "val" """


class Instance:
    """Instance::new (snark.rs:66-128): mats are three (rows, cols, vals) triplets with raw columns; self.mats has the padded instance's"""

    def __init__(self, num_cons, num_vars, num_inputs, mats):
        self.raw = (num_cons, num_vars, num_inputs)
        self.nc, self.nv, self.nx, self.ny = pad_shape(num_cons, num_vars, num_inputs)
        self.ni = num_inputs
        out = []
        for rows, cols, vals in mats:
            nr, ncl, nvl = [], [], []
            for row, col, val in zip(rows, cols, vals):
                if row >= num_cons:
                    raise InstanceError("row")
                if col >= num_vars + 1 + num_inputs:
                    raise InstanceError("col")
                if val >= R_MOD:
                    raise InstanceError("val")
                nr.append(row); ncl.append(col + self.nv - num_vars if col >= num_vars else col); nvl.append(val)
            out.append((nr, ncl, nvl))
        self.mats = tuple(out)


def pad_vars(vars_, nv):
    """Assignment::pad"""
    assert len(vars_) <= nv
    return list(vars_) + [0] * (nv - len(vars_))


def is_sat(inst, vars_, inputs):
    """-> (sat, the number of violated rows, the lowest of them or None)"""
    assert len(vars_) <= inst.nv and len(inputs) == inst.ni                                     # snark.rs:142-147
    z = rpm.build_z(pad_vars(vars_, inst.nv), inputs)
    Az, Bz, Cz = rm.multiply_vec(inst.nc, inst.nv, inst.mats, z)
    bad = [i for i in range(inst.nc) if (Az[i] * Bz[i] - Cz[i]) % R_MOD]
    return not bad, len(bad), (bad[0] if bad else None)


def num_ops(inst):
    return dm.num_ops(inst.mats)


def gens_sizes(num_cons, num_vars, num_inputs, num_nz_entries):
    """-> [(generators without h, label)] of pc, g3, g4, ops, mem, derefs: what sbn_gens_new is asked for"""
    nc, nv, nx, ny = pad_shape(num_cons, num_vars, num_inputs)
    s = sem.Shape(nx, ny, npo2(num_nz_entries), BATCH)
    Rpc = 1 << pm.factored_lens(log2(nv))[1]
    return [(Rpc + 1, b"gens_r1cs_sat"), (3, b"gens_r1cs_sat"), (4, b"gens_r1cs_sat")] + [(s.R(k) + 1, b"gens_r1cs_eval") for k in ("ops", "mem", "derefs")]


def make_gens(points, inst):
    """points: the six point strings sbn_gens_new returns (n + 1 points each), in gens_sizes' order -> dict(sat=..., eval=...)"""
    s = sem.Shape(inst.nx, inst.ny, num_ops(inst), BATCH)
    Rpc = 1 << pm.factored_lens(log2(inst.nv))[1]
    return dict(sat=rpm.make_gens(points[0], Rpc, points[1], points[2]), eval=sem.make_gens(dict(ops=points[3], mem=points[4], derefs=points[5]), s))


def encode(inst, gens):
    """SNARK::encode -> the commitment: dict(nc, nv, ni, batch, N, cells, ops=[points], mem=[points])"""
    dense = dm.Dense(inst.nx, inst.ny, inst.mats)
    s = sem.Shape(inst.nx, inst.ny, dense.N, dense.batch)
    ops, mem = sem.commit_dense(dense, gens["eval"], s)
    return dict(nc=inst.nc, nv=inst.nv, ni=inst.ni, batch=dense.batch, N=dense.N, cells=dense.cells, ops=ops, mem=mem)


def comm_bytes(comm):
    head = b"".join(comm[k].to_bytes(8, "little") for k in ("nc", "nv", "ni", "batch", "N", "cells"))
    return head + b"".join(ol.g1_compress(p) for p in comm["ops"]) + b"".join(ol.g1_compress(p) for p in comm["mem"])


def comm_lens(nc, nv, N):
    """(L_ops, L_mem)"""
    s = sem.Shape(log2(nc), log2(2 * nv), N, BATCH)
    return 1 << pm.factored_lens(s.ell["ops"])[0], 1 << pm.factored_lens(s.ell["mem"])[0]


def comm_from_bytes(b):
    """-> the commitment, or None for bytes sbn_snark_key_from_comm refuses"""
    if len(b) < 48:
        return None
    nc, nv, ni, batch, N, cells = (int.from_bytes(b[8 * k:8 * k + 8], "little") for k in range(6))
    pow2 = lambda x: x >= 1 and x & (x - 1) == 0                                                 # noqa: E731
    if not pow2(nc) or nc < 2 or not pow2(nv) or ni >= nv or batch != BATCH or not pow2(N) or N < 2:
        return None
    if cells != 1 << max(log2(nc), log2(2 * nv)):
        return None
    Lo, Lm = comm_lens(nc, nv, N)
    if len(b) != 48 + 32 * (Lo + Lm):
        return None
    pts = [ol.g1_decompress(b[48 + 32 * i:80 + 32 * i]) for i in range(Lo + Lm)]
    if any(p is None for p in pts):
        return None
    return dict(nc=nc, nv=nv, ni=ni, batch=batch, N=N, cells=cells, ops=pts[:Lo], mem=pts[Lo:])


def append_commitment(tr, comm):
    """the lines in front of R1CSProof (snark.rs:440-442); append_u64 is Merlin's: the eight little-endian bytes under the label"""
    tr.append_message(b"protocol-name", NAME)
    for label, k in ((b"num_cons", "nc"), (b"num_vars", "nv"), (b"num_inputs", "ni"), (b"batch_size", "batch"), (b"num_ops", "N"), (b"num_mem_cells", "cells")):
        tr.append_message(label, comm[k].to_bytes(8, "little"))
    sem.append_poly_commitment(tr, b"comm_comb_ops", comm["ops"])
    sem.append_poly_commitment(tr, b"comm_comb_mem", comm["mem"])


def sizes(comm, kzg=False):
    """(scalars of rnd, bytes of the proof); rnd = the sat half's draws | the eval half's, proof = r1cs_sat_proof | inst_evals | r1cs_eval_proof"""
    a = rpm.sizes(comm["nc"], comm["nv"])
    b = (skm if kzg else sem).sizes(log2(comm["nc"]), log2(2 * comm["nv"]), comm["N"], comm["batch"])
    return a[0] + b[0], a[1] + 96 + b[1]


def prove(tr, inst, comm, vars_, inputs, gens, rnd, srs=None):
    """SNARK::prove -> dict(sat=R1CSProof, evals=(A, B, C)(rx, ry), eval=SparseMatPolyEvalProof); rnd: ONE tape over both halves"""
    assert len(rnd) == sizes(comm, srs is not None)[0]
    n_sat = rpm.sizes(inst.nc, inst.nv)[0]
    append_commitment(tr, comm)
    sat, rx, ry = rpm.prove(tr, inst.nc, inst.nv, inst.mats, pad_vars(vars_, inst.nv), inputs, gens["sat"], list(rnd[:n_sat]))
    evals = rm.evaluate(inst.nc, inst.nv, inst.mats, rx, ry)
    if srs is None:
        ev = sem.prove(tr, inst.nx, inst.ny, inst.mats, rx, ry, list(evals), gens["eval"], list(rnd[n_sat:]))
    else:
        ev = skm.prove(tr, inst.nx, inst.ny, inst.mats, rx, ry, list(evals), gens["eval"], srs, list(rnd[n_sat:]))
    return dict(sat=sat, evals=tuple(evals), eval=ev)


def proof_bytes(proof, kzg=False):
    return rpm.proof_bytes(proof["sat"]) + b"".join(pm.sb(e) for e in proof["evals"]) + (skm if kzg else sem).proof_bytes(proof["eval"])


def proof_spans(comm, kzg=False):
    """{"sat" | "evals" | "eval": (first byte, end)}"""
    a = rpm.sizes(comm["nc"], comm["nv"])[1]
    return dict(sat=(0, a), evals=(a, a + 96), eval=(a + 96, sizes(comm, kzg)[1]))


def verify(tr, proof, comm, inputs, gens, srs=None):
    """SNARK::verify on a parsed proof -> bool; `tr` moves as the reference's verifier moves it"""
    assert len(inputs) == comm["ni"]                                                             # snark.rs:501
    append_commitment(tr, comm)
    got = rpm.verify(tr, proof["sat"], comm["nv"], comm["nc"], inputs, proof["evals"], gens["sat"])
    if got is None:
        return False
    rx, ry = got
    if srs is None:
        return sem.verify(tr, proof["eval"], (comm["ops"], comm["mem"]), comm["N"], comm["cells"], rx, ry, list(proof["evals"]), gens["eval"])
    return skm.verify(tr, proof["eval"], (comm["ops"], comm["mem"]), comm["N"], comm["cells"], rx, ry, list(proof["evals"]), gens["eval"], srs)


def verify_bytes(tr, data, comm, inputs, gens, srs=None):
    """the literal verdict on bytes -> bool; `tr` moves on only behind an accepted proof"""
    kzg = srs is not None
    sp = proof_spans(comm, kzg)
    assert len(data) == sp["eval"][1]
    evals = [int.from_bytes(data[o:o + 32], "little") for o in range(sp["evals"][0], sp["evals"][1], 32)]
    if any(e >= R_MOD for e in evals):                                                           # Scalar::from_bytes fails
        return False
    sat = rpm.proof_from_bytes(data[slice(*sp["sat"])], comm["nc"], comm["nv"])
    shape = sem.Shape(log2(comm["nc"]), log2(2 * comm["nv"]), comm["N"], comm["batch"])
    ed = data[slice(*sp["eval"])]
    if not kzg and not sevm.scalars_canonical(ed, shape):
        return False
    ev = (skm if kzg else sem).proof_from_bytes(ed, shape)
    if sat is None or ev is None:
        return False
    t = tr.clone()
    if not verify(t, dict(sat=sat, evals=tuple(evals), eval=ev), comm, inputs, gens, srs):
        return False
    tr.s = t.s
    return True


# ---- instances ------------------------------------------------------------------------------------------------------------------

def satisfying_instance(num_cons, num_vars, num_inputs, seed, empty=None, min_entries=1, vars_=None, only_vals=None):
    """a raw instance in the circuit's own numbering (vars | 1 | inputs): sparse random A and B rows over the live columns, a random witness, and C
    with one entry per row at the constant-one column whose value is (Az)_i (Bz)_i.  empty: the index of a matrix left without entries (0 or 1:
    every product is then 0 and C holds explicit zeros); min_entries: the fewest entries a row of A or B gets (2 where num_cons = 1, so that N >= 2);
    vars_: the witness to build the instance around; only_vals: the values the witness, the inputs and the entries of A and B are drawn from
    -> (mats, vars, inputs)"""
    rng = random.Random(seed)
    draw = (lambda: rng.choice(only_vals)) if only_vals else (lambda: rng.randrange(R_MOD))
    vars_ = [draw() for _ in range(num_vars)] if vars_ is None else list(vars_)
    inputs = [draw() for _ in range(num_inputs)]
    z = vars_ + [1] + inputs
    live = len(z)

    def sparse(k):
        rows, cols, vals = [], [], []
        if k != empty:
            for i in range(num_cons):
                for _ in range(rng.randrange(min_entries, 4)):
                    rows.append(i); cols.append(rng.randrange(live)); vals.append(rng.choice([1, R_MOD - 1, draw()]))
        return rows, cols, vals
    A, B = sparse(0), sparse(1)

    def times_z(m):
        y = [0] * num_cons
        for r, c, v in zip(*m):
            y[r] = (y[r] + v * z[c]) % R_MOD
        return y
    Az, Bz = times_z(A), times_z(B)
    C = (list(range(num_cons)), [num_vars] * num_cons, [a * b % R_MOD for a, b in zip(Az, Bz)])
    return (A, B, C), vars_, inputs


def random_rnd(comm, seed, kzg=False):
    rng = random.Random(seed)
    return [rng.randrange(R_MOD) for _ in range(sizes(comm, kzg)[0])]
