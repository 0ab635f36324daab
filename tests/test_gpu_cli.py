"""GPU: sbn_spartan, the compiled caller of the C ABI that takes files (harness/sbn_spartan.cpp), run as child processes, one at a time, on circuits of a few
constraints written by tests/circom_model.py: the commitment and the proof bytes against the literal models, the exit statuses, the round trips of both modes
and of the KZG build over a saved SRS file.  After a child that died of a signal or ran into its time limit the module starts no further child: the
remaining tests fail at once."""
import os
import subprocess

import pytest

import circom_model as cm
import circuit_digest_model as dm
import nizk_model as nm
import oracle_lib as ol
import polyeval_model as pm
import proof_file_model as pfm
import random_tape_model as rtm
import snark_model as sm
import sparse_eval_kzg_model as skm
import sparse_eval_model as sem
from conftest import PKG_DIR, golden
from snark_model import R_MOD, Transcript

pytestmark = pytest.mark.gpu
EXE = os.path.join(PKG_DIR, "sbn_spartan")
LABEL = b"keyless_snark"
INIT = 0x5eed5eed5eed5eed1234 * 0x10000000000000001 % R_MOD
NC, NV, NI = 5, 3, 2
TAU = int(golden("pairing_kat.json")["tau"], 16)
_STATE = {"dead": None}


def run(*args, timeout=120):
    """one child; -> CompletedProcess.  A child that was killed or timed out ends the module's use of the GPU"""
    if _STATE["dead"]:
        pytest.fail("no further child is started: " + _STATE["dead"])
    assert os.path.exists(EXE), f"{EXE} is missing: run make"
    try:
        r = subprocess.run([EXE, *map(str, args)], capture_output=True, text=True, timeout=timeout)
    except subprocess.TimeoutExpired:
        _STATE["dead"] = f"`sbn_spartan {' '.join(map(str, args))}` ran into its time limit"
        pytest.fail(_STATE["dead"])
    if r.returncode < 0 or r.returncode > 3:
        _STATE["dead"] = f"`sbn_spartan {' '.join(map(str, args))}` ended with status {r.returncode}: {r.stderr[-500:]}"
        pytest.fail(_STATE["dead"])
    return r


def _sbs(xs):
    return b"".join(pm.sb(x) for x in xs)


@pytest.fixture(scope="module")
def w(tmp_path_factory):
    """the files and the model's side of two circuits of one shape that differ in one value"""
    d = tmp_path_factory.mktemp("cli")
    mats, vars_, inputs = sm.satisfying_instance(NC, NV, NI, seed=11)
    r1, wt = cm.raw_to_circom(NC, NV, NI, mats, vars_, inputs)
    A2 = (mats[0][0], mats[0][1], [(mats[0][2][0] + 1) % R_MOD] + mats[0][2][1:])
    r2, _ = cm.raw_to_circom(NC, NV, NI, (A2, mats[1], mats[2]), vars_, inputs)
    bad_vars = [(vars_[0] + 1) % R_MOD] + vars_[1:]
    _, wt_bad = cm.raw_to_circom(NC, NV, NI, mats, bad_vars, inputs)
    paths = {}
    for name, data in (("c1.r1cs", r1), ("c2.r1cs", r2), ("w.wtns", wt), ("bad.wtns", wt_bad)):
        paths[name] = str(d / name)
        with open(paths[name], "wb") as f:
            f.write(data)
    inst = sm.Instance(NC, NV, NI, mats)
    nnz = max(len(m[0]) for m in mats)
    gens = sm.make_gens([ol.gens_new(n, label)[0] for n, label in sm.gens_sizes(NC, NV, NI, nnz)], inst)
    comm = sm.encode(inst, gens)
    return dict(dir=d, p=paths, r1=r1, r2=r2, mats=mats, vars=vars_, bad_vars=bad_vars, inputs=inputs, inst=inst, nnz=nnz, gens=gens, comm=comm)


def out(w, name):
    return str(w["dir"] / name)


def read(path):
    with open(path, "rb") as f:
        return f.read()


def first_violated(mats, vars_, inputs):
    z = list(vars_) + [1] + list(inputs)
    y = []
    for rows, cols, vals in mats:
        acc = [0] * NC
        for r, c, v in zip(rows, cols, vals):
            acc[r] = (acc[r] + v * z[c]) % R_MOD
        y.append(acc)
    bad = [i for i in range(NC) if (y[0][i] * y[1][i] - y[2][i]) % R_MOD]
    return len(bad), bad[0]


def test_info_prints_the_shape_and_the_digest(w):
    r = run("info", w["p"]["c1.r1cs"])
    assert r.returncode == 0, r.stderr
    fields = dict(ln.split(" ", 1) for ln in r.stdout.splitlines())
    assert fields["digest"] == dm.digest_of_file(w["r1"]).hex()
    assert (fields["num_constraints"], fields["num_variables"], fields["num_pub_inputs"], fields["num_vars"]) == (str(NC), str(1 + NI + NV), str(NI), str(NV))
    assert fields["num_cons_padded"] == str(w["inst"].nc) and fields["num_vars_padded"] == str(w["inst"].nv)
    assert fields["nnz"] == " ".join(str(len(m[0])) for m in w["mats"])


def test_encode_writes_the_models_commitment(w):
    r = run("encode", w["p"]["c1.r1cs"], "-o", out(w, "c1.comm"))
    assert r.returncode == 0, r.stderr
    assert read(out(w, "c1.comm")) == sm.comm_bytes(w["comm"])


def test_snark_proof_with_a_fixed_tape_is_the_models_and_verifies(w):
    r = run("prove", "--mode", "snark", w["p"]["c1.r1cs"], w["p"]["w.wtns"], "-o", out(w, "p.sbnp"), "--tape-init", pm.sb(INIT).hex(), "--check-sat")
    assert r.returncode == 0, r.stderr
    f = pfm.read(read(out(w, "p.sbnp")), pfm.SNARK, 0)
    rnd = rtm.draw_snark(rtm.RandomTape(rtm.SNARK_NAME, INIT), w["comm"])
    want = sm.proof_bytes(sm.prove(Transcript(LABEL), w["inst"], w["comm"], w["vars"], w["inputs"], w["gens"], rnd))
    assert f["proof"] == want and f["inputs"] == _sbs(w["inputs"]) and f["digest"] == b""
    assert (f["num_cons"], f["num_vars"], f["num_inputs"], f["num_nz"]) == (NC, NV, NI, w["nnz"])
    # the breakdown by proof field: the spans of snark_model.proof_spans
    spans = sm.proof_spans(w["comm"])
    lines = [ln.split() for ln in r.stdout.splitlines() if ln.startswith("proof ")]
    assert [(ln[1], int(ln[3]), int(ln[5])) for ln in lines[:3]] == [("r1cs_sat_proof", *spans["sat"]), ("inst_evals", *spans["evals"]), ("r1cs_eval_proof", *spans["eval"])]
    assert any(ln.startswith("stage prove") or ln.startswith("stage check_sat+prove") for ln in r.stdout.splitlines())
    if not os.path.exists(out(w, "c1.comm")):
        assert run("encode", w["p"]["c1.r1cs"], "-o", out(w, "c1.comm")).returncode == 0
    v = run("verify", "--mode", "snark", out(w, "c1.comm"), out(w, "p.sbnp"))
    assert v.returncode == 0 and "accepted" in v.stdout, v.stderr


@pytest.fixture(scope="module")
def snark_files(w):
    """a commitment and a proof made without --tape-init"""
    assert run("encode", w["p"]["c1.r1cs"], "-o", out(w, "s.comm")).returncode == 0
    assert run("prove", "--mode", "snark", w["p"]["c1.r1cs"], w["p"]["w.wtns"], "-o", out(w, "s1.sbnp")).returncode == 0
    return out(w, "s.comm"), out(w, "s1.sbnp")


def test_two_proves_without_a_fixed_tape_differ_and_both_verify(w, snark_files):
    comm, p1 = snark_files
    assert run("prove", "--mode", "snark", w["p"]["c1.r1cs"], w["p"]["w.wtns"], "-o", out(w, "s2.sbnp")).returncode == 0
    a, b = pfm.read(read(p1)), pfm.read(read(out(w, "s2.sbnp")))
    assert a["proof"] != b["proof"] and len(a["proof"]) == len(b["proof"]) and a["inputs"] == b["inputs"]
    assert run("verify", "--mode", "snark", comm, p1).returncode == 0
    assert run("verify", "--mode", "snark", comm, out(w, "s2.sbnp")).returncode == 0


def test_a_flipped_proof_byte_and_altered_inputs_are_refused(w, snark_files):
    comm, p1 = snark_files
    data = bytearray(read(p1))
    f = pfm.read(bytes(data))
    proof_at = len(data) - len(f["proof"])
    flipped = bytearray(data); flipped[proof_at + len(f["proof"]) // 2] ^= 1
    inputs_at = proof_at - 8 - 32 * NI
    assert bytes(data[inputs_at:inputs_at + 32 * NI]) == _sbs(w["inputs"])
    altered = bytearray(data); altered[inputs_at:inputs_at + 32] = pm.sb((w["inputs"][0] + 1) % R_MOD)
    for name, d in (("flipped.sbnp", flipped), ("altered.sbnp", altered)):
        with open(out(w, name), "wb") as fh:
            fh.write(d)
        r = run("verify", "--mode", "snark", comm, out(w, name))
        assert r.returncode == 1 and "refused" in r.stdout, (name, r.returncode, r.stderr)


def test_a_truncated_or_contradicting_proof_file_is_an_error(w, snark_files):
    comm, p1 = snark_files
    data = read(p1)
    for name, d in (("cut.sbnp", data[:-1]), ("cut2.sbnp", data[:40]), ("tail.sbnp", data + b"\0")):
        with open(out(w, name), "wb") as fh:
            fh.write(d)
        r = run("verify", "--mode", "snark", comm, out(w, name))
        assert r.returncode == 2 and "proof file is refused" in r.stderr, (name, r.returncode, r.stderr)
    r = run("verify", "--mode", "nizk", w["p"]["c1.r1cs"], p1)                          # a snark proof where a nizk one is asked for
    assert r.returncode == 2 and "mode" in r.stderr
    assert run("verify", "--mode", "snark", comm, out(w, "missing.sbnp")).returncode == 2
    assert run("prove", "--mode", "snark", w["p"]["c1.r1cs"]).returncode == 2            # usage


def test_nizk_round_trip_with_the_device_digest_and_the_other_circuit(w):
    r = run("prove", "--mode", "nizk", w["p"]["c1.r1cs"], w["p"]["w.wtns"], "-o", out(w, "n.sbnp"), "--tape-init", pm.sb(INIT).hex())
    assert r.returncode == 0, r.stderr
    f = pfm.read(read(out(w, "n.sbnp")), pfm.NIZK, 0)
    digest = dm.digest_of_file(w["r1"])
    assert f["digest"] == digest
    inst = nm.Instance(NC, NV, NI, w["mats"])
    gens = nm.make_gens([ol.gens_new(n, label)[0] for n, label in nm.gens_sizes(NC, NV, NI)], inst)
    rnd = rtm.draw_nizk(rtm.RandomTape(rtm.NIZK_NAME, INIT), inst)
    assert f["proof"] == nm.proof_bytes(nm.prove(Transcript(LABEL), inst, digest, w["vars"], w["inputs"], gens, rnd))
    v = run("verify", "--mode", "nizk", w["p"]["c1.r1cs"], out(w, "n.sbnp"))
    assert v.returncode == 0 and "accepted" in v.stdout, v.stderr
    # the point of the digest: the same proof against another circuit of the same shape
    v = run("verify", "--mode", "nizk", w["p"]["c2.r1cs"], out(w, "n.sbnp"))
    assert v.returncode == 1 and "refused" in v.stdout, (v.returncode, v.stderr)
    assert run("verify", "--mode", "nizk", w["p"]["c1.r1cs"], out(w, "n.sbnp"), "--label", "another").returncode == 1


@pytest.mark.parametrize("mode", ["snark", "nizk"])
def test_an_unsatisfying_witness_under_check_sat(w, mode):
    count, first = first_violated(w["mats"], w["bad_vars"], w["inputs"])
    assert count >= 1
    r = run("prove", "--mode", mode, w["p"]["c1.r1cs"], w["p"]["bad.wtns"], "-o", out(w, "bad.sbnp"), "--check-sat")
    assert r.returncode == 3, (r.returncode, r.stderr)
    assert f"{count} constraints violated, the first is constraint {first}" in r.stderr
    assert not os.path.exists(out(w, "bad.sbnp"))


def test_kzg_round_trip_over_a_saved_srs_file(w, ctx, sbn):
    srs_n = (1 << sem.Shape(w["inst"].nx, w["inst"].ny, w["comm"]["N"], 3).ell["derefs"]) + 1
    srs = ctx.kzg_srs_from_tau(pm.sb(TAU), srs_n)
    try:
        g2_xy, tau_xy = sbn.kzg_srs_g2_from_tau(pm.sb(TAU))
        with open(out(w, "srs.bin"), "wb") as fh:
            fh.write(ctx.kzg_srs_save(srs, g2_xy, tau_xy))
    finally:
        srs.free()
    srs_path = out(w, "srs.bin")
    assert run("encode", w["p"]["c1.r1cs"], "-o", out(w, "k.comm"), "--srs", srs_path).returncode == 0
    assert read(out(w, "k.comm")) == sm.comm_bytes(w["comm"])
    r = run("prove", "--mode", "snark", w["p"]["c1.r1cs"], w["p"]["w.wtns"], "-o", out(w, "k.sbnp"), "--srs", srs_path, "--tape-init", pm.sb(INIT).hex())
    assert r.returncode == 0, r.stderr
    f = pfm.read(read(out(w, "k.sbnp")), pfm.SNARK, 1)
    rnd = rtm.draw_snark(rtm.RandomTape(rtm.SNARK_NAME, INIT), w["comm"], kzg=True)
    assert f["proof"] == sm.proof_bytes(sm.prove(Transcript(LABEL), w["inst"], w["comm"], w["vars"], w["inputs"], w["gens"], rnd, skm.Srs(TAU, srs_n)), True)
    v = run("verify", "--mode", "snark", out(w, "k.comm"), out(w, "k.sbnp"), "--srs", srs_path)
    assert v.returncode == 0 and "accepted" in v.stdout, v.stderr
    assert run("verify", "--mode", "snark", out(w, "k.comm"), out(w, "k.sbnp")).returncode == 2      # a KZG proof without --srs: the file contradicts the command line
