"""GPU: sbn_spartan with a powers-of-tau ceremony file (.ptau), run as child processes, one at a time, on the smallest circuit tests/test_gpu_cli.py uses:
`info` against the model's scan, `srs` against the model's reference-format file, the KZG build's proof from either file format byte for byte, and the
exit status of a corrupted file.  After a child that died of a signal or ran into its time limit the module starts no further child."""
import os
import subprocess

import pytest

import circom_model as cm
import dense_model as dm
import oracle_lib as ol
import pairing_model as pm
import polyeval_model as pem
import ptau_model as ptm
import snark_model as sm
import sparse_eval_model as sem
import srs_model as srm
from conftest import PKG_DIR
from snark_model import R_MOD

pytestmark = pytest.mark.gpu
EXE = os.path.join(PKG_DIR, "sbn_spartan")
INIT = 0x5eed5eed5eed5eed1234 * 0x10000000000000001 % R_MOD
NC, NV, NI = 5, 3, 2
TAU = srm.FIXTURE_TAU
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


def read(path):
    with open(path, "rb") as f:
        return f.read()


@pytest.fixture(scope="module")
def w(tmp_path_factory):
    """the circuit's files, and a .ptau file of the smallest power that holds the powers the circuit's KZG build touches"""
    d = tmp_path_factory.mktemp("ptau_cli")
    mats, vars_, inputs = sm.satisfying_instance(NC, NV, NI, seed=11)
    r1, wt = cm.raw_to_circom(NC, NV, NI, mats, vars_, inputs)
    inst = sm.Instance(NC, NV, NI, mats)
    dense = dm.Dense(inst.nx, inst.ny, inst.mats)
    need = 1 << sem.Shape(inst.nx, inst.ny, dense.N, dense.batch).ell["derefs"]            # npo2(2 batch) N: the derefs polynomial's padded length
    power = 1
    while ptm.counts(power)[0] < need:
        power += 1
    n_g1 = ptm.counts(power)[0]
    xy = ol.g1_mul_gen_batch(b"".join(pem.sb(pow(TAU, i, R_MOD)) for i in range(n_g1)))
    powers = [pm.g1_from_bytes(xy[64 * i:64 * i + 64]) for i in range(n_g1)]
    g2, tau_g2 = srm.g2_from_tau(TAU)
    ptau = ptm.write_ptau(power, TAU, order=(1, 4, 5, 2, 7, 3, 6), powers=powers, g2_real=2)
    paths = {}
    for name, data in (("c.r1cs", r1), ("w.wtns", wt), ("f.ptau", ptau), ("bad.ptau", ptm.replace_g1(ptau, 5, bytes(64)))):
        paths[name] = str(d / name)
        with open(paths[name], "wb") as f:
            f.write(data)
    return dict(dir=d, p=paths, ptau=ptau, power=power, need=need, powers=powers, g2=g2, tau_g2=tau_g2)


def out(w, name):
    return str(w["dir"] / name)


def test_info_prints_the_models_scan(w):
    r = run("info", w["p"]["f.ptau"])
    assert r.returncode == 0, r.stderr
    fields = dict(ln.split(" ", 1) for ln in r.stdout.splitlines())
    s = ptm.scan(w["ptau"])
    assert (fields["power"], fields["ceremonyPower"], fields["n_g1"], fields["n_g2"]) == (str(s["power"]), str(s["ceremony_power"]), str(s["n_g1"]), str(s["n_g2"]))
    assert (fields["off_g1"], fields["off_g2"]) == (str(s["off_g1"]), str(s["off_g2"])) and s["power"] == w["power"]
    cut = out(w, "cut.ptau")
    with open(cut, "wb") as f:
        f.write(w["ptau"][:-1])
    assert run("info", cut).returncode == 2


@pytest.fixture(scope="module")
def srs_file(w):
    r = run("srs", w["p"]["f.ptau"], "-o", out(w, "f.srs"), "--check")
    assert r.returncode == 0, r.stderr
    return out(w, "f.srs")


def test_srs_writes_the_models_reference_format_file(w, srs_file):
    assert read(srs_file) == srm.write_srs(w["powers"], w["tau_g2"], w["g2"])
    r = run("srs", w["p"]["f.ptau"], "-o", out(w, "f9.srs"), "--n", 9)
    assert r.returncode == 0, r.stderr
    assert read(out(w, "f9.srs")) == srm.write_srs(w["powers"][:9], w["tau_g2"], w["g2"])
    assert run("srs", w["p"]["f.ptau"], "-o", out(w, "big.srs"), "--n", len(w["powers"]) + 1).returncode == 2
    assert run("srs", w["p"]["f.ptau"]).returncode == 2                                  # usage: no -o


def test_the_proof_is_the_same_from_either_file_format_and_verifies(w, srs_file):
    hexinit = pem.sb(INIT).hex()
    for name, srs in (("a", w["p"]["f.ptau"]), ("b", srs_file)):
        assert run("encode", w["p"]["c.r1cs"], "-o", out(w, name + ".comm"), "--srs", srs).returncode == 0
        r = run("prove", "--mode", "snark", w["p"]["c.r1cs"], w["p"]["w.wtns"], "-o", out(w, name + ".sbnp"), "--srs", srs, "--tape-init", hexinit)
        assert r.returncode == 0, r.stderr
    assert read(out(w, "a.sbnp")) == read(out(w, "b.sbnp")) and read(out(w, "a.comm")) == read(out(w, "b.comm"))
    for srs in (w["p"]["f.ptau"], srs_file):
        v = run("verify", "--mode", "snark", out(w, "a.comm"), out(w, "a.sbnp"), "--srs", srs)
        assert v.returncode == 0 and "accepted" in v.stdout, v.stderr


def test_a_corrupted_ptau_is_status_2_with_the_index(w):
    for args in (("srs", w["p"]["bad.ptau"], "-o", out(w, "bad.srs")),
                 ("prove", "--mode", "snark", w["p"]["c.r1cs"], w["p"]["w.wtns"], "-o", out(w, "bad.sbnp"), "--srs", w["p"]["bad.ptau"])):
        r = run(*args)
        assert r.returncode == 2 and "power 5:" in r.stderr and "identity" in r.stderr, (r.returncode, r.stderr)
    assert not os.path.exists(out(w, "bad.srs")) and not os.path.exists(out(w, "bad.sbnp"))
