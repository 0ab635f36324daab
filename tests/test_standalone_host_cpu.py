"""CPU: harness/standalone_host.hpp — the proof file of sbn_spartan — against tests/proof_file_model.py.  tests/standalone_host_check.cpp includes the header
alone and is built with g++ under ASan + UBSan as a stand-alone program; each file is copied into a buffer of exactly its length."""
import os
import subprocess

import pytest

import proof_file_model as pfm
from conftest import ROOT
from transcript_model import R_MOD

DIGEST = bytes(range(1, 33))
PROOF = bytes(range(200, 256)) * 3
SMALL = dict(mode=pfm.NIZK, kzg=0, num_cons=5, num_vars=3, num_nz=11, digest=DIGEST, inputs=[7, R_MOD - 1], proof=PROOF)


@pytest.fixture(scope="module")
def check(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("standalone_host") / "standalone_host_check")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        os.path.join(ROOT, "tests", "standalone_host_check.cpp"), "-o", exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr

    def run(cases):
        """cases: [(file, want_mode, want_kzg)] -> the words of each result line"""
        text = "".join(f"{bytes(f).hex() or '-'} {m} {k}\n" for f, m, k in cases)
        r = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]                # a sanitizer report ends the program with another status
        lines = r.stdout.splitlines()
        assert lines[-1] == "STANDALONE HOST CHECK DONE" and len(lines) == len(cases) + 1
        return [ln.split() for ln in lines[:-1]]
    return run


def model_line(data, want_mode=-1, want_kzg=-1):
    try:
        f = pfm.read(data, want_mode, want_kzg)
    except pfm.ProofFileError as e:
        return ["refused", e.args[0]]
    hx = lambda b: b.hex() or "-"                                                    # noqa: E731
    return ["ok", str(f["mode"]), str(f["kzg"]), str(f["num_cons"]), str(f["num_vars"]), str(f["num_inputs"]), str(f["num_nz"]), hx(f["digest"]), hx(f["inputs"]),
            hx(f["proof"]), "same"]


def test_read_of_write(check):
    files = [pfm.write(**SMALL), pfm.write(**dict(SMALL, mode=pfm.SNARK, kzg=1, digest=b"")), pfm.write(**dict(SMALL, mode=pfm.SNARK, inputs=[], proof=b"")),
             pfm.write(**dict(SMALL, digest=bytes(300), num_cons=(1 << 64) - 1, num_nz=1 << 63))]
    got = check([(f, -1, -1) for f in files] + [(files[0], pfm.NIZK, 0), (files[1], pfm.SNARK, 1)])
    for (f, m, k), g in zip([(f, -1, -1) for f in files] + [(files[0], pfm.NIZK, 0), (files[1], pfm.SNARK, 1)], got):
        want = model_line(f, m, k)
        assert want[0] == "ok" and g == want
    assert pfm.read(files[0])["inputs"] == (7).to_bytes(32, "little") + (R_MOD - 1).to_bytes(32, "little") and pfm.read(files[0])["proof"] == PROOF


def test_every_prefix_is_refused(check):
    data = pfm.write(**SMALL)
    prefixes = [data[:n] for n in range(len(data))]
    got = check([(p, -1, -1) for p in prefixes])
    for n, (p, g) in enumerate(zip(prefixes, got)):
        assert g[0] == "refused" and g == model_line(p), n
    assert {g[1] for g in got} == {"short", "length"}


def test_lengths_that_overflow_or_pass_the_end(check):
    big = [1 << 61, (1 << 64) - 1, 1 << 59, (1 << 64) // 32, (1 << 64) // 32 + 1, len(PROOF) + 1]
    cases = [pfm.write(**dict(SMALL, proof_len=n)) for n in big]
    cases += [pfm.write(**dict(SMALL, num_inputs=n)) for n in big]                    # 2^59 * 32 wraps to 0, 2^64 / 32 * 32 to 0 as well
    cases += [pfm.write(**dict(SMALL, digest_len=n)) for n in ((1 << 32) - 1, len(DIGEST) + 64 + 8 + len(PROOF) + 1)]
    got = check([(f, -1, -1) for f in cases])
    for f, g in zip(cases, got):
        assert g == model_line(f) == ["refused", "length"], g
    # a digest length that swallows the rest exactly: the inputs then pass the end
    f = pfm.write(**dict(SMALL, digest_len=len(DIGEST) + 64 + 8 + len(PROOF)))
    assert check([(f, -1, -1)])[0] == model_line(f) and model_line(f)[0] == "refused"


def test_trailing_bytes_inputs_and_each_contradiction(check):
    ok = pfm.write(**SMALL)
    snark_kzg = pfm.write(**dict(SMALL, mode=pfm.SNARK, kzg=1))
    cases = [("trailing", ok + b"\0", -1, -1), ("trailing", ok + ok, -1, -1),
             ("input", pfm.write(**dict(SMALL, inputs=[7, R_MOD])), -1, -1), ("input", pfm.write(**dict(SMALL, inputs=[(1 << 256) - 1, 1])), -1, -1),
             ("magic", pfm.write(**dict(SMALL, magic=b"SBNQ")), -1, -1), ("version", pfm.write(**dict(SMALL, version=2)), -1, -1), ("version", pfm.write(**dict(SMALL, version=0)), -1, -1),
             ("mode", pfm.write(**dict(SMALL, mode=2)), -1, -1), ("kzg", pfm.write(**dict(SMALL, mode=pfm.SNARK, kzg=2)), -1, -1), ("kzg", pfm.write(**dict(SMALL, kzg=1)), -1, -1),
             ("reserved", pfm.write(**dict(SMALL, reserved=1)), -1, -1), ("reserved", pfm.write(**dict(SMALL, reserved=0x100)), -1, -1),
             ("mode_mismatch", ok, pfm.SNARK, -1), ("mode_mismatch", snark_kzg, pfm.NIZK, -1), ("kzg_mismatch", snark_kzg, pfm.SNARK, 0), ("kzg_mismatch", ok, pfm.NIZK, 1),
             ("short", b"", -1, -1), ("short", b"SBN", -1, -1)]
    got = check([(f, m, k) for _, f, m, k in cases])
    for (why, f, m, k), g in zip(cases, got):
        assert g == ["refused", why] == model_line(f, m, k), (why, g)
