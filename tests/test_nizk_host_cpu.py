"""CPU: what NIZK mode adds to csrc/snark_host.hpp — the two transcript lines in front of R1CSProof and the proof's sizes — against tests/nizk_model.py
and tests/transcript_model.py.  tests/nizk_host_check.cpp includes the header alone and is built with g++ under ASan + UBSan as a stand-alone program,
fed one case per line and compared line by line."""
import os
import subprocess

import pytest

import nizk_model as nm
import transcript_model as tm
from conftest import ROOT


@pytest.fixture(scope="module")
def check(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("nizk_host") / "nizk_host_check")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        os.path.join(ROOT, "tests", "nizk_host_check.cpp"), "-o", exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr

    def run(cases):
        """cases: [[word, ...]] (bytes go as hex, integers as decimal) -> the words of each case's result line"""
        def word(w):
            return str(w) if isinstance(w, (int, str)) else (bytes(w).hex() or "-")
        text = "".join(" ".join(word(w) for w in case) + "\n" for case in cases)
        r = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
        lines = r.stdout.splitlines()
        assert lines[-1] == "NIZK HOST CHECK DONE" and len(lines) == len(cases) + 1
        return [ln.split() for ln in lines[:-1]]
    return run


# no bytes (NULL); one byte; a digest as long as a hash; the last length that stays inside STROBE's 166-byte rate behind the message's own framing, the
# first that crosses it, and one that crosses it well inside one message; more than two blocks
DIGEST_LENGTHS = [0, 1, 32, 100, 120, 140, 165, 166, 167, 200, 400]


def test_prefix_state_after_each_of_the_two_lines(check):
    label = b"nizk host"
    digests = [bytes((7 * i + n) & 0xff for i in range(n)) for n in DIGEST_LENGTHS]
    got = check([["prefix", label, d] for d in digests])
    for d, g in zip(digests, got):
        t = tm.Transcript(label)
        t.append_message(b"protocol-name", b"Spartan NIZK proof")
        first = t.state().hex()
        t.append_message(b"R1CSShapeDigest", d)
        assert g == [first, t.state().hex()], len(d)
        m = tm.Transcript(label)
        nm.append_prefix(m, d)
        assert m.state() == t.state()
    assert len({g[1] for g in got}) == len(digests)


def test_sizes_are_the_r1cs_proof_and_the_claimed_point(check):
    shapes = [k[:3] for k in nm.KEYS] + [(2, 2, 0), (1, 1, 0), (9, 9, 9), (1000, 900, 30), (1 << 20, 1 << 20, 10)]
    got = check([["sizes", *s] for s in shapes])
    for s, g in zip(shapes, got):
        nc, nv, nx, ny = nm.pad_shape(*s)
        if nv < 2:                                                  # no variable to open: the model has no sizes here, the header still counts
            continue
        inst = nm.Instance(*s, (([], [], []),) * 3)
        a = nm.rpm.sizes(nc, nv)
        assert [int(x) for x in g] == [a[1], a[0], a[1] + 32 * (nx + ny)] and (a[0], a[1] + 32 * (nx + ny)) == nm.sizes(inst), s
    assert check([["sizes", (1 << 29) + 1, 1, 0]]) == [["refused"]]
