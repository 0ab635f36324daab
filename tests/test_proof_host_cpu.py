"""CPU: the provers' transcript script (csrc/proof_host.hpp: Script, transcript_wide_reduce, fr::fmul) against tests/transcript_model.py and plain
integers.  tests/proof_host_check.cpp includes the header alone and is built with g++ under ASan + UBSan as a stand-alone program, fed one case per
line and compared line by line; the whole 203-byte transcript state is compared after every operation."""
import os
import random
import subprocess

import pytest

import transcript_model as tm
from conftest import ROOT

R = tm.R_MOD
Q = 21888242871839275222246405745257275088696311157297823662689037894645226208583      # BN254's base field


@pytest.fixture(scope="module")
def check(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("proof_host") / "proof_host_check")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        os.path.join(ROOT, "tests", "proof_host_check.cpp"), "-o", exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr

    def run(cases):
        """cases: [[word, ...]] (bytes go as hex, integers as decimal counts) -> the words of each case's result line"""
        def word(w):
            return str(w) if isinstance(w, (int, str)) else (bytes(w).hex() or "-")
        text = "".join(" ".join(word(w) for w in case) + "\n" for case in cases)
        r = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
        lines = r.stdout.splitlines()
        assert lines[-1] == "PROOF HOST CHECK DONE" and len(lines) == len(cases) + 1
        return [ln.split() for ln in lines[:-1]]
    return run


def le32(x):
    return int(x).to_bytes(32, "little")


def compress(x, y):
    """serialize_compressed of an affine point: x, bit 255 set when y > q - y; the identity (0, 0) is the infinity flag alone"""
    if x == 0 and y == 0:
        return (1 << 254).to_bytes(32, "little")
    return (x | (1 << 255 if 2 * y > Q else 0)).to_bytes(32, "little")


def run_script(check, label, ops):
    """ops: [(name, args..)] -> checks every state (and output) against the model applying `ops` to Transcript(label)"""
    words, want = ["script", label], []
    t = tm.Transcript(label)
    for op in ops:
        name, args = op[0], op[1:]
        out = None
        if name == "protocol":
            t.append_message(b"protocol-name", args[0])
        elif name in ("scalar", "point", "message"):
            t.append_message(args[0], args[1])
        elif name == "scalars":
            lab, vals = args
            for v in vals:
                t.append_message(lab, le32(v))
            args = (lab, b"".join(le32(v) for v in vals), len(vals))
        elif name == "point_xy":
            lab, x, y = args
            out = compress(x, y)
            t.append_message(lab, out)
            args = (lab, le32(x) + le32(y))
        elif name == "challenge":
            out = le32(t.challenge_scalar(args[0]))
        elif name == "challenges":
            out = b"".join(le32(t.challenge_scalar(args[0])) for _ in range(args[1]))
        else:
            raise ValueError(name)
        words += [name, *args]
        want.append(((out.hex() or "-") + ":" if out is not None else "") + t.state().hex())
    got = check([words])[0]
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, (label, ops[i][0], i)


def test_every_operation_against_the_model(check):
    rng = random.Random(1)
    sc = [rng.randrange(R) for _ in range(5)]
    run_script(check, b"test", [
        ("protocol", b"R1CS proof"),
        ("scalar", b"input", le32(sc[0])),
        ("scalars", b"a", sc),
        ("point", b"comm_poly", le32(rng.randrange(1 << 256))),
        ("point_xy", b"Cx", rng.randrange(Q), rng.randrange(Q)),
        ("message", b"poly_commitment", b"poly_commitment_begin"),
        ("challenge", b"challenge_nextround"),
        ("challenges", b"challenge_tau", 3),
        ("scalar", b"claim", le32(R - 1)),
        ("challenge", b"c"),
    ])


def test_label_lengths_zero_and_one(check):
    for lab in (b"", b"a"):
        run_script(check, lab, [("scalar", lab, le32(7)), ("point", lab, le32(9)), ("message", lab, b"xyz"), ("scalars", lab, [1, 2]),
                                ("point_xy", lab, 1, 2), ("challenge", lab), ("challenges", lab, 2), ("scalar", lab, le32(0))])


def test_scalars_of_zero_one_and_five(check):
    rng = random.Random(2)
    for n in (0, 1, 5):
        run_script(check, b"slice", [("scalars", b"a", [rng.randrange(R) for _ in range(n)]), ("challenge", b"r")])
    run_script(check, b"slice", [("challenges", b"u", 0), ("challenge", b"r")])


@pytest.mark.parametrize("n", [0, 165, 166, 167])
def test_message_at_the_rate_edge(check, n):
    msg = bytes((i * 7 + 1) & 255 for i in range(n))
    run_script(check, b"edge", [("message", b"m", msg), ("challenge", b"c"), ("message", b"", msg), ("message", b"m", msg), ("challenge", b"c")])


def test_protocol_is_a_message_under_protocol_name(check):
    for name in (b"x", b"polynomial evaluation proof", b"Sparse polynomial evaluation proof"):
        a = check([["script", b"p", "protocol", name, "challenge", b"c"]])[0]
        b = check([["script", b"p", "message", b"protocol-name", name, "challenge", b"c"]])[0]
        assert a == b
        run_script(check, b"p", [("protocol", name), ("challenge", b"c")])


def test_compressed_points_at_the_sign_edge(check):
    # the identity, y just below and just above q / 2 (2 y > q sets the sign bit), the largest y, x with its top bits in use
    pts = [(0, 0), (5, (Q - 1) // 2), (5, (Q + 1) // 2), (1, 1), (Q - 1, Q - 1), (0, 1), (1, 0)]
    run_script(check, b"pts", [("point_xy", b"P", x, y) for x, y in pts])


def test_wide_reduce(check):
    rng = random.Random(3)
    M = 1 << 256
    vals = [M * M - 1, 0, R - 1, R, M - 1, M, M + R, (R - 1) * M + R - 1, (M - 1) * M, 1, R + 1, 2 * R, 5 * R, 6 * R - 1 if 6 * R - 1 < M else M - 1]
    vals += [rng.randrange(M * M) for _ in range(300)]
    vals += [rng.randrange(M) for _ in range(20)] + [rng.randrange(M) * M for _ in range(20)]
    got = check([["wide", v.to_bytes(64, "little")] for v in vals])
    for v, (g,) in zip(vals, got):
        assert g == le32(int.from_bytes(v.to_bytes(64, "little"), "little") % R).hex(), hex(v)


def test_fmul(check):
    rng = random.Random(4)
    edge = [0, 1, R - 1, 2, R - 2, (R - 1) // 2, (R + 1) // 2]
    pairs = [(a, b) for a in edge for b in edge] + [(rng.randrange(R), rng.randrange(R)) for _ in range(300)]
    got = check([["fmul", le32(a), le32(b)] for a, b in pairs])
    for (a, b), (g,) in zip(pairs, got):
        assert g == le32(a * b % R).hex(), (a, b)
