"""CPU: csrc/snark_host.hpp — the shape rules and triplet conversion of Instance::new, R1CSCommitment's bytes, the transcript lines in front of
R1CSProof and the proof's sizes — against tests/snark_model.py and tests/transcript_model.py.  tests/snark_host_check.cpp includes the header alone
and is built with g++ under ASan + UBSan as a stand-alone program, fed one case per line and compared line by line."""
import os
import random
import struct
import subprocess

import pytest

import snark_model as sm
import transcript_model as tm
from conftest import ROOT

R = tm.R_MOD


@pytest.fixture(scope="module")
def check(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("snark_host") / "snark_host_check")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        os.path.join(ROOT, "tests", "snark_host_check.cpp"), "-o", exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr

    def run(cases):
        """cases: [[word, ...]] (bytes go as hex, integers as decimal) -> the words of each case's result line"""
        def word(w):
            return str(w) if isinstance(w, (int, str)) else (bytes(w).hex() or "-")
        text = "".join(" ".join(word(w) for w in case) + "\n" for case in cases)
        r = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
        lines = r.stdout.splitlines()
        assert lines[-1] == "SNARK HOST CHECK DONE" and len(lines) == len(cases) + 1
        return [ln.split() for ln in lines[:-1]]
    return run


def u32s(xs):
    return struct.pack("<%dI" % len(xs), *xs)


def le32(xs):
    return b"".join(int(x).to_bytes(32, "little") for x in xs)


def fake_points(n, seed):
    """n strings of 32 bytes that stand for compressed points (the header never decompresses one); every fifth is an identity with stray x bits"""
    rng = random.Random(seed)
    out = []
    for i in range(n):
        b = bytearray(rng.randbytes(32)); b[31] &= 0xbf
        if i % 5 == 4:
            b[31] |= 0x40
        out.append(bytes(b))
    return out


def normal(p):
    return bytes(31) + b"\x40" if p[31] & 0x40 else p


def comm_case(shape, N, seed=0):
    """(the header words, L_ops, L_mem, ops points, mem points, the bytes the model writes)"""
    nc, nv, nx, ny = sm.pad_shape(*shape)
    Lo, Lm = sm.comm_lens(nc, nv, N)
    ops, mem = fake_points(Lo, seed), fake_points(Lm, seed + 1)
    head = b"".join(x.to_bytes(8, "little") for x in (nc, nv, shape[2], 3, N, 1 << max(nx, ny)))
    return (nc, nv, shape[2], 3, N, 1 << max(nx, ny)), Lo, Lm, ops, mem, head + b"".join(normal(p) for p in ops + mem)


def test_shape_rules_over_every_small_shape(check):
    shapes = [(a, b, c) for a in range(1, 10) for b in range(1, 10) for c in range(0, 10)]
    got = check([["shape", *s] for s in shapes])
    for s, g in zip(shapes, got):
        assert [int(x) for x in g] == list(sm.pad_shape(*s)), s
    assert len(shapes) == 810
    big = check([["shape", (1 << 29) + 1, 1, 0], ["shape", 1, (1 << 29) + 1, 0], ["shape", 1, 1, 1 << 29], ["shape", 1 << 29, 1 << 29, (1 << 29) - 1], ["shape", 0, 0, 0]])
    assert big[:3] == [["refused"]] * 3 and [int(x) for x in big[3]] == [1 << 29, 1 << 29, 29, 30] and [int(x) for x in big[4]] == [2, 1, 1, 1]


def test_column_shift_and_its_three_errors(check):
    rng = random.Random(7)
    cases, want = [], []
    for shape in [(5, 3, 2), (4, 4, 1), (2, 1, 3), (1, 2, 0), (40, 4, 2), (2, 40, 5), (9, 9, 9)]:
        nc, nv, ni = shape
        live = nv + 1 + ni
        for nnz in (0, 1, 7, 64):
            rows = [rng.randrange(nc) for _ in range(nnz)]
            cols = [rng.randrange(live) for _ in range(nnz)]
            if nnz >= 7:
                cols[:4] = [nv - 1, nv, nv + ni, 0][:4]            # the last variable, the constant, the last input
            vals = [rng.choice([0, 1, R - 1, rng.randrange(R)]) for _ in range(nnz)]
            cases.append(["convert", *shape, u32s(rows), u32s(cols), le32(vals)])
            inst = sm.Instance(*shape, [(rows, cols, vals)])
            want.append(["0", str(max(nnz - 1, 0)), u32s(inst.mats[0][1]).hex() or "-"])
            if nnz == 7:
                for at, (r, c, v), code in ((3, (nc, 0, 1), 1), (0, (0, live, 1), 2), (6, (0, 0, R), 3), (2, (nc, live, R), 1), (5, (0, live, R), 2),
                                            (4, (0, 0, (1 << 256) - 1), 3)):
                    r2, c2, v2 = list(rows), list(cols), list(vals)
                    r2[at], c2[at], v2[at] = r, c, v
                    cases.append(["convert", *shape, u32s(r2), u32s(c2), le32(v2)])
                    want.append([str(code), str(at), "-"])
                    with pytest.raises(sm.InstanceError) as e:
                        sm.Instance(*shape, [(r2, c2, v2)])
                    assert e.value.args[0] == {1: "row", 2: "col", 3: "val"}[code]
    assert check(cases) == want


@pytest.mark.parametrize("shape,N", [((5, 3, 2), 16), ((4, 4, 1), 2), ((40, 4, 2), 128), ((2, 40, 5), 8), ((1, 2, 0), 4)])
def test_commitment_bytes_round_trip(check, shape, N):
    head, Lo, Lm, ops, mem, want = comm_case(shape, N)
    built, parsed, short = check([["build", *shape, N, b"".join(ops), b"".join(mem)], ["parse", want], ["build", *shape, N, b"".join(ops[:-1]), b"".join(mem)]])
    assert built == [want.hex()]
    assert [int(x) for x in parsed] == [0, *head, Lo, Lm]
    assert short == ["lengths", str(Lo), str(Lm)]
    # the model reads the same numbers out of the same bytes (its points are real ones: only the header is compared)
    assert [int.from_bytes(want[8 * k:8 * k + 8], "little") for k in range(6)] == list(head)


def test_commitment_bytes_are_refused_field_by_field(check):
    head, Lo, Lm, ops, mem, good = comm_case((5, 3, 2), 16)

    def with_field(k, v):
        b = bytearray(good); b[8 * k:8 * k + 8] = (v % (1 << 64)).to_bytes(8, "little")
        return bytes(b)
    SHORT, CONS, VARS, INPUTS, BATCH, OPS, CELLS, LENGTH = range(1, 9)
    trials = [(good[:47], SHORT), (b"", SHORT), (good[:48], LENGTH), (good[:-1], LENGTH), (good + b"\0", LENGTH), (good[:-32], LENGTH), (good + bytes(32), LENGTH),
              (with_field(0, 0), CONS), (with_field(0, 1), CONS), (with_field(0, 6), CONS), (with_field(0, 1 << 30), CONS), (with_field(0, -1), CONS),
              (with_field(1, 0), VARS), (with_field(1, 3), VARS), (with_field(1, 1 << 63), VARS),
              (with_field(2, 4), INPUTS), (with_field(2, 5), INPUTS), (with_field(2, -1), INPUTS),
              (with_field(3, 2), BATCH), (with_field(3, 0), BATCH), (with_field(3, 4), BATCH),
              (with_field(4, 0), OPS), (with_field(4, 1), OPS), (with_field(4, 12), OPS), (with_field(4, 1 << 32), OPS),
              (with_field(5, 4), CELLS), (with_field(5, 16), CELLS), (with_field(5, 0), CELLS),
              (with_field(0, 16), CELLS),                         # a larger num_cons: the cells no longer fit
              (with_field(4, 64), LENGTH), (with_field(1, 2), INPUTS)]
    got = check([["parse", b] for b, _ in trials])
    for (b, code), g in zip(trials, got):
        assert g == [str(code)], (b[:48].hex(), code)
    assert check([["parse", good]])[0][0] == "0"


@pytest.mark.parametrize("shape,N", [((5, 3, 2), 16), ((4, 4, 1), 2), ((2, 40, 5), 8)])
def test_prefix_state_after_every_line(check, shape, N):
    head, Lo, Lm, ops, mem, good = comm_case(shape, N, seed=3)
    label = b"snark host"
    t = tm.Transcript(label)
    want = []

    def line(lab, msg):
        t.append_message(lab, msg); want.append(t.state().hex())
    line(b"protocol-name", b"Spartan SNARK proof")
    for lab, x in zip((b"num_cons", b"num_vars", b"num_inputs", b"batch_size", b"num_ops", b"num_mem_cells"), head):
        line(lab, x.to_bytes(8, "little"))
    for lab, pts in ((b"comm_comb_ops", ops), (b"comm_comb_mem", mem)):
        line(lab, b"poly_commitment_begin")
        for p in pts:
            line(b"poly_commitment_share", normal(p))
        line(lab, b"poly_commitment_end")
    # the same lines on bytes whose identities carry stray x bits: the prefix absorbs the normalised form
    raw = good[:48] + b"".join(ops + mem)
    got, got_raw = check([["prefix", label, good], ["prefix", label, raw]])
    assert got == want and got_raw == want and len(want) == 7 + 4 + Lo + Lm


def test_sizes_are_the_two_halves_laid_end_to_end(check):
    cases, want = [], []
    for shape, N in [((5, 3, 2), 16), ((4, 4, 1), 2), ((40, 4, 2), 128), ((2, 40, 5), 8), ((1, 2, 0), 4), ((1000, 900, 30), 4096)]:
        head, Lo, Lm, ops, mem, good = comm_case(shape, N)
        comm = dict(nc=head[0], nv=head[1], ni=head[2], batch=3, N=N, cells=head[5])
        for kzg in (0, 1):
            cases.append(["sizes", good, kzg])
            a = sm.rpm.sizes(comm["nc"], comm["nv"])
            b = (sm.skm if kzg else sm.sem).sizes(sm.log2(comm["nc"]), sm.log2(2 * comm["nv"]), N, 3)
            assert (a[0] + b[0], a[1] + 96 + b[1]) == sm.sizes(comm, bool(kzg))
            want.append([str(x) for x in (a[0], a[1], b[0], b[1], a[0] + b[0], a[1] + 96 + b[1])])
    assert check(cases) == want
