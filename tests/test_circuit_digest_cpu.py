"""CPU: the circuit digest's definition (tests/circuit_digest_model.py over hashlib.shake_256): what it binds and what it does not.  It is defined over
what sbn_circom_r1cs_download returns, so it changes with a row, a column, a value, a shape field, the matrix an entry sits in and the order of two
entries, and does not change under another section order or a dropped (>= r) entry.  tests/test_gpu_circuit_digest.py holds the device against it.
The first four tests are about the MODEL alone (they pin the definition against hashlib and pass whatever the library does); only the last one,
test_host_leaf_and_root_are_the_models, runs library code: the host functions of csrc/circom_host.hpp."""
import hashlib
import os
import random
import subprocess

import circom_model as cm
import circuit_digest_model as dm
from conftest import ROOT

R = cm.R_MOD
SHAPE = dict(n_wires=9, n_pub_out=1, n_pub_in=2, n_prv_in=1, n_labels=11)
CONS = [([(4, 1), (0, R - 1)], [(5, 2)], [(6, 3)]), ([(1, 5)], [(2, 6), (3, 7), (0, 8)], [(0, 9)]), ([(7, 11)], [(8, 12)], [(4, 13), (5, 14)])]


def edit(cons, i, m, e, wire=None, val=None):
    out = [tuple(list(run) for run in abc) for abc in cons]
    w, v = out[i][m][e]
    out[i][m][e] = (w if wire is None else wire, v if val is None else val)
    return out


def test_the_definition_written_out_once():
    mats = ([(0, 5, 7)], [], [(1, 2, R - 1), (1, 3, 4)])
    shape5 = (2, 9, 3, 2, 8)
    leaf_a = hashlib.shake_256(b"sbn254/r1cs-digest/leaf/v1" + bytes([0]) + bytes(8) + (1).to_bytes(4, "little") +
                               (0).to_bytes(4, "little") + (5).to_bytes(4, "little") + (7).to_bytes(32, "little")).digest(32)
    leaf_c = hashlib.shake_256(b"sbn254/r1cs-digest/leaf/v1" + bytes([2]) + bytes(8) + (2).to_bytes(4, "little") +
                               (1).to_bytes(4, "little") + (2).to_bytes(4, "little") + (R - 1).to_bytes(32, "little") +
                               (1).to_bytes(4, "little") + (3).to_bytes(4, "little") + (4).to_bytes(32, "little")).digest(32)
    root = hashlib.shake_256(b"sbn254/r1cs-digest/root/v1" + b"".join(x.to_bytes(8, "little") for x in shape5) +
                             (1).to_bytes(8, "little") + leaf_a + (0).to_bytes(8, "little") + (2).to_bytes(8, "little") + leaf_c).digest(32)
    assert dm.digest(shape5, mats) == root
    assert len(dm.leaf_message(2, 0, mats[2])) == 39 + 40 * 2


def test_what_changes_the_digest():
    base = dm.digest_of_file(cm.write_r1cs(SHAPE, CONS))
    seen = {base}

    def differs(data, what):
        d = dm.digest_of_file(data)
        assert d not in seen, what
        seen.add(d)
    differs(cm.write_r1cs(SHAPE, edit(CONS, 1, 1, 1, val=8)), "a value")
    differs(cm.write_r1cs(SHAPE, edit(CONS, 1, 1, 1, wire=4)), "a column")
    differs(cm.write_r1cs(SHAPE, edit(CONS, 2, 2, 0, wire=0)), "a column onto the constant")
    moved_row = [CONS[0], (CONS[1][0], CONS[1][1][:2], CONS[1][2]), (CONS[2][0], [CONS[1][1][2]] + CONS[2][1], CONS[2][2])]
    differs(cm.write_r1cs(SHAPE, moved_row), "the row of an entry")
    moved_mat = [CONS[0], (CONS[1][0] + [CONS[1][1][2]], CONS[1][1][:2], CONS[1][2]), CONS[2]]
    differs(cm.write_r1cs(SHAPE, moved_mat), "the matrix an entry sits in")
    swapped = [CONS[0], (CONS[1][0], [CONS[1][1][1], CONS[1][1][0], CONS[1][1][2]], CONS[1][2]), CONS[2]]
    differs(cm.write_r1cs(SHAPE, swapped), "the order of two entries")
    differs(cm.write_r1cs(dict(SHAPE, n_wires=10), CONS), "num_variables")
    differs(cm.write_r1cs(dict(SHAPE, n_pub_in=1), CONS), "num_pub_inputs (and with it the remapped columns)")
    differs(cm.write_r1cs(SHAPE, CONS + [([], [], [])]), "num_constraints, with no entry more")
    differs(cm.write_r1cs(SHAPE, CONS[:2]), "a constraint less")
    # the padded shape alone: 5 constraints pad to 8 as 6 do, 4 do not
    five, six = CONS + [([], [], [])] * 2, CONS + [([], [], [])] * 3
    assert dm.digest_of_file(cm.write_r1cs(SHAPE, five)) != dm.digest_of_file(cm.write_r1cs(SHAPE, six))
    mats = cm.to_sparse_matrices_padded(cm.read_r1cs(cm.write_r1cs(SHAPE, CONS)), 8)
    assert dm.digest((3, 9, 3, 4, 8), mats) == base != dm.digest((3, 9, 3, 8, 8), mats) != dm.digest((3, 9, 3, 4, 16), mats)


def test_what_does_not_change_it():
    base = dm.digest_of_file(cm.write_r1cs(SHAPE, CONS))
    for kw in (dict(section_order=(2, 1)), dict(section_order=(1, 3, 2)), dict(section_order=(9, 1, 2), extra_sections={9: b"\x01\x02\x03"}),
               dict(section_order=(2, 77, 1, 3), extra_sections={77: b"\xaa" * 10})):
        assert dm.digest_of_file(cm.write_r1cs(SHAPE, CONS, **kw)) == base, kw
    assert dm.digest_of_file(cm.write_r1cs(dict(SHAPE, n_labels=99, n_prv_in=3), CONS)) == base            # fields no prover or verifier reads
    # an entry whose value is >= r is dropped by the reader: the file with it and the file without it are one circuit
    with_dropped = [(CONS[0][0] + [(3, R)], CONS[0][1], [(2, R + 5)] + CONS[0][2]), CONS[1], (CONS[2][0], CONS[2][1] + [(1, (1 << 256) - 1)], CONS[2][2])]
    r = cm.read_r1cs(cm.write_r1cs(SHAPE, with_dropped))
    assert r["dropped"] == [1, 1, 1] and dm.digest_of_file(cm.write_r1cs(SHAPE, with_dropped)) == base


def test_leaf_boundaries_and_the_rate_edges():
    """a leaf holds 128 entries; the leaf index and the count are hashed, so cutting the same entries otherwise gives another digest"""
    ents = [(i, i % 7, i + 1) for i in range(300)]
    assert len(dm.leaves(0, ents)) == 3 and len(dm.leaves(1, ents[:128])) == 1 and len(dm.leaves(1, ents[:129])) == 2 and dm.leaves(2, []) == []
    assert dm.leaves(0, ents)[1] == dm.leaf(0, 1, ents[128:256]) != dm.leaf(0, 0, ents[128:256]) != dm.leaf(1, 1, ents[128:256])
    # k = 16 puts a leaf's length on 135 mod 136, where the two pad bits share a byte; so does every k = 16 mod 17; no k ends a block exactly
    edges = dm.rate_edge_counts()
    assert edges == {k: 135 for k in range(16, 129, 17)} and len(dm.leaf_message(0, 0, ents[:16])) == 679 == 5 * 136 - 1
    shape5 = (300, 9, 3, 512, 8)
    assert dm.digest(shape5, (ents, [], ents[:16])) != dm.digest(shape5, (ents, ents[:16], []))              # which matrix is the empty one


# ---- the host half of the library (csrc/circom_host.hpp) alone, under ASan + UBSan --------------------------------------------

def test_host_leaf_and_root_are_the_models(tmp_path):
    """tests/circuit_digest_check.cpp: digest_leaf is the function the device computes, digest_root what sbn_circom_r1cs_digest runs over the leaves"""
    exe = str(tmp_path / "circuit_digest_check")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        os.path.join(ROOT, "tests", "circuit_digest_check.cpp"), "-o", exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    rng = random.Random(4)
    cases = []
    for counts in ((0, 0, 0), (1, 0, 16), (17, 127, 128), (129, 0, 257), (33, 50, 67)):
        mats = tuple([(rng.randrange(1 << 32), rng.randrange(1 << 32), rng.choice([0, 1, R - 1, rng.randrange(R)])) for _ in range(n)] for n in counts)
        cases.append(((rng.randrange(1 << 40), rng.randrange(1 << 33), 3, 1 << 20, (1 << 64) - 1), mats))
    text = ""
    for shape5, mats in cases:
        ents = "".join((r_.to_bytes(4, "little") + c.to_bytes(4, "little") + v.to_bytes(32, "little")).hex() for m in mats for r_, c, v in m)
        text += " ".join(map(str, shape5)) + " " + " ".join(str(len(m)) for m in mats) + " " + (ents or "-") + "\n"
    r = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]                      # a sanitizer report ends the program with another status
    lines = r.stdout.splitlines()
    assert lines[-1] == "CIRCUIT DIGEST CHECK DONE" and len(lines) == len(cases) + 1
    for (shape5, mats), ln in zip(cases, lines):
        root, leaves = ln.split()
        want = b"".join(b"".join(dm.leaves(m, mat)) for m, mat in enumerate(mats))
        assert (bytes.fromhex(leaves) if leaves != "-" else b"") == want
        assert bytes.fromhex(root) == dm.digest(shape5, mats)
