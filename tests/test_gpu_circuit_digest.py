"""GPU: sbn_circom_r1cs_digest — the library's own circuit digest, leaves hashed by k_circom_digest_leaves — against tests/circuit_digest_model.py
(hashlib.shake_256): every leaf count at which the kernel's last block changes shape (k = 16 mod 17 puts the message on 135 mod 136, where the two pad
bits share the rate's last byte), empty matrices, files with permuted sections and with dropped values, two contexts, a context that ran a larger job in
between, and what the digest is for: a NIZK proof made for one circuit is refused against another circuit of the same shape."""
import random

import pytest

import circom_model as cm
import circuit_digest_model as dm
import snark_model as sm

pytestmark = pytest.mark.gpu
R = cm.R_MOD
N_WIRES, N_PUB, N_CONS = 41, 3, 9
SHAPE = dict(n_wires=N_WIRES, n_pub_out=1, n_pub_in=2, n_prv_in=1, n_labels=50)
# entries per matrix (A, B, C).  Every count of {0, 1, 16, 17, 127, 128, 129, 256, 257}; last leaves of k = 33, 50, 67, 84, 101, 118 (with 16: every k on
# the rate's edge); one empty matrix between two others, in front and behind; no entries at all
COUNTS = [(0, 1, 16), (17, 127, 128), (129, 256, 257), (128 + 33, 50, 256 + 67), (84, 128 + 101, 118), (5, 0, 7), (0, 0, 3), (130, 0, 0), (0, 0, 0)]


def circuit(counts, seed, big=()):
    """N_CONS constraints whose matrix m holds counts[m] entries, spread over the rows in order; big: (m, e) whose value is replaced by one >= r"""
    rng = random.Random(seed)
    cons = [([], [], []) for _ in range(N_CONS)]
    for m, n in enumerate(counts):
        for e in range(n):
            v = rng.choice([1, R - 1, rng.randrange(R)])
            if (m, e) in big:
                v = rng.choice([R, R + 1, 2**256 - 1])
            cons[e * N_CONS // n][m].append((rng.randrange(N_WIRES), v))
    return cons


def device_digest(ctx, data):
    f = ctx.circom_r1cs_load(data)
    try:
        return f.digest(), f.info()
    finally:
        f.free()


def test_the_edge_counts_are_what_the_cases_hold():
    assert dm.rate_edge_counts() == {k: 135 for k in (16, 33, 50, 67, 84, 101, 118)}
    last = {n % 128 for c in COUNTS for n in c if n}
    assert set(dm.rate_edge_counts()) <= last and {0, 1, 17, 127} <= last
    assert {0, 1, 16, 17, 127, 128, 129, 256, 257} <= {n for c in COUNTS for n in c}


@pytest.mark.parametrize("counts", COUNTS)
def test_device_digest_is_the_models(ctx, counts):
    data = cm.write_r1cs(SHAPE, circuit(counts, sum(counts) + 1))
    got, info = device_digest(ctx, data)
    assert info["nnz"] == counts
    assert got == dm.digest_of_file(data)


def test_context_method_and_repeat(ctx):
    data = cm.write_r1cs(SHAPE, circuit((129, 16, 33), 3))
    f = ctx.circom_r1cs_load(data)
    try:
        a, b, c = f.digest(), ctx.circom_r1cs_digest(f), f.digest()
    finally:
        f.free()
    assert a == b == c == dm.digest_of_file(data)


def test_permuted_sections_and_dropped_values(ctx):
    counts = (140, 17, 129)
    cons = circuit(counts, 9)
    base = cm.write_r1cs(SHAPE, cons)
    want = dm.digest_of_file(base)
    assert device_digest(ctx, base)[0] == want
    for kw in (dict(section_order=(2, 1)), dict(section_order=(1, 3, 2)), dict(section_order=(9, 2, 1), extra_sections={9: b"\x01\x02\x03"})):
        assert device_digest(ctx, cm.write_r1cs(SHAPE, cons, **kw))[0] == want, kw
    # the same circuit with entries >= r among it: in the first leaf, across the leaf boundary, the last entry
    rng = random.Random(10)
    extra = [tuple(list(run) for run in abc) for abc in cons]
    for i, m, pos in ((0, 0, 0), (3, 0, 2), (8, 0, len(cons[8][0])), (4, 1, 1), (8, 2, len(cons[8][2])), (0, 2, 0)):
        extra[i][m].insert(pos, (rng.randrange(N_WIRES), rng.choice([R, R + 7, 2**256 - 1])))
    data = cm.write_r1cs(SHAPE, extra)
    got, info = device_digest(ctx, data)
    assert info["dropped"] == (3, 1, 2) and info["nnz"] == counts and got == dm.digest_of_file(data) == want
    # and a value that changes is seen: one entry of the last leaf of C
    changed = [tuple(list(run) for run in abc) for abc in cons]
    w, v = changed[8][2][-1]
    changed[8][2][-1] = (w, (v + 1) % R)
    data = cm.write_r1cs(SHAPE, changed)
    assert device_digest(ctx, data)[0] == dm.digest_of_file(data) != want


def test_two_contexts_and_a_larger_job_in_between(ctx, sbn):
    small = cm.write_r1cs(SHAPE, circuit((129, 16, 257), 21))
    large = cm.write_r1cs(dict(SHAPE, n_wires=400, n_labels=500), [([((7 * i + j) % 400, j + 1) for j in range(300)], [(i, 2)], [(i + 1, R - 3)]) for i in range(12)])
    want = dm.digest_of_file(small)
    f = ctx.circom_r1cs_load(small)
    try:
        assert f.digest() == want
        g = ctx.circom_r1cs_load(large)
        try:
            assert g.digest() == dm.digest_of_file(large)
            h = ctx.r1cs_from_circom(g)                                # sorts through the workspace the leaves came back from
            h.free()
        finally:
            g.free()
        assert f.digest() == want
    finally:
        f.free()
    cx = sbn.Context(0)
    try:
        assert device_digest(cx, small)[0] == want
    finally:
        cx.close()


def test_a_nizk_proof_is_bound_to_its_circuit_by_the_digest(ctx, sbn):
    """two satisfied circuits of one shape that differ in one value: with each instance carrying its own device digest, the proof made for the first is
    accepted against the first and refused against the second although the second's matrices accept the same (rx, ry) claim format"""
    nc, nv, ni = 5, 3, 2
    mats, vars_, inputs = sm.satisfying_instance(nc, nv, ni, seed=11)
    r1, wt = cm.raw_to_circom(nc, nv, ni, mats, vars_, inputs)
    A = (mats[0][0], mats[0][1], [(mats[0][2][0] + 1) % R] + mats[0][2][1:])
    r2, _ = cm.raw_to_circom(nc, nv, ni, (A, mats[1], mats[2]), vars_, inputs)
    f1, f2 = ctx.circom_r1cs_load(r1), ctx.circom_r1cs_load(r2)
    hs = []
    try:
        d1, d2 = f1.digest(), f2.digest()
        assert d1 == dm.digest_of_file(r1) and d2 == dm.digest_of_file(r2) and d1 != d2
        i1, i2 = ctx.nizk_instance_from_circom(f1, d1), ctx.nizk_instance_from_circom(f2, d2)
        i2_wrong = ctx.nizk_instance_from_circom(f1, d2)               # the first circuit's matrices under the second's digest
        dg = ctx.nizk_gens_new(nc, nv, ni)
        vt, inp, _ = ctx.circom_wtns_load(wt, ni)
        hs += [i1, i2, i2_wrong, dg, vt]
        tape = sbn.RandomTape(b"proof")
        hs.append(tape)
        proof = ctx.nizk_prove(i1, vt, inp, dg, tape.draw_nizk(i1), sbn.Transcript(b"keyless_snark"), check_sat=True)
        assert ctx.nizk_verify(i1, inp, dg, proof, sbn.Transcript(b"keyless_snark")) is True
        assert ctx.nizk_verify(i2, inp, dg, proof, sbn.Transcript(b"keyless_snark")) is False
        assert ctx.nizk_verify(i2_wrong, inp, dg, proof, sbn.Transcript(b"keyless_snark")) is False      # the digest alone refuses it
    finally:
        for h in reversed(hs):
            h.free()
        f1.free(); f2.free()
