"""CPU: the prover's RandomTape and the draw plans behind the C ABI (sbn_random_tape_*, sbn_*_draw_rnd; no context, no device) and their host header
alone (csrc/random_tape_host.hpp through tests/random_tape_check.cpp, a stand-alone program under ASan + UBSan), both against the literal model of
tests/random_tape_model.py on transcript_model.Transcript.  The snark and nizk plans take resident handles: tests/test_gpu_random_tape_prove.py has them."""
import ctypes as C
import os
import subprocess

import pytest

import polyeval_model as pm
import r1cs_proof_model as rpm
import random_tape_model as rtm
import sparse_eval_kzg_model as skm
import sparse_eval_model as sem
from conftest import ROOT
from transcript_model import R_MOD

INIT = 0x1234567890abcdef1122334455667788 * 0x10001 % R_MOD
SMALL = (2, 2)                                                        # the smallest legal shape: num_cons = num_vars = 2 (L = 1, lg = 1)
WIDE = (8, 64)                                                        # ell = 6: L = 8 > 1, lg = 3 >= 2


def ib(x):
    return int(x).to_bytes(32, "little")


def model(name, init=INIT):
    return rtm.RandomTape(name, init)


def scalars(b):
    return [int.from_bytes(b[i:i + 32], "little") for i in range(0, len(b), 32)]


# ---- through the C ABI ------------------------------------------------------------------------------------------------------------

def test_raw_draws_labels_empty_label_and_zero_count(sbn):
    t, m = sbn.RandomTape(b"proof", ib(INIT)), model(b"proof")
    try:
        for label, n in ((b"d", 1), (b"blinds_vec_1", 5), (b"", 2), (b"x" * 200, 1), (b"d", 0), (b"", 0), (b"r", 3)):      # a label longer than STROBE's rate too
            got = t.scalars(label, n)
            assert len(got) == 32 * n and scalars(got) == m.random_vector(label, n), label
    finally:
        t.free()
    # the name is part of the tape: another name, other draws; the empty name is legal
    a, b = sbn.RandomTape(b"snark_proof", ib(INIT)), sbn.RandomTape(b"", ib(INIT))
    try:
        assert scalars(a.scalars(b"d", 2)) == model(b"snark_proof").random_vector(b"d", 2) != model(b"proof").random_vector(b"d", 2)
        assert scalars(b.scalars(b"d", 2)) == model(b"").random_vector(b"d", 2)
    finally:
        a.free(); b.free()


@pytest.mark.parametrize("init", [0, 1, R_MOD - 1])
def test_init_at_the_ends_of_its_range(sbn, init):
    t = sbn.RandomTape(b"proof", ib(init))
    try:
        assert scalars(t.scalars(b"t1", 3)) == model(b"proof", init).random_vector(b"t1", 3)
    finally:
        t.free()


@pytest.mark.parametrize("nc,nv", [SMALL, WIDE, (64, 2), (2, 4)])
def test_r1cs_proof_plan(sbn, nc, nv):
    t = sbn.RandomTape(rtm.NIZK_NAME, ib(INIT))
    try:
        got = t.draw_r1cs_proof(nc, nv)
        n = C.c_size_t(0)
        assert sbn.lib().sbn_r1cs_proof_sizes(nc, nv, C.byref(n), None) == 0 and len(got) == 32 * n.value == 32 * rpm.sizes(nc, nv)[0]
        m = model(rtm.NIZK_NAME)
        assert scalars(got) == rtm.draw_r1cs_proof(m, nc, nv)
        assert scalars(t.scalars(b"next", 1)) == m.random_vector(b"next", 1)             # the tape stands where the model's stands
    finally:
        t.free()


@pytest.mark.parametrize("rounds,n", [(1, 4), (1, 3), (7, 4), (6, 3)])
def test_zk_sumcheck_plan(sbn, rounds, n):
    t = sbn.RandomTape(b"proof", ib(INIT))
    try:
        got = t.draw_zk_sumcheck(rounds, n)
        assert len(got) == 32 * rounds * (n + 4) and scalars(got) == rtm.draw_zk_sumcheck(model(b"proof"), rounds, n)
    finally:
        t.free()


@pytest.mark.parametrize("ell", [1, 2, 6, 7])
def test_polyeval_plan_and_its_pair_layout(sbn, ell):
    lg = pm.factored_lens(ell)[1]
    t = sbn.RandomTape(b"proof", ib(INIT))
    try:
        got = scalars(t.draw_polyeval(ell))
    finally:
        t.free()
    assert len(got) == 3 + 2 * lg and got == rtm.draw_polyeval(model(b"proof"), lg)
    # blinds_vec_1 is drawn whole, then blinds_vec_2; rnd holds (v1[i], v2[i]) pairs
    m = model(b"proof")
    head = [m.random_scalar(b"d"), m.random_scalar(b"r_delta"), m.random_scalar(b"r_delta")]
    v1, v2 = m.random_vector(b"blinds_vec_1", lg), m.random_vector(b"blinds_vec_2", lg)
    assert got[:3] == head and got[3::2] == v1 and got[4::2] == v2


def test_r_beta_is_drawn_under_the_label_r_delta(sbn):
    """nizk/mod.rs:460.  A model that draws r_beta under b"r_beta" gives another r_beta and, behind it, other blinds: the plan must not be that one"""
    ell, lg = 6, 3
    t = sbn.RandomTape(b"proof", ib(INIT))
    try:
        got = scalars(t.draw_polyeval(ell))
    finally:
        t.free()
    literal, renamed = rtm.draw_polyeval(model(b"proof"), lg), rtm.draw_polyeval(model(b"proof"), lg, beta_label=b"r_beta")
    assert got == literal and literal[:2] == renamed[:2] and literal[2] != renamed[2]
    assert all(a != b for a, b in zip(literal[3:], renamed[3:]))
    nc, nv = WIDE
    t = sbn.RandomTape(rtm.NIZK_NAME, ib(INIT))
    try:
        got = scalars(t.draw_r1cs_proof(nc, nv))
    finally:
        t.free()
    assert got == rtm.draw_r1cs_proof(model(rtm.NIZK_NAME), nc, nv) != rtm.draw_r1cs_proof(model(rtm.NIZK_NAME), nc, nv, beta_label=b"r_beta")


@pytest.mark.parametrize("kzg", [False, True])
@pytest.mark.parametrize("nx,ny,N,batch", [(1, 2, 2, 3), (3, 7, 32, 3), (5, 2, 4, 1)])
def test_sparse_eval_plan_and_the_snark_tape(sbn, nx, ny, N, batch, kzg):
    t = sbn.RandomTape(rtm.SNARK_NAME, ib(INIT))
    try:
        got = t.draw_sparse_eval(nx, ny, N, batch, kzg)
    finally:
        t.free()
    assert len(got) == 32 * (skm if kzg else sem).sizes(nx, ny, N, batch)[0]
    assert scalars(got) == rtm.draw_sparse_eval(model(rtm.SNARK_NAME), nx, ny, N, batch, kzg)
    if batch == 3:                                                    # SNARK::prove: one tape through both halves
        comm = dict(nc=1 << nx, nv=1 << (ny - 1), N=N, batch=3)
        t = sbn.RandomTape(rtm.SNARK_NAME, ib(INIT))
        try:
            both = t.draw_r1cs_proof(comm["nc"], comm["nv"]) + t.draw_sparse_eval(nx, ny, N, 3, kzg)
        finally:
            t.free()
        assert scalars(both) == rtm.draw_snark(model(rtm.SNARK_NAME), comm, kzg)


def test_refusals_draw_nothing(sbn):
    L = sbn.lib()
    h = C.c_void_p()
    for bad in (R_MOD, R_MOD + 1, (1 << 256) - 1):
        assert L.sbn_random_tape_new(b"proof", 5, ib(bad), C.byref(h)) == -1 and not h.value
        assert b"canonical" in L.sbn_random_tape_last_error(None)
        with pytest.raises(sbn.SbnError):
            sbn.RandomTape(b"proof", ib(bad))
    assert L.sbn_random_tape_new(b"proof", 5, ib(INIT), None) == -1
    t, m = sbn.RandomTape(b"proof", ib(INIT)), model(b"proof")
    try:
        buf = (C.c_uint8 * (32 * 64))()
        assert L.sbn_r1cs_proof_draw_rnd(2, 2, t.h, buf, 5) == -1 and b"5 scalars" in L.sbn_random_tape_last_error(t.h)      # another count
        assert L.sbn_r1cs_proof_draw_rnd(3, 2, t.h, buf, 64) == -1 and L.sbn_r1cs_proof_draw_rnd(2, 1, t.h, buf, 64) == -1      # shapes sbn_r1cs_proof_sizes refuses
        assert L.sbn_r1cs_proof_draw_rnd(2, 2, t.h, None, rpm.sizes(2, 2)[0]) == -1
        assert L.sbn_zk_sumcheck_draw_rnd(0, 4, t.h, buf, 0) == -1 and L.sbn_zk_sumcheck_draw_rnd(2, 5, t.h, buf, 18) == -1
        assert L.sbn_polyeval_draw_rnd(0, t.h, buf, 3) == -1 and L.sbn_polyeval_draw_rnd(41, t.h, buf, 45) == -1
        assert L.sbn_sparse_eval_draw_rnd(1, 2, 3, 3, 0, t.h, buf, 21) == -1 and L.sbn_sparse_eval_draw_rnd(1, 2, 2, 5, 0, t.h, buf, 21) == -1
        assert L.sbn_snark_draw_rnd(None, 0, t.h, buf, 1) == -1 and L.sbn_nizk_draw_rnd(None, t.h, buf, 1) == -1
        assert L.sbn_random_tape_scalars(t.h, None, 3, 1, buf) == -1 and L.sbn_random_tape_scalars(None, b"d", 1, 1, buf) == -1
        assert L.sbn_r1cs_proof_draw_rnd(2, 2, None, buf, rpm.sizes(2, 2)[0]) == -1
        assert scalars(t.scalars(b"d", 2)) == m.random_vector(b"d", 2)                   # the tape is where it was
    finally:
        t.free()
    L.sbn_random_tape_free(None)


def test_os_seeded_tapes_differ_and_draw_canonical_scalars(sbn):
    a, b = sbn.RandomTape(b"proof"), sbn.RandomTape(b"proof")
    try:
        da, db = scalars(a.draw_r1cs_proof(*WIDE)), scalars(b.draw_r1cs_proof(*WIDE))
    finally:
        a.free(); b.free()
    assert all(x < R_MOD for x in da + db) and da != db and len(set(da)) == len(da)
    assert not set(da) & set(db)


# ---- the header alone, under ASan + UBSan -------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def check(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("random_tape") / "random_tape_check")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        os.path.join(ROOT, "tests", "random_tape_check.cpp"), "-o", exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr

    def run(cases):
        """cases: [(name, init, "op args ...")] -> the scalars each tape drew"""
        text = "".join(f"{name.hex() or '-'} {ib(init).hex()} {ops}\n" for name, init, ops in cases)
        r = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]                  # a sanitizer report ends the program with another status
        lines = r.stdout.splitlines()
        assert lines[-1] == "RANDOM TAPE CHECK DONE" and len(lines) == len(cases) + 1
        return [scalars(bytes.fromhex(ln)) if ln != "-" else [] for ln in lines[:-1]]
    return run


def test_header_alone_draws_what_the_model_draws(check):
    def shape(nc, nv):
        ell = rtm.log2(nv)
        left, right = pm.factored_lens(ell)
        return 1 << left, rtm.log2(nc), ell + 1, right
    se = sem.Shape(3, 7, 32, 3)
    cases = [(b"proof", INIT, f"raw {b'd'.hex()} 2 raw - 3 raw {b'r'.hex()} 0 raw {(b'y' * 170).hex()} 1"),
             (b"", 1, "zk 1 4 zk 5 3"),
             (b"proof", R_MOD - 1, "pe 1 pe 3"),
             (b"proof", INIT, "pe_beta 3"),
             (b"proof", INIT, "r1cs %d %d %d %d" % shape(*SMALL)),
             (b"snark_proof", INIT, "r1cs %d %d %d %d se %d %d %d 0" % (shape(8, 64) + (se.lg["derefs"], se.lg["ops"], se.lg["mem"]))),
             (b"snark_proof", INIT, "se %d %d %d 1" % (se.lg["derefs"], se.lg["ops"], se.lg["mem"])),
             (b"proof", 0, "raw - 0")]
    got = check(cases)
    m = model(b"proof")
    assert got[0] == m.random_vector(b"d", 2) + m.random_vector(b"", 3) + m.random_vector(b"y" * 170, 1)
    m = model(b"", 1)
    assert got[1] == rtm.draw_zk_sumcheck(m, 1, 4) + rtm.draw_zk_sumcheck(m, 5, 3)
    m = model(b"proof", R_MOD - 1)
    assert got[2] == rtm.draw_polyeval(m, 1) + rtm.draw_polyeval(m, 3)
    assert got[3] == rtm.draw_polyeval(model(b"proof"), 3, beta_label=b"r_beta") != rtm.draw_polyeval(model(b"proof"), 3)
    assert got[4] == rtm.draw_r1cs_proof(model(b"proof"), *SMALL)
    assert got[5] == rtm.draw_snark(model(b"snark_proof"), dict(nc=8, nv=64, N=32, batch=3))
    assert got[6] == rtm.draw_sparse_eval(model(b"snark_proof"), 3, 7, 32, 3, kzg=True)
    assert got[7] == []
