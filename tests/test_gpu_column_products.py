"""GPU: the column-wise field products of csrc/fp.cuh that run two at a time or sum two products under one reduction — fe_mulu2,
fe_squ2, fe_mac2u — through the probe library (harness/fe_probe.hip: ops mulu2, squ2, mac2u), limb for limb against tests/fe_model.py.

  * mulu2(a0, b0, a1, b1) must return what two fe_mulu return, squ2(a0, a1) what two fe_squ return;
  * mac2u(a0, b0, a1, b1) must return cols_reduce(cols_mac(cols_mac(0, a0, b0), a1, b1)).

The model is the word-serial one, unchanged: a column-wise product takes the same column totals and the same digits in another order,
so equal limbs are the whole claim.  Operands: every limb at the top of its stated range (2^29 - 1 normalised, the biased difference's
top for the lazy operand, sums of two normalised values), k p in several representations, zero, one, and 2^12 random cases per op,
on both fields.  Every case is also checked to be congruent to the exact result."""
import ctypes
import os
import random
import subprocess
import zlib

import numpy as np
import pytest

import fe_model as fm

pytestmark = pytest.mark.gpu
PKG_DIR = os.path.join(fm.ROOT, "spartan-bn254_amd")
SO = os.path.join(PKG_DIR, "libsbn_fe_probe.so")
N_RANDOM = 1 << 12


@pytest.fixture(scope="module")
def run():
    if not os.path.exists(SO):
        subprocess.run(["make", "-s", "-C", PKG_DIR, "libsbn_fe_probe.so"], check=True)
    lib = ctypes.CDLL(SO)
    lib.fe_probe_op_name.restype = ctypes.c_char_p
    lib.fe_probe_run.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_char_p, ctypes.c_size_t]
    ops = {lib.fe_probe_op_name(i).decode(): i for i in range(lib.fe_probe_num_ops())}

    def go(op, F, cases):
        """cases: n lists of nin limb vectors -> n lists of nout limb vectors"""
        nin, nout, lanes = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
        assert lib.fe_probe_shape(ops[op], 0 if F is fm.FQ else 1, ctypes.byref(nin), ctypes.byref(nout), ctypes.byref(lanes)) == 0, op
        a = np.array(cases, dtype=np.int64).reshape(len(cases), nin.value, fm.NL)
        assert (a == a.astype(np.int32)).all(), "limbs must be int32"
        a = np.ascontiguousarray(a.astype(np.int32))
        out = np.zeros((len(cases), nout.value, fm.NL), dtype=np.int32)
        err = ctypes.create_string_buffer(256)
        rc = lib.fe_probe_run(ops[op], 0 if F is fm.FQ else 1, a.ctypes.data, out.ctypes.data, len(cases), err, 256)
        assert rc == 0, f"{op}: HIP error {rc}: {err.value.decode()}"
        return out.tolist()

    return go


def uval(v):
    return sum(fm.u32(x) << (fm.W * k) for k, x in enumerate(v))


def kp_reps(F):
    """k p as a normalised value (rep_at) and in the inflated form of a biased difference (bias: limbs 0..7 at J 2^29 - J and more)"""
    return [fm.rep_at(F, 0, k) for k in (1, 2, 5)] + [fm.bias(F, K, J) for K, J in ((2, 1), (4, 3), (6, 1))]


def mulu_pairs(F, rng):
    """(a, b) operand pairs of fe_mulu: adversarial first, then random"""
    p, P8 = F.p, F.P8
    two = fm.top_at(F, 2 * P8 + 1, 2 * fm.MASK)                                  # a sum of two normalised values, every limb at its maximum
    norm_top = fm.top_at(F, 5 * P8, fm.MASK)                                     # normalised, 5.2p-sized, limbs 2^29 - 1
    lazy_top = fm.fe_subb(F, 6, 1, fm.top_at(F, P8, fm.MASK), fm.ZERO)           # the biased difference's top: 2^29 - 1 + (6p inflated)
    special = [fm.ZERO, fm.from_int(1), list(F.ONE29), norm_top] + kp_reps(F)
    C = [(two, two), (lazy_top, norm_top), (norm_top, lazy_top), (norm_top, norm_top)]
    C += [(a, b) for a in special for b in special + [lazy_top] if fm.pre_mulu(list(a), list(b))]     # (two inflated forms exceed a column together)
    for _ in range(N_RANDOM):
        d = fm.fe_subb(F, 6, 1, fm.from_int(rng.randrange(0, int(1.2 * p))), fm.from_int(rng.randrange(0, int(5.2 * p))))
        C.append((d, fm.from_int(rng.randrange(0, int(5.2 * p)))))
    assert all(fm.pre_mulu(list(a), list(b)) for a, b in C)
    return C


def squ_operands(F, rng):
    p, P8 = F.p, F.P8
    C = [fm.top_at(F, 2 * P8 + 1, 2 * fm.MASK), fm.top_at(F, 5 * P8, fm.MASK), fm.top_at(F, 7 * P8, (1 << 30) - 1), fm.ZERO, fm.from_int(1), list(F.ONE29)]
    C += [v for v in kp_reps(F) if fm.pre_squ(v)]
    C += [fm.fe_add_lazy(fm.from_int(rng.randrange(0, 1 << 255)), fm.from_int(rng.randrange(0, 1 << 255))) for _ in range(N_RANDOM // 2)]
    C += [fm.from_int(rng.randrange(0, int(7.2 * p))) for _ in range(N_RANDOM // 2)]
    assert all(fm.pre_squ(v) for v in C)
    return C


def in_lockstep(items):
    """every item once as the first and once as the second product of a case, beside a different partner"""
    return [(items[i], items[(i + 1) % len(items)]) for i in range(len(items))]


@pytest.mark.parametrize("fname", ["Fq", "Fr"])
def test_mulu2_equals_two_mulu(run, fname):
    F = fm.FQ if fname == "Fq" else fm.FR
    pairs = mulu_pairs(F, random.Random(zlib.crc32(b"mulu2" + fname.encode())))
    want = [fm.fe_mulu(F, list(a), list(b)) for a, b in pairs]
    idx = in_lockstep(list(range(len(pairs))))
    got = run("mulu2", F, [[pairs[i][0], pairs[i][1], pairs[j][0], pairs[j][1]] for i, j in idx])
    rinv = pow(fm.RMONT, -1, F.p)
    bad = [(i, j, out) for (i, j), out in zip(idx, got) if out != [[fm.i32(x) for x in want[i]], [fm.i32(x) for x in want[j]]]]
    assert not bad, f"mulu2 on {fname}: {len(bad)} of {len(idx)} cases differ from two fe_mulu, first: {pairs[bad[0][0]]}, {pairs[bad[0][1]]} -> {bad[0][2]}"
    for (a, b), r in zip(pairs, want):
        assert fm.is_normalised(r) and (fm.to_int(r) - uval(a) * uval(b) * rinv) % F.p == 0


@pytest.mark.parametrize("fname", ["Fq", "Fr"])
def test_squ2_equals_two_squ(run, fname):
    F = fm.FQ if fname == "Fq" else fm.FR
    ops = squ_operands(F, random.Random(zlib.crc32(b"squ2" + fname.encode())))
    want = [fm.fe_squ(F, list(a)) for a in ops]
    idx = in_lockstep(list(range(len(ops))))
    got = run("squ2", F, [[ops[i], ops[j]] for i, j in idx])
    rinv = pow(fm.RMONT, -1, F.p)
    bad = [(i, j, out) for (i, j), out in zip(idx, got) if out != [[fm.i32(x) for x in want[i]], [fm.i32(x) for x in want[j]]]]
    assert not bad, f"squ2 on {fname}: {len(bad)} of {len(idx)} cases differ from two fe_squ, first: {ops[bad[0][0]]}, {ops[bad[0][1]]} -> {bad[0][2]}"
    for a, r in zip(ops, want):
        assert fm.is_normalised(r) and (fm.to_int(r) - uval(a) ** 2 * rinv) % F.p == 0


@pytest.mark.parametrize("fname", ["Fq", "Fr"])
def test_mac2u_equals_two_cols_mac_and_one_reduction(run, fname):
    """operands as cols_mac_lazy states them: a0, a1 normalised (limbs below 2^29), b0, b1 non-negative with limbs below 2^30.6"""
    F = fm.FQ if fname == "Fq" else fm.FR
    p, P8 = F.p, F.P8
    rng = random.Random(zlib.crc32(b"mac2u" + fname.encode()))
    norm_top = fm.top_at(F, int(5.2 * P8), fm.MASK)
    lazy_top = fm.fe_subb(F, 6, 1, fm.top_at(F, P8, fm.MASK), fm.ZERO)
    neg_top = fm.fe_negb(F, 4, fm.ZERO)
    norm = [fm.ZERO, fm.from_int(1), list(F.ONE29), norm_top, fm.top_at(F, P8, fm.MASK)] + [fm.rep_at(F, 0, k) for k in (1, 2, 5)]
    lazy = norm + [lazy_top, neg_top] + [fm.bias(F, K, J) for K, J in ((2, 1), (4, 3), (6, 1))]
    C = [[norm_top, lazy_top, norm_top, lazy_top],                                # both products at the top: 2 * 9 * 2^59.6 per column
         [norm_top, lazy_top, fm.top_at(F, P8, fm.MASK), neg_top]]                # g1.cuh's Y3 at its top
    C += [[a0, b0, a1, b1] for a0 in norm for b0 in lazy for a1, b1 in ((norm_top, lazy_top), (fm.ZERO, fm.ZERO), (list(F.ONE29), neg_top))]
    C += [[a1, b1, a0, b0] for a0 in norm for b0 in lazy for a1, b1 in ((norm_top, lazy_top),)]
    for _ in range(N_RANDOM):
        R = fm.from_int(rng.randrange(0, int(5.2 * p)))
        t1 = fm.fe_subb(F, 6, 1, fm.from_int(rng.randrange(0, int(1.1 * p))), fm.from_int(rng.randrange(0, int(5.2 * p))))
        C.append([R, t1, fm.from_int(rng.randrange(0, int(1.1 * p))), fm.fe_negb(F, 4, fm.from_int(rng.randrange(0, int(3.2 * p))))])
    got = run("mac2u", F, C)
    rinv = pow(fm.RMONT, -1, F.p)
    bad = []
    for ins, out in zip(C, got):
        s = fm.cols_zero()
        fm.cols_mac(s, ins[0], ins[1]); fm.cols_mac(s, ins[2], ins[3])          # (the model asserts that no column leaves 64 bits)
        want = fm.cols_reduce(F, s)
        total = uval(ins[0]) * uval(ins[1]) + uval(ins[2]) * uval(ins[3])
        assert fm.is_normalised(want) and (fm.to_int(want) - total * rinv) % F.p == 0 and 0 <= fm.to_int(want) * fm.RMONT < total + F.p * fm.RMONT
        if out[0] != [fm.i32(x) for x in want]:
            bad.append((ins, out[0]))
    assert not bad, f"mac2u on {fname}: {len(bad)} of {len(C)} cases differ from cols_mac x 2 + cols_reduce, first: {bad[0]}"
