"""GPU: the lazy field / G1 layer (csrc/fp.cuh, csrc/g1.cuh) at the edges of its value ranges, through the test-only probe library
spartan-bn254_amd/libsbn_fe_probe.so (harness/fe_probe.hip: the shipped inline functions, one thread per case, raw 9-limb I/O).

Every field primitive runs on both fields over adversarial cases (thresholds, range tops, k p in several representations) plus a
random batch, and must match tests/fe_model.py limb for limb, be congruent to the exact result and land inside its documented range.
The G1 formulas run on real curve points scaled by random lambda, with every coordinate moved to the top of its range, including
the degenerate cases, and in chains of 4096 steps whose ranges are checked after every step.

The probe checks the semantics of the shipped inline functions in the probe's own kernels.  A miscompile that only happens in one
product kernel's register context is not visible here: that stays the job of the end-to-end tests (MSM, sumcheck, bullet folds)."""
import ctypes
import os
import random
import subprocess
import zlib
from fractions import Fraction

import numpy as np
import pytest

import fe_model as fm
import pyref

pytestmark = pytest.mark.gpu
PKG_DIR = os.path.join(fm.ROOT, "spartan-bn254_amd")
SO = os.path.join(PKG_DIR, "libsbn_fe_probe.so")
N_CHEAP, N_PROD = 1 << 16, 1 << 14          # random cases per op: limb-wise ops / products (the model runs in Python)
STATS = {}                                  # (op, what) -> [cases, max value / p, bound]


class Probe:
    def __init__(self, lib):
        self.lib = lib
        lib.fe_probe_op_name.restype = ctypes.c_char_p
        lib.fe_probe_run.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_char_p, ctypes.c_size_t]
        self.ops = {lib.fe_probe_op_name(i).decode(): i for i in range(lib.fe_probe_num_ops())}

    def run(self, op, F, cases):
        """cases: n lists of lanes * nin limb vectors -> n lists of lanes lists of nout limb vectors (ints)"""
        field = 0 if F is fm.FQ else 1
        nin, nout, lanes = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
        assert self.lib.fe_probe_shape(self.ops[op], field, ctypes.byref(nin), ctypes.byref(nout), ctypes.byref(lanes)) == 0, op
        n = len(cases)
        a = np.ascontiguousarray(np.array(cases, dtype=np.int64).reshape(n, lanes.value * nin.value, fm.NL).astype(np.int32))
        assert (a.astype(np.int64) == np.array(cases, dtype=np.int64).reshape(a.shape)).all(), "limbs must be int32"
        out = np.zeros((n, lanes.value, nout.value, fm.NL), dtype=np.int32)
        err = ctypes.create_string_buffer(256)
        rc = self.lib.fe_probe_run(self.ops[op], field, a.ctypes.data, out.ctypes.data, n, err, 256)
        assert rc == 0, f"{op}: HIP error {rc}: {err.value.decode()}"
        return out.tolist()


@pytest.fixture(scope="module")
def probe():
    if not os.path.exists(SO):
        subprocess.run(["make", "-s", "-C", PKG_DIR, "libsbn_fe_probe.so"], check=True)
    yield Probe(ctypes.CDLL(SO))
    if STATS:
        print("\nfe_probe ranges: op / value: cases, max over all cases, stated bound")
        for (op, what), (n, mx, bound) in sorted(STATS.items()):
            print(f"  {op:22s} {what:8s} {n:8d}  max {mx:.4f}p of {bound}p" if what != "cases" else f"  {op:22s} cases    {n:8d}")


def note(op, what, v, p, bound):
    s = STATS.setdefault((op, what), [0, float("-inf"), bound])
    s[0] += 1
    s[1] = max(s[1], fm.to_int(v) / p)


def below(v, hi, p, lo=0):
    x = fm.to_int(v)
    return Fraction(str(lo)) * p <= x < Fraction(str(hi)) * p


# ---------------------------------------------------------------- field primitives
def rand_int(rng, lo, hi):
    return rng.randrange(int(lo), int(hi))


def wide_edges(F, rng):
    """the top of fe_reduce's wide domain and the sums the equal-base merge feeds it, both signs"""
    p, K = F.p, fm.REDUCE_WIDE
    xs = [K * p - 1, K * p - (1 << 200), K * p - p // 3, (K - 1) * p, (K - 1) * p + 1, 320 * p - 1, 320 * p, 160 * p + 1, 13 * p, 13 * p + 1]
    xs += [rand_int(rng, 13 * p, K * p) for _ in range(64)]
    return xs + [-x for x in xs]


def field_cases(F, op, rng):
    """(inputs, model output, check) per case: adversarial first, then random"""
    p, P8 = F.p, F.P8
    nr = N_PROD if op in ("mul", "sqr", "mulu", "squ", "reduce", "canon", "is_zero", "eq", "cols_mac12", "cols_lazy2", "to_mont",
                           "from_mont", "from_ark_mont", "ark_mont_to_plain") else N_CHEAP
    C = []
    if op in ("norm",):
        for x in [0, -1, 1, p, -p, 13 * p, -13 * p] + [rand_int(rng, -13 * p, 13 * p) for _ in range(nr)]:
            C.append([fm.unnormalised(x, rng)])
    elif op == "normu":
        for _ in range(nr):
            C.append([[rng.randrange(0, 1 << 31) for _ in range(8)] + [rng.randrange(0, 1 << 26)]])
        C.append([[(1 << 31) - 1] * 8 + [0]])
    elif op in ("add", "sub"):
        edge = [0, -1, 4 * p - 1, -(4 * p - 1)]
        C += [[fm.from_int(a), fm.from_int(b)] for a in edge for b in edge]
        C += [[fm.from_int(rand_int(rng, -4 * p, 4 * p)), fm.from_int(rand_int(rng, -4 * p, 4 * p))] for _ in range(nr)]
    elif op in ("dbl", "neg"):
        C += [[fm.from_int(x)] for x in [0, -1, 1, 4 * p - 1, -(4 * p - 1)]]
        C += [[fm.from_int(rand_int(rng, -4 * p, 4 * p))] for _ in range(nr)]
    elif op in ("mul", "sqr", "reduce", "canon"):
        edge = [13 * p - 1, -(13 * p - 1), 2 * p - 1, -(2 * p - 1), p, -p, 1, -1, 0, (1 << 232) - 1, -(1 << 232)]
        if op == "mul":
            C += [[fm.from_int(a), fm.from_int(b)] for a in edge for b in edge if abs(a * b) < 169 * p * p]
            C += [[fm.from_int(rand_int(rng, -13 * p, 13 * p)), fm.from_int(rand_int(rng, -12 * p, 12 * p))] for _ in range(nr // 2)]
            C += [[fm.from_int(rand_int(rng, -2 * p, 2 * p)), fm.from_int(rand_int(rng, -2 * p, 2 * p))] for _ in range(nr // 2)]
        else:
            C += [[fm.from_int(x)] for x in edge] + ([[fm.unnormalised(x, rng)] for x in edge] if op != "sqr" else [])
            C += [[fm.from_int(rand_int(rng, -13 * p, 13 * p))] for _ in range(nr)]
            if op != "sqr":                                 # the wide line of fe_reduce's contract: |a| < 448 p (the equal-base merge's sums)
                C += [[v] for x in wide_edges(F, rng) for v in (fm.from_int(x), fm.unnormalised(x, rng))]
    elif op in ("mulu", "squ"):
        top = [fm.MASK * 2] * 8 + [2 * P8 + 1]              # a sum of two normalised values, limbs at their maximum
        if op == "mulu":
            C += [[top, top], [fm.bias(F, 6, 1), [fm.MASK] * 8 + [5 * P8]]]
            for _ in range(nr):
                d = fm.fe_subb(F, 6, 1, fm.from_int(rand_int(rng, 0, 1.2 * p)), fm.from_int(rand_int(rng, 0, 5.2 * p)))
                C.append([d, fm.from_int(rand_int(rng, 0, 5.2 * p))])
        else:
            C += [[top], [fm.from_int(0)]]
            C += [[fm.fe_add_lazy(fm.from_int(rand_int(rng, 0, 1 << 255)), fm.from_int(rand_int(rng, 0, 1 << 255)))]   # limbs < 2^30
                  for _ in range(nr // 2)]
            C += [[fm.from_int(rand_int(rng, 0, 7.2 * p))] for _ in range(nr // 2)]
    elif op == "canon_small":
        C += [[fm.from_int(x)] for x in [-p + 1, -1, 0, 1, p - 1, p, p + 1, 2 * p - 1]]
        C += [[fm.from_int(rand_int(rng, -p + 1, 2 * p))] for _ in range(nr)]
    elif op in ("is_zero", "maybe_zero"):
        for k in range(-8 if op == "maybe_zero" else -12, 9 if op == "maybe_zero" else 13):
            C += [[fm.from_int(k * p)]] + [[fm.unnormalised(k * p, rng)] for _ in range(4)]
        C += [[fm.from_int(rand_int(rng, -8 * p, 8 * p))] for _ in range(nr)]
        if op == "is_zero":                                 # up to the top of the wide domain: k p and its neighbours, both signs
            for k in (14, 160, 320, 400, fm.REDUCE_WIDE - 1):
                for x in (k * p, -k * p, k * p + 1, -k * p - 1, k * p - 1):
                    C += [[fm.from_int(x)], [fm.unnormalised(x, rng)]]
            C += [[v] for x in wide_edges(F, rng) for v in (fm.from_int(x), fm.unnormalised(x, rng))]
    elif op == "eq":
        for _ in range(nr):
            x = rand_int(rng, 0, p)
            y = x + rng.randrange(-4, 5) * p if rng.random() < 0.5 else rand_int(rng, -4 * p, 4 * p)
            C.append([fm.from_int(x + rng.randrange(-4, 5) * p), fm.unnormalised(y, rng)])
    elif op.startswith("subb_"):
        K, J = map(int, op.split("_")[1:])
        top_max = int(Fraction(K * 1000 - 1, 1000) * p / (1 << 232))
        C.append([[fm.MASK] * 8 + [int(5.2 * P8)], [J * fm.MASK] * 8 + [top_max - J]])
        C.append([[0] * 9, [J * fm.MASK] * 8 + [top_max - J]])
        for _ in range(nr):
            b = [0] * 9
            for _ in range(J):
                b = fm.fe_add_lazy(b, fm.from_int(rand_int(rng, 0, min(p, (K - 0.001) * p / J))))
            C.append([fm.from_int(rand_int(rng, 0, 5.2 * p)), b])
    elif op.startswith("negb_"):
        K = int(op.split("_")[1])
        C += [[fm.from_int(x)] for x in (0, p - 1, (K * 1000 - 1) * p // 1000 - 1)]
        C += [[fm.from_int(rand_int(rng, 0, (K - 0.001) * p))] for _ in range(nr)]
    elif op.startswith("fix_nonneg_"):
        K = int(op.split("_")[2])
        C += [[fm.from_int(x)] for x in (-K * p + 1, -1, 0, 1, (1 << 256) - K * p - 1)]
        C += [[fm.from_int(rand_int(rng, -K * p + 1, (1 << 256) - K * p))] for _ in range(nr)]
    elif op in ("fix_tab", "store_tab"):
        for t in (-2 * P8, -P8, 0, 2 * P8 + 2, int(4.5 * P8)):
            for top in range(t - 3, t + 4):
                for low in (0, fm.MASK, rng.randrange(fm.MASK + 1)):
                    x = fm.top_at(F, top, low)
                    if fm.pre_fix_tab(F, x):
                        C.append([x if op == "fix_tab" else fm.unnormalised(fm.to_int(x), rng)])
        C += [[fm.from_int(x)] for x in (-2 * p + 1, -p - 1, -p, -p + 1, -1, 0, 2 * p - 1, 2 * p, 2 * p + 1, 9 * p // 2 - 1)]
        C += [[fm.from_int(rand_int(rng, -2 * p + 1, 4.5 * p))] for _ in range(nr)]
    elif op == "cols_mac12":
        full = [fm.MASK] * 8 + [3 * P8]
        C.append([full] * 24)
        C += [[fm.from_int(rand_int(rng, 0, 2.5 * p)) for _ in range(24)] for _ in range(nr // 8)]
    elif op == "cols_lazy2":
        for _ in range(nr):
            R = fm.from_int(rand_int(rng, 0, 5.2 * p))
            t1 = fm.fe_subb(F, 6, 1, fm.from_int(rand_int(rng, 0, 1.1 * p)), fm.from_int(rand_int(rng, 0, 5.2 * p)))
            C.append([R, t1, fm.from_int(rand_int(rng, 0, 1.1 * p)), fm.fe_negb(F, 4, fm.from_int(rand_int(rng, 0, 3.2 * p)))])
        C.append([[fm.MASK] * 8 + [int(5.2 * P8)], fm.fe_subb(F, 6, 1, [fm.MASK] * 8 + [P8], [0] * 9), [fm.MASK] * 8 + [P8],
                  fm.fe_negb(F, 4, [0] * 9)])
    elif op in ("to_mont", "from_mont", "from_ark_mont", "ark_mont_to_plain"):
        C += [[fm.from_int(x)] for x in (0, 1, p - 1)]
        C += [[fm.from_int(rand_int(rng, 0, p))] for _ in range(nr)]
    elif op == "from_u64":
        for x in [0, 1, (1 << 29) - 1, 1 << 29, (1 << 58) - 1, 1 << 58, (1 << 64) - 1] + [rng.randrange(1 << 64) for _ in range(nr)]:
            C.append([[fm.i32(x), fm.i32(x >> 32)] + [0] * 7])
    elif op == "inv":
        C += [[fm.from_int(x)] for x in (1, p - 1, fm.to_int(F.ONE29))] + [[fm.from_int(rand_int(rng, 1, p))] for _ in range(256)]
    elif op in ("is_canonical", "unpack"):
        ws = [p - 1, p, p + 1, (1 << 256) - 1, 0, ((p >> 224) + 1) << 224, (((p >> 192) + 1) << 192), (p >> 224) << 224 | ((1 << 224) - 1),
              p - (1 << 32), p + (1 << 32)]
        ws += [rng.randrange(1 << 256) for _ in range(nr)] + [rand_int(rng, 0, p) for _ in range(nr)]
        C += [[fm.int_to_words(x) + [0]] for x in ws]
    elif op == "pack":
        C += [[fm.from_int(x)] for x in ((1 << 256) - 1, 0, p - 1, 5 * p)] + [[fm.from_int(rng.randrange(1 << 256))] for _ in range(nr)]
    return C


def model_field(F, op, ins):
    """(model output limbs, check(out) -> bool, (what, value, bound) or None for the range statistics)"""
    p = F.p
    a = ins[0]
    rinv = pow(fm.RMONT, -1, p)
    if op == "norm":
        r = fm.fe_norm(a); return r, fm.is_normalised(r) and fm.to_int(r) == fm.to_int(a), None
    if op == "normu":
        r = fm.fe_normu(a); return r, fm.is_normalised(r) and fm.to_int(r) == sum(fm.u32(x) << (29 * k) for k, x in enumerate(a)), None
    if op in ("add", "sub"):
        r = (fm.fe_add if op == "add" else fm.fe_sub)(a, ins[1])
        want = fm.to_int(a) + (1 if op == "add" else -1) * fm.to_int(ins[1])
        return r, fm.is_normalised(r) and fm.to_int(r) == want, None
    if op in ("dbl", "neg"):
        r = (fm.fe_dbl if op == "dbl" else fm.fe_neg)(a)
        return r, fm.is_normalised(r) and fm.to_int(r) == (2 if op == "dbl" else -1) * fm.to_int(a), None
    if op in ("mul", "sqr"):
        b = ins[1] if op == "mul" else a
        assert fm.pre_mul(a, b)
        r = fm.fe_mul(F, a, b) if op == "mul" else fm.fe_sqr(F, a)
        x, y = fm.to_int(a), fm.to_int(b)
        lo, hi = (-0.1, 1.1) if abs(x) < 2 * p and abs(y) < 2 * p else (-1, 2)
        ok = fm.is_normalised(r) and below(r, hi, p, lo) and (fm.to_int(r) - x * y * rinv) % p == 0
        return r, ok, (op, r, hi)
    if op in ("mulu", "squ"):
        b = ins[1] if op == "mulu" else a
        assert fm.pre_mulu(a, b) if op == "mulu" else fm.pre_squ(a)
        r = fm.fe_mulu(F, a, b) if op == "mulu" else fm.fe_squ(F, a)
        x, y = (sum(fm.u32(v) << (29 * k) for k, v in enumerate(t)) for t in (a, b))
        ok = fm.is_normalised(r) and 0 <= fm.to_int(r) < Fraction(x * y, fm.RMONT) + p and (fm.to_int(r) - x * y * rinv) % p == 0
        return r, ok, None
    if op in ("reduce", "canon"):
        tight = fm.pre_reduce(F, a)
        assert tight or fm.pre_reduce(F, a, wide=True)
        r = fm.fe_reduce(F, a) if op == "reduce" else fm.fe_canon(F, a)
        if tight:
            ok = (below(r, 1.1, p, -0.1) if op == "reduce" else fm.to_int(r) == fm.to_int(a) % p) and fm.is_normalised(r)
            return r, ok and (fm.to_int(r) - fm.to_int(a)) % p == 0, (op, r, 1.1) if op == "reduce" else None
        lo, hi = fm.reduce_interval(F, a)
        ok = (lo <= fm.to_int(r) < hi and below(r, 1.76, p, -0.76) if op == "reduce" else fm.to_int(r) == fm.to_int(a) % p) and fm.is_normalised(r)
        return r, ok and (fm.to_int(r) - fm.to_int(a)) % p == 0, (op + " wide", r, 1.76) if op == "reduce" else None
    if op == "canon_small":
        assert fm.pre_canon_small(F, a)
        r = fm.fe_canon_small(F, a); return r, r == fm.from_int(fm.to_int(a) % p), None
    if op in ("is_zero", "maybe_zero", "eq"):
        if op == "is_zero":
            assert fm.pre_reduce(F, a, wide=True)
            v = fm.fe_is_zero(F, a); ok = v == (fm.to_int(a) % p == 0)
        elif op == "eq":
            v = fm.fe_eq(F, a, ins[1]); ok = v == ((fm.to_int(a) - fm.to_int(ins[1])) % p == 0)
        else:
            assert fm.pre_maybe_zero(F, a)
            v = fm.fe_maybe_zero(F, a); ok = v or fm.to_int(a) % p != 0          # never a false negative
        return [int(v)] + [0] * 8, ok, None
    if op.startswith("subb_") or op.startswith("negb_"):
        parts = list(map(int, op.split("_")[1:]))
        K, J = parts[0], parts[1] if len(parts) > 1 else 1
        if op.startswith("subb_"):
            assert fm.pre_subb(F, K, J, a, ins[1])
            r = fm.fe_subb(F, K, J, a, ins[1]); want = fm.to_int(a) - fm.to_int(ins[1]) + K * p
        else:
            assert fm.pre_subb(F, K, 1, [0] * 9, a)
            r = fm.fe_negb(F, K, a); want = K * p - fm.to_int(a)
        ok = sum(fm.u32(x) << (29 * k) for k, x in enumerate(r)) == want and want > 0
        return r, ok, None
    if op.startswith("fix_nonneg_"):
        K = int(op.split("_")[2])
        assert fm.pre_fix_nonneg(F, K, a)
        r = fm.fe_fix_nonneg(F, K, a)
        return r, fm.is_normalised(r) and 0 <= fm.to_int(r) < 1 << 256 and (fm.to_int(r) - fm.to_int(a)) % p == 0, None
    if op == "fix_tab":
        assert fm.pre_fix_tab(F, a)
        r = fm.fe_fix_tab(F, a)
        return r, fm.is_normalised(r) and below(r, 2.5, p) and (fm.to_int(r) - fm.to_int(a)) % p == 0, (op, r, 2.5)
    if op == "store_tab":
        x = fm.fe_fix_tab(F, fm.fe_norm(a))
        w = fm.to_int(x)
        return fm.int_to_words(w) + [0], 0 <= w and below(x, 2.5, p) and (w - fm.to_int(a)) % p == 0, None
    if op in ("cols_mac12", "cols_lazy2"):
        s = fm.cols_zero()
        total = 0
        for i in range(0, len(ins), 2):
            fm.cols_mac(s, ins[i], ins[i + 1])
            total += sum(fm.u32(v) << (29 * k) for k, v in enumerate(ins[i])) * sum(fm.u32(v) << (29 * k) for k, v in enumerate(ins[i + 1]))
            if op == "cols_mac12" and i == 10:
                fm.cols_carry(s)
        r = fm.cols_reduce(F, s)
        return r, fm.is_normalised(r) and 0 <= fm.to_int(r) < Fraction(total, fm.RMONT) + p and (fm.to_int(r) - total * rinv) % p == 0, None
    if op in ("to_mont", "from_mont", "from_ark_mont", "ark_mont_to_plain"):
        x = fm.to_int(a)
        if op == "to_mont":
            r = fm.fe_mul(F, a, F.R2_29); want = x * fm.RMONT
        elif op == "from_ark_mont":
            r = fm.fe_mul(F, a, F.CIN_29); want = x * 32
        else:
            r = fm.fe_canon_small(F, fm.fe_mul(F, a, fm.from_int(1 if op == "from_mont" else 32)))
            want = x * rinv * (1 if op == "from_mont" else 32)
            return r, fm.to_int(r) == want % p, None
        return r, fm.is_normalised(r) and below(r, 1.1, p) and (fm.to_int(r) - want) % p == 0, None
    if op == "from_u64":
        x = fm.u32(a[0]) | fm.u32(a[1]) << 32
        r = fm.from_int(x); return r, True, None
    if op == "inv":
        return None, None, None
    if op == "is_canonical":
        v = fm.words_to_int(a) < p
        return [int(v)] + [0] * 8, True, None
    if op == "unpack":
        r = fm.from_int(fm.words_to_int(a)); return r, True, None
    if op == "pack":
        return fm.int_to_words(fm.to_int(a)) + [0], True, None
    raise KeyError(op)


FIELD_OPS = ["norm", "normu", "add", "sub", "dbl", "neg", "mul", "sqr", "mulu", "squ", "reduce", "canon_small", "canon", "is_zero", "eq",
             "maybe_zero", "subb_3_1", "subb_4_2", "subb_9_1", "subb_14_1", "subb_2_1", "subb_4_1", "subb_4_3", "subb_6_1", "negb_2", "negb_4",
             "fix_nonneg_1", "fix_nonneg_2", "fix_nonneg_4", "fix_tab", "cols_mac12", "cols_lazy2", "to_mont", "from_mont",
             "from_ark_mont", "ark_mont_to_plain", "from_u64", "inv", "is_canonical", "unpack", "pack", "store_tab"]
FR_ONLY = {"subb_3_1", "subb_4_2", "subb_9_1", "subb_14_1"}
FQ_ONLY = {"subb_2_1", "subb_4_1", "subb_4_3", "subb_6_1", "negb_4", "fix_nonneg_1", "fix_nonneg_2", "fix_nonneg_4"}
PARAMS = [(f, op) for op in FIELD_OPS for f in ("Fq", "Fr") if not (f == "Fq" and op in FR_ONLY) and not (f == "Fr" and op in FQ_ONLY)]


@pytest.mark.parametrize("fname,op", PARAMS, ids=["%s-%s" % t for t in PARAMS])
def test_field_primitive(probe, fname, op):
    F = fm.FQ if fname == "Fq" else fm.FR
    rng = random.Random(zlib.crc32((fname + op).encode()))
    cases = field_cases(F, op, rng)
    assert cases, op
    got = probe.run(op, F, cases)
    bad = []
    for ins, out in zip(cases, got):
        r = out[0][0]
        if op == "inv":
            ok = fm.is_normalised(r) and (fm.to_int(r) * fm.to_int(ins[0]) - fm.RMONT * fm.RMONT) % F.p == 0
        else:
            want, ok, st = model_field(F, op, ins)
            ok = ok and r == [fm.i32(x) for x in want]
            if st:
                note(f"{fname} {st[0]}", "value", st[1], F.p, st[2])
        if not ok:
            bad.append((ins, r))
    STATS.setdefault((f"{fname} {op}", "cases"), [len(cases), 0.0, "-"])
    assert not bad, f"{op} on {fname}: {len(bad)} of {len(cases)} cases wrong, first: {bad[0]}"


# ---------------------------------------------------------------- G1
def check_xyzz(op, pt, want, extra=""):
    F = fm.FQ
    for name, v, lim in zip(fm.RANGES, pt, fm.RANGES.values()):
        assert fm.is_normalised(v) and below(v, lim, F.p), (op, name, fm.ratio(F, v), extra)
        note(op, name, v, F.p, lim)
    assert fm.xyzz_affine(pt) == want, (op, extra)
    if pt[2] != [0] * 9:
        zz, zzz = (fm.to_int(v) for v in pt[2:])
        assert (zz ** 3 - zzz ** 2 * fm.RMONT) % F.p == 0, "ZZ^3 != ZZZ^2"      # Montgomery values: zz = ZZ R, zzz = ZZZ R


def steer_same_x(acc, qx, k, F=fm.FQ):
    """acc with its X representative chosen so that madd's P = U2 - X + 6p is exactly k p (None if out of range)"""
    U2 = fm.to_int(fm.fe_mulu(F, qx, acc[2]))
    X = U2 + (6 - k) * F.p
    if not 0 <= X < Fraction("5.2") * F.p:
        return None
    return (fm.from_int(X),) + tuple(acc[1:])


def g1_pairs(rng, n):
    pts = [pyref.mul(pyref.G, rng.randrange(1, pyref.R)) for _ in range(n)]
    out = []
    for i, a in enumerate(pts):
        b = pts[(i + 1) % n]
        out += [(a, b), (a, a), (a, pyref.neg(a)), (None, a), (a, None)]
    return out


def test_madd_edges(probe):
    F = fm.FQ
    rng = random.Random(101)
    cases, meta = [], []
    for a, b in g1_pairs(rng, 48):
        for neg in (False, True):
            acc = fm.xyzz_of(a, rng.randrange(2, F.p))
            accs = [acc]
            if a is not None and b is not None and a[0] == b[0]:
                for k in range(1, 7):                     # P = k p for every k the range allows
                    s = steer_same_x(acc, fm.affine_of(b)[0], k)
                    if s:
                        accs.append(s)
            for ac in accs:
                cases.append(list(ac) + list(fm.affine_of(b)))
                meta.append((a, b, neg))
    for neg in (False, True):
        idx = [i for i, m in enumerate(meta) if m[2] == neg]
        got = probe.run("madd_neg" if neg else "madd", F, [cases[i] for i in idx])
        for i, out in zip(idx, got):
            a, b, _ = meta[i]
            r = tuple(out[0])
            acc, q = tuple(cases[i][:4]), tuple(cases[i][4:])
            assert list(r) == [list(v) for v in fm.xyzz_madd(acc, q, neg)], (a, b, neg)
            check_xyzz("madd_neg" if neg else "madd", r, pyref.add(a, pyref.neg(b) if neg else b))


def test_add_inl_and_quad_edges(probe):
    F = fm.FQ
    rng = random.Random(202)
    cases, meta, ks = [], [], set()
    for a, b in g1_pairs(rng, 40):
        tries = 24 if (a is not None and b is not None and a[0] == b[0]) else 1
        for _ in range(tries):
            A, B = fm.xyzz_of(a, rng.randrange(2, F.p)), fm.xyzz_of(b, rng.randrange(2, F.p))
            if tries > 1:                                  # P = U2 - U1 + 2p: keep the representations that reach p and 3p
                tr = {}
                fm.xyzz_add_inl(A, B, tr)
                k = fm.to_int(tr["P"]) // F.p
                if k in ks and rng.random() < 0.9:
                    continue
                ks.add(k)
            cases.append(list(A) + list(B))
            meta.append((a, b))
    assert {2} <= ks
    got = probe.run("add_inl", F, cases)
    quad = probe.run("add_quad", F, [c * 4 for c in cases])
    for ins, out, qd, (a, b) in zip(cases, got, quad, meta):
        A, B = tuple(ins[:4]), tuple(ins[4:])
        want = fm.xyzz_add_inl(A, B)
        assert [list(v) for v in out[0]] == [list(v) for v in want]
        check_xyzz("add_inl", tuple(out[0]), pyref.add(a, b))
        assert qd[0] == qd[1] == qd[2] == qd[3], "quad lanes disagree"
        check_xyzz("add_quad", tuple(qd[0]), pyref.add(a, b))
        if a is not None and b is not None and a[0] != b[0]:
            assert qd[0][1] == fm.xyzz_add_quad_y(A, B) and qd[0][0] == out[0][0] and qd[0][2:] == out[0][2:]
    STATS[("add_inl", "P=kp k")] = [len(ks), max(ks), "{1,2,3}"]


def test_dbl_and_store_load(probe):
    F = fm.FQ
    rng = random.Random(303)
    pts = [pyref.mul(pyref.G, rng.randrange(1, pyref.R)) for _ in range(128)]
    xyzz = [fm.xyzz_of(a, rng.randrange(2, F.p)) for a in pts]
    got = probe.run("dbl_xyzz", F, [list(p) for p in xyzz] + [list(fm.xyzz_inf())])
    for a, p, out in zip(pts + [None], xyzz + [fm.xyzz_inf()], got):
        assert [list(v) for v in out[0]] == [list(v) for v in fm.xyzz_dbl(p)[0]]
        check_xyzz("dbl_xyzz", tuple(out[0]), pyref.add(a, a))
    aff = probe.run("dbl_affine", F, [list(fm.affine_of(a)) for a in pts])
    for a, out in zip(pts, aff):
        assert [list(v) for v in out[0]] == [list(v) for v in fm.xyzz_dbl_affine(*fm.affine_of(a))[0]]
        check_xyzz("dbl_affine", tuple(out[0]), pyref.add(a, a))
    # the store format: coordinates at the top of their ranges, and the signed-path outputs above (X down to -2.2p before the fix-up)
    signed = []
    for a, p, out, o2 in zip(pts, xyzz, got, aff):
        X, Y = fm.xyzz_dbl(p)[1]
        signed.append((X, Y) + tuple(out[0][2:]))
        X, Y = fm.xyzz_dbl_affine(*fm.affine_of(a))[1]
        signed.append((X, Y) + tuple(o2[0][2:]))
    assert min(fm.to_int(q[0]) for q in signed) < -F.p             # X below -p reaches the fix-up's second multiple of p
    inputs = [list(p) for p in xyzz] + [list(s) for s in signed] + [list(fm.xyzz_inf())]
    back = probe.run("store_load", F, inputs)
    for p, out in zip(inputs, back):
        assert [list(v) for v in out[0]] == [list(v) for v in fm.xyzz_store_load(tuple(p))]
        assert fm.xyzz_affine(tuple(out[0])) == fm.xyzz_affine(tuple(p))
    aff_back = probe.run("to_affine", F, [list(p) for p in xyzz[:32]] + [list(fm.xyzz_inf())])
    for a, out in zip(pts[:32] + [None], aff_back):
        assert [fm.to_int(v) for v in out[0]] == ([0, 0] if a is None else [F.mont(a[0]), F.mont(a[1])])


def test_wave_sum(probe):
    F = fm.FQ
    rng = random.Random(404)
    cases, wants = [], []
    for c in range(12):
        pts = [pyref.mul(pyref.G, rng.randrange(1, pyref.R)) for _ in range(64)]
        for i in range(64):                                 # equal, opposite and empty lanes, at several tree levels
            if rng.random() < 0.15:
                pts[i] = None
            elif rng.random() < 0.15:
                pts[i] = pts[i ^ (1 << rng.randrange(6))]
            elif rng.random() < 0.1 and pts[i ^ 1] is not None:
                pts[i] = pyref.neg(pts[i ^ 1])
        want = None
        for q in pts:
            want = pyref.add(want, q)
        cases.append([list(fm.xyzz_of(q, rng.randrange(2, F.p))) for q in pts])
        wants.append(want)
    got = probe.run("wave_sum", F, [sum(c, []) for c in cases])
    for out, want in zip(got, wants):
        assert all(lane == out[0] for lane in out), "wave lanes disagree"
        check_xyzz("wave_sum", tuple(out[0]), want)


@pytest.mark.parametrize("kind", ["madd", "add_inl"])
def test_chain(probe, kind):
    """4096 steps on 32 chains, each output fed back in; random, equal and opposite addends; ranges after every step"""
    F = fm.FQ
    rng = random.Random(505 if kind == "madd" else 606)
    pool = [pyref.mul(pyref.G, rng.randrange(1, pyref.R)) for _ in range(64)]
    nch, steps = 32, 4096
    state = [list(fm.xyzz_inf()) for _ in range(nch)]
    point = [None] * nch
    for step in range(steps):
        neg = kind == "madd" and step % 2 == 1
        ins, adds = [], []
        for c in range(nch):
            u = rng.random()
            q = point[c] if u < 0.02 else pyref.neg(point[c]) if u < 0.03 else rng.choice(pool)
            adds.append(pyref.neg(q) if neg else q)
            if kind == "madd":
                ins.append(state[c] + list(fm.affine_of(q)))
            else:
                ins.append(state[c] + list(fm.xyzz_of(q, rng.randrange(2, F.p))))
        got = probe.run(("madd_neg" if neg else "madd") if kind == "madd" else "add_inl", F, ins)
        for c in range(nch):
            point[c] = pyref.add(point[c], adds[c])
            state[c] = got[c][0]
            for name, v, lim in zip(fm.RANGES, state[c], fm.RANGES.values()):
                assert fm.is_normalised(v) and below(v, lim, F.p), (kind, step, c, name, fm.ratio(F, v))
                note(f"{kind} chain", name, v, F.p, lim)
        if step % 64 == 63 or step == steps - 1:
            for c in range(nch):
                assert fm.xyzz_affine(tuple(state[c])) == point[c], (kind, step, c)
