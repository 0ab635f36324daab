"""CPU: the host's planning rules (csrc/msm_plan.hpp: overrides, window choice, accumulate / reduction geometry, the two sorts' geometry) against
the plain-integer models (tests/acc_model.py, tests/window_model.py).  tests/msm_plan_check.cpp is built with g++ under ASan + UBSan as a
stand-alone program, fed one case per line and compared line by line: this is where the model meets the host without a device
(tests/test_gpu_acc_geometry.py holds the two together through a real job)."""
import itertools
import os
import subprocess

import pytest

import acc_model as am
import window_model as wm
from conftest import ROOT

S2_OK, S2_TOO_WIDE, S2_COUNTERS = 0, 1, 2


@pytest.fixture(scope="module")
def check(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("msm_plan") / "msm_plan_check")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        os.path.join(ROOT, "tests", "msm_plan_check.cpp"), "-o", exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr

    def run(cases):
        """cases: [(words, {override: value})] -> one list of integers per case"""
        text = "".join(" ".join(str(w) for w in words) + "".join(" %s=%s" % kv for kv in over.items()) + "\n" for words, over in cases)
        r = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=600)       # the program clears the overrides itself, before every case
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
        lines = r.stdout.splitlines()
        assert lines[-1] == "MSM PLAN CHECK DONE" and len(lines) == len(cases) + 1
        return [ln.split() if words[0] == "const" else [int(x) for x in ln.split()] for ln, (words, _) in zip(lines, cases)]
    return run


def over(**kw):
    """{SBN_name: value} of the overrides that are set (None: unset)"""
    return {k: str(v) for k, v in kw.items() if v is not None}


def test_constants(check):
    got = dict(w.split("=") for w in check([(("const",), {})])[0])
    for name in ("MSM_C_MAX", "ACC_SEG_MAX", "MERGE_LANE_MAX", "S2_C_MAX"):
        assert int(got[name]) == getattr(am, name), name
    assert int(got["COMB_C_MAX"]) == wm.COMB_C_MAX
    assert [int(got[k]) for k in ("S2_C_MIN", "S2_P_MAX", "S2_LO_LOG_MAX", "S2_SPT", "S2_SPT_SMALL", "S2_SUB", "MODE_SINGLE", "MODE_ROWS")] == [13, 1024, 11, 8, 2, 16384, 0, 1]


def test_make_shape(check):
    cases = [(("shape", c, bits), {}) for c in range(7, 23) for bits in (254, 127)]
    for ((_, c, bits), _), got in zip(cases, check(cases)):
        s = wm.make_shape(c, bits)
        assert got == [c, s.W, s.nb], (c, bits)


TERMS = [1, 100, 511, 512, 513, 4096, 4097, 32768, 32769, 1 << 16, 1 << 19, (1 << 20) - 1, 1 << 20, 1 << 21, 1 << 22, 1 << 24, 1 << 26]


def test_choose_shape(check):
    keys = list(itertools.product(TERMS, (False, True), (0, 1, 2, 255, 256, 4096), ((15, 16), (16, 16), (22, 22)), (None, 6, 7, 16, 17, 22, 23)))
    cases = [(("choose", terms, int(shared), cmax, problems, chard), over(SBN_MSM_C=v)) for terms, shared, problems, (cmax, chard), v in keys]
    for (terms, shared, problems, (cmax, chard), v), got in zip(keys, check(cases)):
        want = v if v is not None and 7 <= v <= chard else am.choose_c(terms, shared, cmax, problems, chard)
        assert got == [want], (terms, shared, problems, cmax, chard, v)


def test_glv_shape(check):
    keys = list(itertools.product(range(10, 25), (None, 12, 13, 17, 18)))
    cases = [(("glv", 1 << k), over(SBN_MSM_C=v)) for k, v in keys]
    for (k, v), got in zip(keys, check(cases)):
        c = v if v is not None and 13 <= v <= 17 else am.glv_c(1 << k)
        assert got == [c, wm.make_shape(c, 127).W], (k, v)


def acc_case(mode, n, P, estride, c, seg=None, red_l=None):
    env = over(SBN_MSM_SEG=seg, SBN_RED_L=red_l)
    want = am.geometry(mode, n, P, estride, c, env)
    nb = 1 << (c - 1)
    max_extra = P * estride // want[0] + 1
    return (("acc", 0 if mode == am.SINGLE else 1, n, P, estride, nb), env), list(want) + [max_extra, min(P * nb, max_extra)]


def test_acc_plan(check):
    cases, wants = [], []
    for c in range(7, 23):
        W = wm.make_shape(c).W
        for n in (100, 511, 512, 3007, 3008, 4096, 4097, 90000, 1 << 20, 1 << 21):
            for mode, P, estride in [(am.SINGLE, W, n)] + [(am.ROWS, P, n * W) for P in (1, 5, 4096)]:
                for seg, red_l in itertools.product((None, 7, 8, 64, 8192, 8193), (None, 0, 1, 3, 64, 65)):
                    case, want = acc_case(mode, n, P, estride, c, seg, red_l)
                    cases.append(case); wants.append(want)
    for case, want, got in zip(cases, wants, check(cases)):
        assert got == want, case


def test_acc_plan_at_the_shipped_sizes(check):
    """am.shipped_jobs() through the host's rule is the table of DESIGN.md §4.0a (test_acc_model_cpu.py reads the table against the model)"""
    jobs = am.shipped_jobs()
    pairs = [acc_case(mode, n, P, estride, c) for _, mode, n, P, estride, c in jobs]
    got = check([case for case, _ in pairs])
    assert got == [want for _, want in pairs]
    assert {name: g[:6] for (name, *_), g in zip(jobs, got)} == {
        "2^20 GLV": [256, 2, 4, 128, 2, 1], "2^20 plain": [256, 2, 5, 52, 1, 1], "2^22 plain": [256, 1, 16, 64, 1, 1],
        "2^26 plain": [512, 1, 16, 512, 2, 0], "Hyrax 4096 x 2815": [64, 1, 16, 2, 1, 0]}


S2_N = [1024, 8193, 1 << 20, 1 << 21, (1 << 21) + 1, 1 << 22]


def test_sort2_plan_invariants(check):
    keys = list(itertools.product(range(13, 23), S2_N, (None, 4)))
    cases = [(("sort2", n, c, 254), over(SBN_SORT2_LO=lo)) for c, n, lo in keys]
    for (c, n, lo), (status, lo_log, P, spt, K, max_sc, W) in zip(keys, check(cases)):
        nb = 1 << (c - 1)
        assert status in (S2_OK, S2_COUNTERS) and W == wm.make_shape(c).W, (c, n, lo)
        assert P << lo_log == nb and P <= 1024 and lo_log <= 11
        assert spt in (2, 8) and K == -(-n // (1024 * spt))
        assert W * P * 4 <= 24 * 1024 * 4 or status == S2_COUNTERS
        assert max_sc == W * n // 16384 + W * P


def test_sort2_plan_values_and_overrides(check):
    def plan(n, c, bits=254, **kw):
        return check([(("sort2", n, c, bits), over(**kw))])[0][:5]
    # read off the rule: lo_log = max(c - 9, 8); P = 2^(c-1-lo_log); 2 scalars per thread while n <= 2^21 and P <= 64, else 8
    assert plan(1 << 20, 15) == [S2_OK, 8, 64, 2, 512]
    assert plan(1 << 22, 17) == [S2_OK, 8, 256, 8, 512]
    assert plan(1 << 21, 16, 127) == [S2_OK, 8, 128, 8, 256]          # 2^21 GLV records
    for lo in (3, 12):                                                 # out of range: ignored
        assert plan(1 << 20, 15, SBN_SORT2_LO=lo) == [S2_OK, 8, 64, 2, 512]
    assert plan(1 << 20, 15, SBN_SORT2_LO=4) == [S2_OK, 4, 1024, 8, 128]      # P > 64: the large blocks
    assert plan(1 << 20, 15, SBN_SORT2_LO=11) == [S2_OK, 11, 8, 2, 512]
    assert plan(1 << 22, 17, SBN_SORT2_SPT=2) == [S2_OK, 8, 256, 2, 2048]
    assert plan(1 << 20, 15, SBN_SORT2_SPT=8) == [S2_OK, 8, 64, 8, 128]
    assert plan(1 << 20, 15, SBN_SORT2_SPT=4) == [S2_OK, 8, 64, 2, 512] and plan(1 << 22, 17, SBN_SORT2_SPT=4) == [S2_OK, 8, 256, 8, 512]


def test_sort1_plan_invariants(check):
    keys = [(rs, c, P, cols) for rs in (16384, 32768) for c in range(7, 17) for P in (1, 5, 17, 4096) for cols in (1, 100, 4096, 4097, 90000, 1 << 20)]
    cases = [(("sort1", rs, P, cols, 1 << (c - 1)), {}) for rs, c, P, cols in keys]
    for (rs, c, P, estride), (RS, logRS, R, K, chunk) in zip(keys, check(cases)):
        nb = 1 << (c - 1)
        assert RS == min(nb, rs) == 1 << logRS and R * RS == nb, (rs, c, P, estride)
        assert K >= 1 and K * chunk >= estride
