"""CPU: the model of the accumulate geometry (tests/acc_model.py) is consistent with itself, its builders land on the loads they are
asked for, and the geometry it gives at the shipped sizes is the one DESIGN.md states.  tests/test_gpu_acc_geometry.py holds the
model against the host's run_bucket_job and the device's counters through a real job; tests/test_msm_plan_cpu.py is where the model meets the
host's rules (csrc/msm_plan.hpp) without a device, over their whole range."""
import os
import random
import re

import pytest

import acc_model as am
import window_model as wm
from test_glv_cpu import LAM, split

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEGS = [8, 32, 64, 256, 8192]


def counts_to_check(SEG):
    out = set(range(0, 3 * SEG + 2))
    for m in (13, 14, 65):
        out |= set(range(m * SEG - 2, m * SEG + 3))
    return sorted(out)


@pytest.mark.parametrize("G", [1, 2])
@pytest.mark.parametrize("SEG", SEGS)
def test_cut_partitions_a_bucket_exactly_once(SEG, G):
    for cnt in counts_to_check(SEG):
        parts, k, extras, path = am.cut(cnt, SEG, G)
        assert len(parts) == G and len(extras) == k
        pos = 0
        for fr, to in parts + extras:                        # in order, contiguous, none longer than a segment
            assert fr == pos and fr <= to and to - fr <= SEG, (cnt, fr, to)
            pos = to
        assert pos == cnt
        assert sum(to - fr for fr, to in parts) == min(cnt, SEG)
        assert all(to - fr == SEG for fr, to in extras[:-1]) and all(to > fr for fr, to in extras)
        assert path == ("none" if cnt <= SEG else "lane" if cnt <= 13 * SEG else "wave")
        assert am.expected_counters([cnt], SEG) == (k, 1 if k else 0)
        assert am.merge_paths([cnt], SEG) == (int(path == "lane"), int(path == "wave"))
        if G == 2:                                           # the second lane's part: empty for one entry, one shorter for an odd segment
            a, b = (to - fr for fr, to in parts)
            assert a - b == min(cnt, SEG) % 2


def test_cut_names_the_seams_of_the_load_set():
    for SEG in SEGS:
        ks = {t: am.cut(t, SEG, 2) for t in am.load_set(SEG)}
        assert [ks[t][1] for t in (SEG - 1, SEG, SEG + 1, 2 * SEG, 2 * SEG + 1)] == [0, 0, 1, 1, 2]
        assert ks[SEG + 1][2] == [(SEG, SEG + 1)] and ks[2 * SEG][2] == [(SEG, 2 * SEG)]
        assert ks[1][0] == [(0, 1), (1, 1)] and ks[3][0] == [(0, 2), (2, 3)]
        if SEG < am.ACC_SEG_MAX:
            assert (ks[13 * SEG][1], ks[13 * SEG][3]) == (12, "lane") and ks[13 * SEG][2][-1] == (12 * SEG, 13 * SEG)
            assert (ks[13 * SEG + 1][1], ks[13 * SEG + 1][3]) == (13, "wave") and ks[13 * SEG + 1][2][-1] == (13 * SEG, 13 * SEG + 1)
            assert (ks[65 * SEG + 1][1], ks[65 * SEG + 1][3]) == (65, "wave")
        assert len(am.load_set(SEG)) == (13 if SEG < am.ACC_SEG_MAX else 10)


@pytest.mark.parametrize("c,bits", [(7, 254), (8, 254), (9, 254), (12, 254), (13, 254), (16, 254), (20, 254), (13, 127), (16, 127)])
def test_edge_scalars_land_on_their_loads(c, bits):
    s = wm.make_shape(c, bits)
    windows = [0, s.W // 2, s.W - 1]
    for SEG in (8, 64):
        background = am.loads_of(am.masked_uniform(300, 5 * c + SEG, c, windows, bits), c, s.W)
        assert not any(w in windows for w, _ in background)          # the filler leaves the requested windows alone
        sc, plan = am.edge_plan(c, s.W, SEG, windows, background, bits)
        assert all(0 <= k < wm.bound_of(bits) for k in sc)
        loads = am.loads_of(sc, c, s.W)
        for w in windows:
            want = am.window_loads(c, s.W, w, SEG, bits)
            assert len(want) == min(13, sum(am.usable_buckets(c, s.W, w, bits))) and len(want) >= 3
            assert {65 * SEG + 1, 13 * SEG + 1, 13 * SEG} <= set(want)
            assert sorted(plan[w]) == sorted(want)
            for t, b in plan[w].items():
                assert loads.get((w, b), 0) == t, (w, b, t)
            assert plan[w][max(want)] == 0                           # bucket 0 ...
            if w < s.W - 1:
                assert (1 << (c - 1)) - 1 in plan[w].values()        # ... and the window's last bucket are among the chosen ones
        # nothing else is loaded but bucket 0 of the window above a last bucket (the carry of -2^(c-1))
        assert {k for k in loads if k[0] not in windows} <= {(w + 1, 0) for w in windows}


def test_edge_scalars_top_up_a_background():
    c, SEG = 12, 32
    s = wm.make_shape(c)
    rnd = random.Random(12)
    fill = [rnd.randrange(wm.R) for _ in range(3000)]
    background = am.loads_of(fill, c, s.W)
    sc, plan = am.edge_plan(c, s.W, SEG, [0, 9], background)
    loads = am.loads_of(fill + sc, c, s.W)
    for w in (0, 9):
        assert sorted(plan[w]) == sorted(am.load_set(SEG))
        assert all(loads.get((w, b), 0) == t for t, b in plan[w].items())
    total = am.expected_counters(loads, SEG)
    assert total[1] >= 2 * 9 and total[0] >= 2 * (1 + 1 + 2 + 12 + 13 + 65)


def test_glv_edge_scalars_split_into_their_halves():
    """the full scalars glv_scalars makes of edge halves decompose (model of the kernel's glv_split) into exactly those halves"""
    for c in (13, 16):
        s = wm.make_shape(c, 127)
        halves = am.edge_scalars(c, s.W, 8, [0, s.W // 2, s.W - 1], bits=127)
        ks = am.glv_scalars(halves, c, s.W, LAM, wm.R)
        got = [h for k in ks for h in split(k) if h]
        assert sorted(got) == sorted(halves)
        assert sum(1 for k in ks if split(k)[1]) >= 100 * 8            # a whole window's set travels as second halves
        assert am.loads_of(got, c, s.W) == am.loads_of(halves, c, s.W)


def test_row_columns_land_on_their_loads():
    c, SEG = 8, 64
    s = wm.make_shape(c)
    fill = am.digit_range_columns(500, 3, c, s.W, 65, 126)
    background = {b: t for (_, b), t in am.loads_of_rows([fill], c, s.W).items()}
    assert min(background) >= 64 and max(background) <= 125
    cols, plan = am.row_edge_columns(c, s.W, SEG, am.load_set(SEG), background)
    loads = am.loads_of_rows([fill + cols], c, s.W)
    assert sorted(plan) == sorted(am.load_set(SEG)) and plan[65 * SEG + 1] == 0 and plan[13 * SEG + 1] == 127
    assert all(loads.get((0, b), 0) == t for t, b in plan.items())
    assert len(cols) < 1500


@pytest.mark.parametrize("c,bits,width", [(7, 254, 32), (12, 254, 32), (15, 254, 32), (16, 254, 32), (17, 254, 32), (20, 254, 32), (13, 127, 16), (16, 127, 16)])
def test_numpy_loads_match_the_integer_model(c, bits, width):
    s = wm.make_shape(c, bits)
    rnd = random.Random(c)
    sc = wm.seam_scalars(c, bits) + [rnd.randrange(wm.bound_of(bits)) for _ in range(500)] + am.edge_scalars(c, s.W, 8, [0, s.W - 1], bits=bits)
    arr = am.loads_of_bytes(b"".join(k.to_bytes(width, "little") for k in sc), c, s.W, width)
    want = am.loads_of(sc, c, s.W)
    assert arr.shape == (s.W, s.nb) and int(arr.sum()) == sum(want.values())
    assert all(arr[w, b] == t for (w, b), t in want.items())
    assert am.expected_counters(arr, 8) == am.expected_counters(want, 8)


def test_geometry_at_the_shipped_sizes_is_sane_and_documented():
    doc = open(os.path.join(ROOT, "DESIGN.md")).read()
    jobs = am.shipped_jobs()
    assert [(name, c) for name, _, _, _, _, c in jobs] == [("2^20 GLV", 16), ("2^20 plain", 15), ("2^22 plain", 17), ("2^26 plain", 20), ("Hyrax 4096 x 2815", 12)]
    for name, mode, n, P, estride, c in jobs:
        SEG, LPB, L, chunks, levels, quad = am.geometry(mode, n, P, estride, c)
        nb = 1 << (c - 1)
        assert 32 <= SEG <= am.ACC_SEG_MAX and SEG & (SEG - 1) == 0
        assert SEG >= 2 * (estride // nb)                        # a uniformly loaded bucket stays inside its first segment
        assert LPB in (1, 2) and 1 <= L <= 32
        assert chunks * 64 * L >= nb > (chunks - 1) * 64 * L
        assert 64 ** (levels - 1) < max(chunks, 2) <= 64 ** levels
        assert quad == (P * chunks <= 2048)
        row = re.search(r"^\| %s \|([^\n]*)\|$" % re.escape(name), doc, flags=re.M)
        assert row, "DESIGN.md has no row for " + name
        cells = [x.strip() for x in row.group(1).split("|")]
        assert cells[:8] == [str(c), str(P), str(SEG), str(LPB), str(L), str(chunks), str(levels), "quad" if quad else "plain"], (name, cells)


def test_geometry_overrides_and_the_small_msm_rule():
    W7, W12 = wm.make_shape(7).W, wm.make_shape(12).W
    assert am.geometry(am.SINGLE, 511, W7, 511, 7)[0] == 32 and am.geometry(am.SINGLE, 512, W7, 512, 7)[0] == 8
    assert am.geometry(am.SINGLE, 4096, W7, 4096, 7)[0] == 8 and am.geometry(am.SINGLE, 4097, W7, 4097, 7)[0] == 32
    assert am.geometry(am.ROWS, 3000, 3, 3000 * 32, 8)[:2] == (32, 1)                  # rows: never 8 by the rule, never two lanes
    assert am.geometry(am.SINGLE, 3007, W7, 3007, 7)[:2] == (8, 1) and am.geometry(am.SINGLE, 3008, W7, 3008, 7)[:2] == (8, 2)
    for seg in (8, 64, 8192):
        assert am.geometry(am.SINGLE, 90000, W12, 90000, 12, {"SBN_MSM_SEG": str(seg)})[:2] == (seg, 1)
    assert am.geometry(am.SINGLE, 90000, W12, 90000, 12, {"SBN_MSM_SEG": "7"})[0] == 32     # out of range: ignored
    assert am.geometry(am.SINGLE, 47 * 2048, W12, 47 * 2048, 12)[1] == 2 and am.geometry(am.SINGLE, 47 * 2048 - 1, W12, 47 * 2048 - 1, 12)[1] == 1
    W20 = wm.make_shape(20).W
    assert am.geometry(am.SINGLE, 10277, W20, 10277, 20, {"SBN_RED_L": "1"})[2:] == (1, 8192, 3, 0)
    assert am.geometry(am.SINGLE, 10277, W20, 10277, 20, {"SBN_RED_L": "64"})[2:] == (64, 128, 2, 1)
