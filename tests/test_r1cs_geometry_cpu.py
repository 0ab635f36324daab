"""CPU: tests/r1cs_geometry.py — the replay of the merge-path layout of csrc/r1cs_kernels.cuh and the instances built on it.
  - its constants are the kernel's (a retune of the kernel fails here first: the instances must then be derived again);
  - every instance hits the seam classes it is built for (conditions on the instances, asserted through classes(), never skipped);
  - the replay, through chunks, carries and fix-up passes, computes what r1cs_model.py computes, on every instance: the class labels are labels
    of an algorithm that gives the right result.
tests/test_gpu_r1cs_seams.py runs the same instances on the device."""
import os
import random
import re

import pytest

import r1cs_geometry as g
import r1cs_model as rm
from conftest import PKG_DIR

R = rm.R
NAMES = sorted(g.instances())


def _kernel_source():
    with open(os.path.join(PKG_DIR, "csrc", "r1cs_kernels.cuh")) as f:
        return f.read()


def _rand(n, seed):
    rng = random.Random(seed)
    return [rng.randrange(R) for _ in range(n)]


def _classes(name):
    nc, nv, mats = g.instances()[name][:3]
    return tuple(g.classes(lay) for lay in g.layouts(nc, nv, mats))


def test_constants_mirror_the_kernel():
    src = _kernel_source()
    msg = "csrc/r1cs_kernels.cuh was retuned: set the constant in tests/r1cs_geometry.py and derive the instances again (every class test below)"
    for name in ("R1CS_CHUNK", "R1CS_FIX_FIRST", "R1CS_FIX_CHUNK"):
        found = re.findall(r"constexpr\s+uint32_t\s+%s\s*=\s*(\d+)\s*;" % name, src)
        assert len(found) == 1 and int(found[0]) == getattr(g, name), f"{name}: {msg}"
    found = re.findall(r"if\s*\(\s*\+\+pend\s*==\s*(\d+)\s*\)", src)
    assert len(found) == 1 and int(found[0]) == g.CARRY_CADENCE, f"the carry cadence: {msg}"
    assert g.CARRY_CADENCE in g.CADENCE_COUNTS and 2 * g.CARRY_CADENCE in g.CADENCE_COUNTS
    assert {g.CARRY_CADENCE, g.R1CS_CHUNK, 2 * g.R1CS_CHUNK} <= set(g.LENGTHS)


def test_layout_of_a_hand_made_list():
    """3 rows of 2, 0 and 17 non-zeros: 22 items, two chunks; written out by hand from the definition (row end g is item row_end[g] + g)"""
    lay = g.layout(3, [2, 0, 17])
    assert (lay.nnz, lay.row_end, lay.nchunks, lay.start_row) == (19, [2, 2, 19], 2, [0, 2, 3])
    # chunk 0: nz nz END0 END1 and 12 non-zeros of row 2 -> carry (2, True); chunk 1: 5 non-zeros of row 2, END2 -> carry (3, False)
    assert lay.chunks[0] == g.Chunk([(0, 0, 2, True), (1, 2, 0, True), (2, 2, 12, False)], [0, 1], (2, True))
    assert lay.chunks[1] == g.Chunk([(2, 14, 5, True)], [2], (3, False))
    assert {("row", 0, 2), ("row", 3, 0), ("row", 4, 17), ("long_row", 2), ("cadence", 2), ("cadence_carry", 12), ("cadence_tail", 5), ("carry_run", 0, 1),
            ("last_chunk_items", 6), ("chunks", 2), ("passes", 1)} <= g.classes(lay)


def test_fix_passes_of_a_hand_made_key_list():
    """9 carries: lanes of 4 -> 3 carries -> one lane of 32"""
    p = g.fix_passes([0, 0, 0, 1, 1, 1, 1, 1, 5])
    assert len(p) == 2 and [(q["n"], q["F"]) for q in p] == [(9, 4), (3, 32)]
    assert p[0]["lanes"] == [dict(range=(0, 4), adds=[(0, 0, 3)], hands_on=(1, 3, 4)), dict(range=(4, 8), adds=[], hands_on=(1, 4, 8)),
                             dict(range=(8, 9), adds=[], hands_on=(5, 8, 9))]
    assert p[1]["keys"] == [1, 1, 5] and p[1]["lanes"] == [dict(range=(0, 3), adds=[(1, 0, 2), (5, 2, 3)], hands_on=None)]
    # n -> ceil(n / 4) -> ceil(n / 32) -> ... until one lane is left
    for n, want in zip(g.CHUNK_COUNTS, (1, 1, 2, 2, 3, 3, 4)):
        assert len(g.fix_passes([0] * n)) == want, n


@pytest.mark.parametrize("axis", ["rows", "cols"])
def test_offsets_by_lengths_hits_every_pair(axis):
    seq = g.offset_length_sequence()
    assert (len(seq), sum(seq)) == (16 * len(g.LENGTHS), 16 * sum(g.LENGTHS)) == (208, 2864)
    designed = _classes(f"offsets_{axis}")[axis == "cols"]
    missing = {("row", o, n) for o in range(g.R1CS_CHUNK) for n in g.LENGTHS} - designed
    assert not missing, missing
    nc, nv = g.instances()[f"offsets_{axis}"][:2]
    assert (nc, nv) == ((128, 64) if axis == "rows" else (g.MIN_CONS, 128))


@pytest.mark.parametrize("name", sorted(g.SEAM_VARIANTS))
def test_matrix_seams_hit_every_named_seam(name):
    mod, row0 = g.SEAM_VARIANTS[name]
    nc, nv, mats = g.instances()[name][:3]
    rowc, colc = _classes(name)
    want = {("shared_chunk", 0), ("shared_chunk", 1), ("last_row_nonempty", 0), ("last_row_nonempty", 1), ("last_row_nonempty", 2),
            ("last_chunk_items", mod or g.R1CS_CHUNK), ("row0_nonempty",) if row0 else ("row0_empty",), ("chunk_of_row_ends",)}
    assert want <= rowc, want - rowc
    assert {("long_row", nv), ("long_row", 2 * nv - 1)} <= colc
    lay = g.layouts(nc, nv, mats)[0]
    assert (lay.nrows + lay.nnz) % g.R1CS_CHUNK == mod and lay.chunks[-1].carry == (3 * nc, False)
    assert all(lay.row_end[2 * nc + i] > lay.row_end[2 * nc + i - 1] for i in range(nc)), "every row of C holds a non-zero (tuned() needs one)"


def test_degenerate_sets():
    assert ("single_row",) in _classes("one_row")[0]
    assert ("single_row",) in _classes("one_col")[1]
    assert all(("single_nonzero",) in c for c in _classes("one_nonzero"))


@pytest.mark.parametrize("n0,launches", list(zip(g.CHUNK_COUNTS, (1, 1, 2, 2, 3, 3, 4))))
def test_chunk_counts_hit_their_chunk_and_pass_counts(n0, launches):
    nc, nv, mats = g.instances()[f"chunks_{n0}"][:3]
    assert nc == g.MIN_CONS
    lay = g.layouts(nc, nv, mats)[0]
    cls = g.classes(lay)
    passes = g.fix_passes([ch.carry[0] for ch in lay.chunks])
    assert lay.nchunks == n0 and ("chunks", n0) in cls
    assert len(passes) == launches and ("passes", launches) in cls
    longest = max((c[2] for c in cls if c[0] == "carry_run"), default=0)
    assert longest >= n0 // 2, "one row over at least n0 // 2 chunks"
    # a run lies across two lane ranges in every pass that can have one: the last carry of every pass is the dropped one (key nrows), so a pass of
    # F + 1 carries has a second lane that holds nothing else
    for p, ps in enumerate(passes, 1):
        if ps["n"] > ps["F"] + 1:
            assert ("fix_run_crosses", p) in cls, (n0, p)


def test_run_alignments_hit_every_start_and_span():
    rowc = _classes("run_alignments")[0]
    missing = {("carry_run", a, n) for a in range(g.R1CS_FIX_FIRST) for n in g.RUN_SPANS} - rowc
    assert not missing, missing
    assert {("fix_run_crosses", 2), ("fix_run_crosses_off_edge", 2), ("run_boundary", "lane_edge"), ("run_boundary", "inside_lane"), ("passes", 3)} <= rowc
    assert max(c[2] for c in rowc if c[0] == "carry_run") >= g.BIG_RUN


def test_cadence_hits_every_count():
    rowc = _classes("cadence")[0]
    want = {(kind, n) for kind in ("cadence", "cadence_tail", "cadence_carry") for n in g.CADENCE_COUNTS}
    assert want <= rowc, want - rowc


def test_saturated_sets_are_what_they_say():
    inst = g.instances()
    nc, nv, mats, z = inst["offsets_rm1"]
    assert all(v == R - 1 for m in mats for v in m[2]) and z == [R - 1] * (2 * nv)
    assert [m[:2] for m in mats] == [m[:2] for m in inst["offsets_rows"][2]]
    for name, stored in (("carry_rm1", 0), ("carry_rm1_stored", R - 1)):
        nc, nv, mats, z = inst[name]
        rowm, _ = g.csr_copies(nc, nv, mats)
        lay = g.layout(rowm.nrows, rowm.lengths, nc)
        assert rowm.lengths[0] == g.SAT_ROW + (stored != 0) and sum(rowm.lengths[1:]) == 0 and set(z) == {1}
        full = g.SAT_ROW // g.R1CS_CHUNK
        for ch in lay.chunks[:full]:                                    # every chunk of the row leaves the carry r - 1
            (row, first, cnt, ended), = ch.segs
            assert (row, cnt, ended, ch.carry) == (0, g.R1CS_CHUNK, False, (0, True))
            assert sum(rowm.val[first:first + cnt]) == R - 1
        assert sum(rowm.val[full * g.R1CS_CHUNK:]) == stored            # what the row's own lane stores
        passes = g.fix_passes([ch.carry[0] for ch in lay.chunks])
        assert len(passes) == 3 and passes[1]["lanes"][0]["hands_on"] == (0, 0, g.R1CS_FIX_CHUNK), "a second-pass lane sums 32 sums of 4 carries"


def test_tuned_changes_values_only_and_violates_what_it_is_told():
    for name in ["offsets_rows"] + sorted(g.SEAM_VARIANTS):
        nc, nv, mats = g.instances()[name][:3]
        z = _rand(nv, 1) + [1] + _rand(nv - 1, 2)
        bad = [0, nc // 2 + 1, nc - 1]
        for violate in ([], bad):
            t = g.tuned(nc, nv, mats, z, violate)
            assert [m[:2] for m in t] == [(list(m[0]), list(m[1])) for m in mats]
            Az, Bz, Cz = rm.multiply_vec(nc, nv, t, z)
            assert [i for i in range(nc) if (Az[i] * Bz[i] - Cz[i]) % R] == violate


@pytest.mark.parametrize("name", NAMES)
def test_replay_is_the_geometry(name):
    nc, nv, mats, z = g.instances()[name]
    z = z or _rand(2 * nv, 3)
    assert g.replay_multiply(nc, nv, mats, z) == rm.multiply_vec(nc, nv, mats, z)
    lx, ly = nc.bit_length() - 1, (2 * nv).bit_length() - 1
    rx, ry, (rA, rB, rC) = _rand(lx, 4), _rand(ly, 5), _rand(3, 6)
    assert g.replay_eval_table(nc, nv, mats, rx, rA, rB, rC) == rm.eval_table(nc, nv, mats, rx, rA, rB, rC)
    assert g.replay_evaluate(nc, nv, mats, rx, ry) == rm.evaluate(nc, nv, mats, rx, ry)
