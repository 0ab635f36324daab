"""CPU: the plans of the two device transcript steps (csrc/transcript_plan.hpp: transcript_plan_round, transcript_plan_boundary, the record
layout) executed in plain C++ the way k_tr_sumcheck_step and k_tr_layer_step consume them, against MerlinTranscript running the literal
operation sequence.  tests/transcript_plan_check.cpp includes the header alone, is built with g++ under ASan + UBSan as a stand-alone program
and fed one case per line; it compares every challenge's 64 bytes, the 200 sponge bytes at the end and end[3], and reports OK or FAIL per case.
Here: the sweep (every phase, every closing shape), and the block, challenge and source counts from byte counting alone.

Counts: 493 phases (every pos in 0..165 with pos_begin in {0, 1, pos - 1} where those lie in [0, pos - 1], plus 0); round plan 493 + 1 cases;
opening boundary 493 x 24 = 11832 cases; closing boundaries 300 shapes x up to 3 n_open = 876 cases."""
import os
import subprocess

import pytest

from conftest import ROOT

RATE = 166
FLAG_A, FLAG_IAC = 2, 7


def phases():
    out = []
    for pos in range(RATE):
        for pb in sorted({0} | {b for b in (1, pos - 1) if 0 <= b <= pos - 1}):
            out.append((pos, pb))
    return out


PHASES = phases()
SHAPES = [(nc, nd) for nc in range(1, 25) for nd in range(0, 25 - nc)]
assert len({p for p, _ in PHASES}) == 166 and len(PHASES) == 493 and len(set(PHASES)) == 493
assert len(set(SHAPES)) == 300


@pytest.fixture(scope="module")
def check(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("transcript_plan") / "transcript_plan_check")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        os.path.join(ROOT, "tests", "transcript_plan_check.cpp"), "-o", exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr

    def run(cases):
        """cases: [[word, ...]] -> one list of integers per case (behind its OK); any FAIL line, sanitizer report or other exit fails here"""
        text = "".join(" ".join(str(w) for w in case) + "\n" for case in cases)
        r = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=600)
        lines = r.stdout.splitlines()
        bad = [(case, ln) for case, ln in zip(cases, lines) if not ln.startswith("OK ")]
        assert not bad, "%d of %d cases, the first: %s" % (len(bad), len(cases), bad[:5])
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
        assert lines[-1] == "TRANSCRIPT PLAN CHECK DONE" and len(lines) == len(cases) + 1
        return [[int(x) for x in ln.split()[1:]] for ln in lines[:-1]]
    return run


def count_blocks(pos, ops):
    """permutations of a sequence of Merlin operations from `pos`, by byte counting: ("msg", label_len, n) = append_message of n bytes,
    ("chal", label_len) = challenge_bytes of 64 -> (blocks, per challenge the blocks completed when it is read, the final pos)"""
    blocks, chal = 0, []

    def absorb(n):
        nonlocal pos, blocks
        blocks += (pos + n) // RATE
        pos = (pos + n) % RATE
    for op in ops:
        absorb(2 + op[1] + 4)                     # meta_ad(label), meta_ad(length, more)
        absorb(2)                                 # the operation's header
        if op[0] == "msg":
            absorb(op[2])
        else:
            if pos:                               # an operation with C starts on a fresh block
                blocks += 1
            pos = 64
            chal.append(blocks)
    return blocks, chal, pos


def boundary_ops(nc, nd, n_open):
    ops = []
    if nc:
        ops += [("msg", len("claim_prod_left"), 32), ("msg", len("claim_prod_right"), 32)] * nc
        ops += [("msg", len("claim_dotp_left"), 32), ("msg", len("claim_dotp_right"), 32), ("msg", len("claim_dotp_weight"), 32)] * nd
        ops.append(("chal", len("challenge_r_layer")))
    return ops + [("chal", len("rand_coeffs_next_layer"))] * n_open


ROUND_OPS = [("msg", 4, 13)] + [("msg", 5, 32)] * 4 + [("msg", 4, 11), ("chal", 19)]


def test_round_plan_every_phase(check):
    cases = [("round", pos, pb, FLAG_A, 1000 + 7 * pos + pb) for pos, pb in PHASES] + [("round", 64, 0, FLAG_IAC, 5)]
    assert len(cases) == 494
    for (_, pos, pb, _, _), got in zip(cases, check(cases)):
        nblk, chal, end = count_blocks(pos, ROUND_OPS)
        assert chal == [nblk] and nblk == (2 if pos <= 77 else 3)
        assert got == [nblk, end, 0, FLAG_IAC] and end == 64, (pos, pb)


OPEN_CHUNKS = [range(1 + 6 * chunk, 7 + 6 * chunk) for chunk in range(4)]
assert sorted(n for opens in OPEN_CHUNKS for n in opens) == list(range(1, 25))


@pytest.mark.parametrize("chunk", range(4))
def test_opening_boundary_every_phase(check, chunk):
    """the first step of a product proof: nothing closes, n_open coefficients are drawn from the caller's phase"""
    opens = OPEN_CHUNKS[chunk]
    cases = [("bound", pos, pb, FLAG_A, 0, 0, n_open, 2000 + 31 * pos + 7 * pb + n_open) for pos, pb in PHASES for n_open in opens]
    assert len(cases) == 493 * 6
    for (_, pos, pb, _, _, _, n_open, _), got in zip(cases, check(cases)):
        nblk, chal, end = count_blocks(pos, boundary_ops(0, 0, n_open))
        assert chal[-1] == nblk and len(set(chal)) == n_open
        assert got == [nblk, end, 0, FLAG_IAC, n_open, 0] and end == 64, (pos, pb, n_open)


def test_closing_boundary_every_shape(check):
    """every later step: from behind a PRF (64, 0, I|A|C) it closes n_close circuits + n_dotp dot products and opens nothing (the last step),
    the circuits again (a middle layer) or everything (the layer that brings the dot products in)"""
    cases = []
    for nc, nd in SHAPES:
        for n_open in sorted({0, nc, nc + nd}):
            cases.append(("bound", 64, 0, FLAG_IAC, nc, nd, n_open, 3000 + 97 * nc + 5 * nd + n_open))
    assert len({(c[4], c[5]) for c in cases}) == 300 and len(cases) == 300 + 300 + 276
    for (_, _, _, _, nc, nd, n_open, _), got in zip(cases, check(cases)):
        nblk, chal, end = count_blocks(64, boundary_ops(nc, nd, n_open))
        assert chal[-1] == nblk and len(set(chal)) == 1 + n_open
        assert got == [nblk, end, 0, FLAG_IAC, 1 + n_open, 32 * (2 * nc + 3 * nd)] and end == 64, (nc, nd, n_open)


def test_closing_boundary_from_other_phases(check):
    """the planner takes any phase: a closing step from a sample of them (the library only starts one at 64, 0)"""
    cases = [("bound", pos, pb, FLAG_A, nc, nd, nc + nd, 4000 + pos + nc) for pos, pb in PHASES[::7] for nc, nd in ((1, 0), (3, 2), (18, 6), (1, 23))]
    for (_, pos, pb, _, nc, nd, n_open, _), got in zip(cases, check(cases)):
        nblk, chal, end = count_blocks(pos, boundary_ops(nc, nd, n_open))
        assert got == [nblk, end, 0, FLAG_IAC, 1 + n_open, 32 * (2 * nc + 3 * nd)], (pos, pb, nc, nd)
