"""CPU: the window recoding model (tests/window_model.py) and the seam scalars the GPU width tests feed every path with.
For every width a path accepts: both recodings reconstruct the scalar, the digits stay in their ranges, the two rules differ only at
the documented corner, and the seam set really lands on every named corner — if it stopped doing so this file fails first."""
import random

import pytest

import window_model as wm

CASES = [(c, 254) for c in range(7, 23)] + [(c, 127) for c in range(13, 18)]


def _uniform(bits, n, seed):
    rnd = random.Random(seed)
    return [rnd.randrange(wm.bound_of(bits)) for _ in range(n)]


def test_make_shape_known_values():
    """the shapes the code comments quote: 254 = 16 x 15 + 14 (17 windows), c = 16 -> 16, c = 17 -> 15, c = 7 -> 37; GLV: 8 x 16, 127 = 7 x 16 + 15"""
    assert [(c, wm.make_shape(c).W) for c in (7, 11, 13, 15, 16, 17, 20, 22)] == [(7, 37), (11, 24), (13, 20), (15, 17), (16, 16), (17, 15), (20, 13), (22, 12)]
    assert [wm.make_shape(c, 127).W for c in range(13, 18)] == [10, 10, 9, 8, 8]
    for c, bits in CASES:
        s = wm.make_shape(c, bits)
        assert s.nb == 1 << (c - 1) and c * s.W >= bits and bits - c * (s.W - 1) <= c - 1       # the top window holds at most c - 1 bits


@pytest.mark.parametrize("c,bits", CASES)
def test_recodings_reconstruct_and_stay_in_range(c, bits):
    s = wm.make_shape(c, bits); half = s.nb
    seams = wm.seam_scalars(c, bits)
    assert len(set(seams)) == len(seams) and all(0 <= k < wm.bound_of(bits) for k in seams)
    for k in seams + _uniform(bits, 1000, 100 * c + bits):
        seq, carry = wm.recode_sequential(k, c, s.W)
        ind = wm.recode_independent(k, c, s.W)
        assert carry == 0, hex(k)                                                           # nothing is lost above the top window
        assert sum(d << (c * w) for w, d in enumerate(seq)) == k, hex(k)
        assert sum(d << (c * w) for w, d in enumerate(ind)) == k, hex(k)
        assert all(-half <= d < half for d in seq), hex(k)
        assert all(-half <= d <= half for d in ind), hex(k)
        assert 0 <= seq[-1] <= wm.max_top_digit(c, bits) and 0 <= ind[-1] <= wm.max_top_digit(c, bits), hex(k)    # the top digit: never negative, never above the maximum


@pytest.mark.parametrize("c,bits", CASES)
def test_rules_differ_only_at_the_corner(c, bits):
    """corner = a raw window of 2^(c-1) - 1 that receives a carry.  There the sequential digit is -2^(c-1); the independent one is +2^(c-1)
    (2^(c-1) - 1 inside a run of corners, whose carry the independent rule does not see); the window after a corner is one larger under
    the sequential rule.  Every other digit is the same."""
    s = wm.make_shape(c, bits); half = s.nb
    differing = 0
    for k in wm.seam_scalars(c, bits) + _uniform(bits, 1000, 7 * c + bits):
        seq, _ = wm.recode_sequential(k, c, s.W)
        ind = wm.recode_independent(k, c, s.W)
        corners = set(wm.corner_windows(k, c, s.W))
        for w in range(s.W):
            if w in corners:
                assert seq[w] == -half and ind[w] == (half - 1 if w - 1 in corners else half), (hex(k), w)
                differing += 1
            elif w - 1 in corners:
                assert seq[w] == ind[w] + 1, (hex(k), w)
            else:
                assert seq[w] == ind[w], (hex(k), w)
        assert [w for w in range(s.W) if ind[w] == half] == [w for w in sorted(corners) if w - 1 not in corners], hex(k)
    assert differing


@pytest.mark.parametrize("c,bits", CASES)
def test_seam_set_hits_every_named_corner(c, bits):
    s = wm.make_shape(c, bits); half, full, W = s.nb, (1 << c) - 1, s.W
    seams = wm.seam_scalars(c, bits)
    bound = wm.bound_of(bits)
    assert {0, 1, bound - 1, bound - 2} <= set(seams)
    seq = {k: wm.recode_sequential(k, c, W)[0] for k in seams}
    ind = {k: wm.recode_independent(k, c, W) for k in seams}
    raws = {k: wm.raw_windows(k, c, W) for k in seams}
    for w in range(W):
        # 2^(c w): digit 1 alone; 2^(c w + c - 1): raw 2^(c-1), sequential -2^(c-1) with a carry into w + 1; all ones up to the window's end
        if w < W - 1 or (1 << (c * w)) < bound:
            assert (1 << (c * w)) in seq and seq[1 << (c * w)][w] == 1
        if w < W - 1:
            k = 1 << (c * w + c - 1)
            assert seq[k][w] == -half and seq[k][w + 1] == 1 and ind[k][w] == -half and ind[k][w + 1] == 1
            k = (1 << (c * w + c)) - 1
            assert raws[k][:w + 1] == [full] * (w + 1) and seq[k][w + 1] == 1 and seq[k][0] == -1
        # the corner in window w: +2^(c-1) under the independent rule (the last entry of a table column), -2^(c-1) and a carry under the sequential one
        if wm.corner_feasible(c, w, bits):
            hit = [k for k in seams if ind[k][w] == half]
            assert hit, (c, bits, w)
            assert all(seq[k][w] == -half and (seq[k][w + 1] - ind[k][w + 1]) % (1 << c) == 1 for k in hit)     # ... which the next window takes in
            assert {raws[k][w - 1] for k in hit} >= {half, full}                            # carried into by a raw 2^(c-1) and by all ones
        else:
            assert w == 0 or w == W - 1                                                      # only the ends can be out of reach
            assert not any(d[w] == half for d in ind.values())
    # the maximal top digit: the largest scalar has it, and the all-ones carry chain reaches the top window as well
    top = wm.max_top_digit(c, bits)
    assert seq[bound - 1][-1] == top == max(d[-1] for d in seq.values()) and 0 < top < half
    k = wm.carried_top_scalar(c, bits)
    assert k in seq and seq[k][-1] == ind[k][-1] == raws[k][-1] + 1 and seq[k][0] == -1 and set(seq[k][1:-1]) <= {0}
    # every window 2^(c-1) / all ones (below the bound), and a run of corners through every window above the lowest
    assert any(all(r == half for r in raws[k][:W - 1]) for k in seams)
    assert any(all(r == full for r in raws[k][:W - 1]) for k in seams)
    run = max(seams, key=lambda k: len(wm.corner_windows(k, c, W)))
    assert len(wm.corner_windows(run, c, W)) >= W - 2 and ind[run][1] == half and ind[run][2] == half - 1
    # both signs of the extreme digits occur in every window below the top: bucket 2^(c-1) (index nb - 1) is reached in each of them
    for w in range(W - 1):
        assert any(d[w] == -half for d in seq.values()) and any(d[w] == half - 1 for d in seq.values()), (c, bits, w)


@pytest.mark.parametrize("c,bits", [(7, 254), (16, 254), (17, 254), (22, 254), (16, 127)])
def test_a_wrong_recoding_is_caught(c, bits, monkeypatch):
    """the checks above are not vacuous: an off-by-one in the carry bit of the independent rule, a top-window mask one bit short and a
    recentring threshold off by one all break the reconstruction on the seam set of the width"""
    s = wm.make_shape(c, bits)
    seams = wm.seam_scalars(c, bits)

    def rebuilt(digits):
        return sum(d << (c * w) for w, d in enumerate(digits))

    def carry_bit_off_by_one(k):
        out = []
        for w, raw in enumerate(wm.raw_windows(k, c, s.W)):
            carry = (k >> (c * w)) & 1 if w else 0                # bit c w instead of c w - 1
            out.append(raw + carry - (1 << c) if raw >> (c - 1) else raw + carry)
        return out

    def short_mask(k):
        half, carry, out = 1 << (c - 1), 0, []
        for raw in wm.raw_windows(k, c, s.W):
            d = (raw & ((1 << (c - 1)) - 1)) + carry              # a window mask of c - 1 bits
            carry = 1 if d >= half else 0
            out.append(d - (1 << c) if carry else d)
        return out

    def threshold_off_by_one(k):
        half, carry, out = 1 << (c - 1), 0, []
        for raw in wm.raw_windows(k, c, s.W):
            d = raw + carry
            carry = 1 if d > half else 0                          # > instead of >=: the digit 2^(c-1) stays positive and overflows the buckets
            out.append(d - (1 << c) if carry else d)
        return out

    assert any(rebuilt(carry_bit_off_by_one(k)) != k for k in seams)
    assert any(rebuilt(short_mask(k)) != k for k in seams)
    assert any(max(threshold_off_by_one(k)) >= s.nb for k in seams)
    # and a seam set that lost its corner scalars no longer passes the corner check
    monkeypatch.setattr(wm, "corner_feasible", lambda *a, **k: False)
    with pytest.raises(AssertionError):
        test_seam_set_hits_every_named_corner(c, bits)


def test_lookup_budget_model():
    """need(c) = npts W 2^(c-1) 64: the figures the code comments quote, and the choice of the widest width that fits"""
    assert wm.lookup_need(2814, 16) == 2814 * 16 * 32768 * 64 and wm.lookup_need(2814, 17) == 2814 * 15 * 65536 * 64
    assert wm.lookup_need(6, 17) == 377487360 and wm.lookup_need(7, 13) == 36700160 and wm.lookup_need(6, 14) == 59768832
    for npts in (1, 3, 6, 100):
        for c in range(7, 18):
            assert wm.lookup_width(npts, wm.lookup_need(npts, c)) == c
            assert wm.lookup_width(npts, wm.lookup_need(npts, c) - 1) == (c - 1 if c > 7 else None)
    assert wm.lookup_width(6, 1 << 40) == 17
    g = bytes(range(64))
    assert wm.lookup_points(g * 10) == 2 and wm.lookup_points(b"".join(bytes([i]) * 64 for i in range(10))) == 10
    assert wm.lookup_points(b"".join(bytes([i]) * 64 for i in range(9)), bytes([0]) * 64) == 10      # 9 of 10 unique: merged (U + 1)
