"""Plain-integer model of the geometry of a bucket job (msm_host.hpp: run_bucket_job) and of how the accumulate kernels cut a bucket
(msm_kernels.cuh: k_acc_first<G>, k_acc_extra, k_acc_merge), with builders for scalars that put chosen loads into chosen buckets.

A bucket's sorted entry list of cnt entries is cut into segments of SEG entries.  Segment 0 is taken by the bucket's G = LPB owner
lanes (k_acc_first<G>: G contiguous parts of ceil(min(cnt, SEG) / G) entries, the later ones possibly short or empty), the k =
ceil(cnt / SEG) - 1 other segments go to the work list of k_acc_extra, and k_acc_merge folds their partial sums into the bucket's
slot 0: one lane per bucket while k <= MERGE_LANE_MAX, one wave per bucket (lane l takes partials l, l + 64, ...) beyond.
"""
import collections

import numpy as np

import window_model as wm

ACC_SEG_MAX = 8192               # msm_kernels.cuh
MERGE_LANE_MAX = 12              # msm_kernels.cuh
ACC_EXTRA_GRID = 2048 * 256      # work items one pass of k_acc_extra's grid covers
MERGE_LANE_GRID = 4096 * 64      # big-list entries one pass of k_acc_merge's lane loop covers
MERGE_WAVE_GRID = 4096           # ... and of its wave loop
SINGLE, ROWS = "single", "rows"


def geometry(mode, n, P, estride, c, env=None):
    """(SEG, LPB, L, chunks, levels, quad) of run_bucket_job.
    mode: SINGLE (one MSM: P = W windows) or ROWS (P rows over one shared bucket set each).  n: the records of a problem as the digit
    kernel counts them (J.da.n: the terms of a plain MSM, TWICE the terms under GLV, the columns of a row, blind included).
    estride: sorted entries per problem (n for an MSM, columns x W for rows).  env: SBN_MSM_SEG / SBN_RED_L as strings, when set."""
    env = env or {}
    nb = 1 << (c - 1)
    NB = P * nb
    mean = estride // nb + 1
    SEG = 32
    while SEG < 2 * mean and SEG < ACC_SEG_MAX:
        SEG <<= 1
    if NB < 262144:
        cap = 32
        while cap * 262144 < P * estride and cap < ACC_SEG_MAX:
            cap <<= 1
        SEG = min(SEG, cap)
    if mode == SINGLE and 512 <= n <= 4096:
        SEG = 8
    if "SBN_MSM_SEG" in env and 8 <= int(env["SBN_MSM_SEG"]) <= ACC_SEG_MAX:
        SEG = int(env["SBN_MSM_SEG"])
    LPB = 2 if mode == SINGLE and mean >= 48 and NB <= 1 << 19 else 1
    L = 1
    while L * 64 * 2048 < NB and L < 16:
        L <<= 1
    L = max(L, 4)
    L = min(L, nb // 64)
    L = max(L, 1)
    if NB <= 64 * 16 * 1024:
        best, bl = None, L
        t = 1
        while t <= 32 and t * 64 <= max(nb, 64):
            waves = P * ((nb + 64 * t - 1) // (64 * t))
            cost = ((waves + 1023) // 1024) * ((2 * t - 1) + t * (LPB - 1) + 10)
            if best is None or cost < best:
                best, bl = cost, t
            t += 1
        L = bl
    if "SBN_RED_L" in env and 1 <= int(env["SBN_RED_L"]) <= 64:
        L = int(env["SBN_RED_L"])
    chunks = (nb + 64 * L - 1) // (64 * L)
    levels, G = 0, chunks
    while True:
        levels += 1
        G = (G + 63) // 64
        if G == 1:
            break
    return SEG, LPB, L, chunks, levels, 1 if P * chunks <= 2048 else 0


GEOMETRY_KEYS = ("SEG", "LPB", "L", "chunks", "levels", "quad")


def geometry_of(acc):
    """the six host values of Context.prof_last_acc(), in the order geometry() returns them"""
    return tuple(acc[k] for k in GEOMETRY_KEYS)


def cut(cnt, SEG, G):
    """-> (the G (from, to) parts of segment 0, k, the k (from, to) extra segments, 'none' / 'lane' / 'wave')"""
    first = min(cnt, SEG)
    per = (first + G - 1) // G
    parts = []
    for g in range(G):
        fr = min(g * per, first)
        parts.append((fr, min(g * per + per, first)))
    k = (cnt + SEG - 1) // SEG - 1 if cnt > SEG else 0
    extras = [(j * SEG, min(j * SEG + SEG, cnt)) for j in range(1, k + 1)]
    return parts, k, extras, "none" if k == 0 else "lane" if k <= MERGE_LANE_MAX else "wave"


def _counts(loads):
    if isinstance(loads, dict):
        loads = list(loads.values())
    return np.asarray(loads, dtype=np.int64).ravel()


def expected_counters(loads, SEG):
    """(extra_count, big_count) the accumulate kernel leaves for these per-bucket loads ({bucket: count}, or any array of counts)"""
    cn = _counts(loads)
    big = cn > SEG
    return int(((cn[big] + SEG - 1) // SEG - 1).sum()), int(big.sum())


def merge_paths(loads, SEG):
    """(buckets merged by one lane, buckets merged by one wave)"""
    cn = _counts(loads)
    k = np.where(cn > SEG, (cn + SEG - 1) // SEG - 1, 0)
    return int(((k > 0) & (k <= MERGE_LANE_MAX)).sum()), int((k > MERGE_LANE_MAX).sum())


def loads_of(scalars, c, W):
    """{(window, bucket): entries} of a single MSM over these scalars (integers): digit d != 0 of window w is one entry of bucket |d| - 1"""
    out = collections.Counter()
    for k, times in collections.Counter(scalars).items():
        digits, carry = wm.recode_sequential(k, c, W)
        assert carry == 0, hex(k)
        for w, d in enumerate(digits):
            if d:
                out[(w, abs(d) - 1)] += times
    return dict(out)


def loads_of_rows(rows, c, W):
    """{(row, bucket): entries} of a row commit (one bucket set per row, shared by its W windows); rows: lists of integers, blind included"""
    out = collections.Counter()
    for r, row in enumerate(rows):
        for (w, b), t in loads_of(row, c, W).items():
            out[(r, b)] += t
    return dict(out)


def loads_of_bytes(blob, c, W, width=32):
    """loads_of for many scalars at once: little-endian records of `width` bytes -> int64 array [W, 2^(c-1)] (numpy twin of loads_of;
    tests/test_acc_model_cpu.py holds the two against each other)"""
    a = np.frombuffer(blob, dtype="<u8").reshape(-1, width // 8)
    n, words = a.shape
    half, full = 1 << (c - 1), 1 << c
    out = np.zeros((W, half), dtype=np.int64)
    carry = np.zeros(n, dtype=np.int64)
    for w in range(W):
        o = c * w
        i, sh = o // 64, o % 64
        if i >= words:
            raw = np.zeros(n, dtype=np.uint64)
        else:
            raw = a[:, i] >> np.uint64(sh)
            if sh + c > 64 and i + 1 < words:
                raw = raw | (a[:, i + 1] << np.uint64(64 - sh))
        d = (raw & np.uint64(full - 1)).astype(np.int64) + carry
        neg = d >= half
        carry = neg.astype(np.int64)
        mag = np.where(neg, full - d, d)
        out[w] = np.bincount(mag[mag > 0] - 1, minlength=half)
    assert not carry.any()
    return out


# ---- scalars that put chosen loads into chosen buckets ----------------------------------------------------------------------
def load_set(SEG):
    """the per-bucket loads every case drives: below, on and past one and two segments; k = 12 (the last merge by one lane, the last
    segment full), k = 13 (the first merge by a wave, the last segment one entry) and k = 65 (lane 0 of the wave takes two partials).
    With segments of ACC_SEG_MAX the three long ones are left out (65 segments would be half a million entries in one bucket)."""
    s = [0, 1, 2, 3, SEG - 1, SEG, SEG + 1, 2 * SEG - 1, 2 * SEG, 2 * SEG + 1]
    if SEG < ACC_SEG_MAX:
        s += [13 * SEG, 13 * SEG + 1, 65 * SEG + 1]
    return s


def usable_buckets(c, W, w, bits=254):
    """(buckets 0 .. m - 1 of window w a scalar d 2^(c w) below the bound can reach, whether the window's last bucket 2^(c-1) - 1 is
    reachable through the digit -2^(c-1)).  A top window narrower than c - 1 bits has few."""
    half, bound = 1 << (c - 1), wm.bound_of(bits)
    m = min(half - 1, (bound - 1) >> (c * w))
    return m, w < W - 1 and (half << (c * w)) < bound


def window_loads(c, W, w, SEG, bits=254):
    """the load set of window w: all of it, or, where the window has too few reachable buckets (a narrow top window), its longest loads
    first: the merge seams, then the segment seams"""
    m, last = usable_buckets(c, W, w, bits)
    full = load_set(SEG)
    prio = [65 * SEG + 1, 13 * SEG + 1, 13 * SEG, SEG + 1, 2 * SEG, SEG, 2 * SEG + 1, 2 * SEG - 1, SEG - 1, 3, 2, 1, 0]
    return full if m + last >= len(full) else [t for t in prio if t in full][:m + last]


def edge_plan(c, W, SEG, windows, background=None, bits=254):
    """-> (scalars, {window: {load: bucket}}).  `windows`: a list of windows, each given window_loads(), or {window: loads}.
    `background`: {(window, bucket): entries} the other scalars of the job already put there (loads_of of them); a bucket is topped up to
    its load, so a load needs a bucket whose background does not exceed it.
    Scalars are d 2^(c w) (digit +d in window w, zero elsewhere) and 2^(c-1) 2^(c w) (digit -2^(c-1): the LAST bucket of window w, and +1
    in window w + 1, bucket 0 there).  Per window the longest load goes to bucket 0, the second longest to the last bucket (where it can
    be reached), the others to buckets 1, 2, ... in decreasing order."""
    half = 1 << (c - 1)
    bg = collections.Counter(background or {})
    want = {w: window_loads(c, W, w, SEG, bits) for w in windows} if not isinstance(windows, dict) else {w: list(v) for w, v in windows.items()}
    out, plan, rest = [], {w: {} for w in want}, {}
    for w in sorted(want):                                 # the last buckets first: each of their scalars also lands in bucket 0 of w + 1
        loads = sorted(want[w], reverse=True)
        assert len(set(loads)) == len(loads)
        if usable_buckets(c, W, w, bits)[1] and len(loads) >= 2:
            t = loads.pop(1)
            have = bg[(w, half - 1)]
            assert have <= t, (w, t, have)
            out += [half << (c * w)] * (t - have)
            bg[(w, half - 1)] = t; bg[(w + 1, 0)] += t - have
            plan[w][t] = half - 1
        rest[w] = loads
    for w in sorted(want):
        m = usable_buckets(c, W, w, bits)[0]
        b = 0
        for i, t in enumerate(rest[w]):
            while b < m and bg[(w, b)] > t:
                b += 1
            assert b < m and (i > 0 or b == 0), "window %d has no bucket left for a load of %d" % (w, t)
            out += [(b + 1) << (c * w)] * (t - bg[(w, b)])
            bg[(w, b)] = t
            plan[w][t] = b
            b += 1
    return out, plan


def edge_scalars(c, W, SEG, windows, background=None, bits=254):
    return edge_plan(c, W, SEG, windows, background, bits)[0]


def glv_scalars(edge_halves, c, W, lam, r):
    """full scalars whose GLV halves are the given edge halves (all of one window each).  The kernel's decomposition returns the pair
    (k1, k2) of k = k1 + lambda k2 that lies in its fundamental cell: (k1, 0) for a k1 below 2^126, but never (0, k2); a second half k2
    needs a first half of at least k2 2^-63 beside it.  So the halves of the middle window travel as second halves beside those of the top
    window (or the other way round, the shorter list second), every other half alone as a first half.  The caller checks the result
    with the model of the decomposition (tests/test_glv_cpu.py: split)."""
    by_w = collections.defaultdict(list)
    for h in edge_halves:
        by_w[(h.bit_length() - 1) // c].append(h)
    mid, top = by_w.pop(W // 2, []), by_w.pop(W - 1, [])
    first, second = (top, mid) if len(top) >= len(mid) else (mid, top)
    out = [(k1 + lam * k2) % r for k1, k2 in zip(first, second)] + first[len(second):]
    for lst in by_w.values():
        out += lst
    return out


def masked_uniform(n, seed, c, windows, bits=254):
    """n uniform scalars below the bound whose digits in the given windows are zero (the window and the two bits below it cleared, so
    that no carry reaches it): a filler that leaves those windows to the edge scalars.  What it does load is found with loads_of."""
    import random
    rnd, bound = random.Random(seed), wm.bound_of(bits)
    mask = 0
    for w in windows:
        lo = max(c * w - 2, 0)
        mask |= ((1 << (c * w + c - lo)) - 1) << lo
    return [rnd.randrange(bound) & ~mask for _ in range(n)]


def row_edge_columns(c, W, SEG, loads, background=None):
    """columns of ONE row of a row commit that top the row's buckets up to `loads`: a column sum_w d 2^(c w) over m windows is m entries of
    bucket d - 1, whichever windows they are.  The longest load goes to bucket 0, the second longest to the last bucket (columns
    2^(c-1) 2^(c w): one entry there and one, the carry, in bucket 0), the others to buckets 1, 2, ...  -> (columns, {load: bucket})"""
    half = 1 << (c - 1)
    bg = collections.Counter(background or {})
    loads = sorted(loads, reverse=True)
    lowW = W - 1                                            # windows every digit below 2^(c-1) fits (the top one may be narrow)
    assert usable_buckets(c, W, 0)[0] == half - 1
    out, plan = [], {}

    def fill(d, t):                                         # t entries of digit d
        while t > 0:
            m = min(t, lowW)
            out.append(sum(d << (c * w) for w in range(m))); t -= m

    t = loads.pop(1)
    have = bg[half - 1]
    assert have <= t
    for j in range(t - have):
        out.append(half << (c * (j % (lowW - 1))))
    bg[0] += t - have; plan[t] = half - 1
    b = 0
    for i, t in enumerate(loads):
        while b < half - 1 and bg[b] > t:
            b += 1
        assert b < half - 1 and (i > 0 or b == 0)
        fill(b + 1, t - bg[b]); bg[b] = t; plan[t] = b
        b += 1
    return out, plan


def digit_range_columns(n, seed, c, W, lo, hi):
    """n columns whose digits are uniform in [lo, hi] (positive, below 2^(c-1): no carries) in every window but the top one"""
    import random
    rnd = random.Random(seed)
    assert 1 <= lo <= hi < 1 << (c - 1)
    return [sum(rnd.randint(lo, hi) << (c * w) for w in range(W - 1)) for _ in range(n)]


# ---- the window width the host takes (msm_host.hpp: choose_shape, glv_shape), to name the shipped jobs ------------------------
MSM_C_MAX, S2_C_MAX = 16, 22


def choose_c(terms, shared, cmax, problems=0, chard=MSM_C_MAX):
    """window bits of choose_shape without SBN_MSM_C.  A single MSM: shared False, problems 1, cmax = chard = S2_C_MAX when it takes the
    two-level sort, else MSM_C_MAX.  A row commit: shared True, cmax 16, problems = rows, terms = columns."""
    cmax = min(cmax, chard)
    if problems and problems * terms <= 32768:
        if not shared and problems == 1 and 512 <= terms <= 4096 and cmax >= 8:
            return 8 if terms <= 512 else 7
        bl, bcl = None, 7
        for c in range(7, cmax + 1):
            s = wm.make_shape(c)
            tb = 254 - (s.W - 1) * c
            top = terms / float(1 << (min(tb, 20) if tb > 0 else 0))
            load = (terms * s.W / s.nb if shared else terms / s.nb) + top
            if load <= 6.0:
                return c
            if bl is None or load < bl:
                bl, bcl = load, c
        return bcl
    if not shared and terms < 1 << 20 and cmax >= 15:
        return 15
    best, bc = None, 7
    for c in range(7, cmax + 1):
        s = wm.make_shape(c)
        per_bucket = 40.0 if chard > MSM_C_MAX or (shared and problems >= 256) else 56.0
        cost = terms * s.W * 10.0 + (1.0 if shared else s.W) * s.nb * per_bucket
        if not shared and 254 - (s.W - 1) * c < c - 1:
            cost += terms * 5.0
        if best is None or cost < best:
            best, bc = cost, c
    return bc


def glv_c(n):
    """window bits of glv_shape for n bases (2n half-scalars of 127 bits) without SBN_MSM_C"""
    def cost(c):
        s = wm.make_shape(c, 127)
        return 2 * n * s.W * 10.0 + s.W * s.nb * 40.0 + (2 * n * 5.0 if 127 - (s.W - 1) * c < c - 1 else 0.0)
    best = 16
    for c in range(13, 18):
        if cost(c) < cost(best):
            best = c
    return best


def shipped_jobs():
    """[(name, mode, n, P, estride, c)] of the jobs the benchmark runs: single MSMs of 2^20 terms over a resident handle (GLV) and
    staged (plain), of 2^22 and 2^26 terms, and the bucket-method commit of the derefs matrix (4096 rows x 2815 merged columns)"""
    out = []
    c = glv_c(1 << 20); s = wm.make_shape(c, 127)
    out.append(("2^20 GLV", SINGLE, 2 << 20, s.W, 2 << 20, c))
    for log_n in (20, 22, 26):
        c = choose_c(1 << log_n, False, S2_C_MAX, 1, S2_C_MAX); s = wm.make_shape(c)
        out.append(("2^%d plain" % log_n, SINGLE, 1 << log_n, s.W, 1 << log_n, c))
    c = choose_c(2815, True, 16, 4096); s = wm.make_shape(c)
    out.append(("Hyrax 4096 x 2815", ROWS, 2815, 4096, 2815 * s.W, c))
    return out
