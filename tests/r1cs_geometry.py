"""The geometry of the merge-path SpMV over the R1CS matrices (csrc/r1cs_kernels.cuh, csrc/abi_r1cs.inc), replayed in plain Python, and the
deterministic instances that put a row end, a carry or a run of carries on every seam of it.

    layout(nrows, row_lengths)       the merged list of (non-zeros, row ends) cut into chunks: start_row, and per chunk the rows it stores and its carry
    layouts(nc, nv, mats)            both compressed copies of a triplet set: row-major [A; B; C] (3 nc rows), column-major [A | B | C]^T (2 nv rows)
    fix_passes(carry_keys)           the fix-up passes: lane ranges, the runs a lane adds, the run it hands on; len() of it is the number of launches
    replay_multiply / replay_eval_table / replay_evaluate     the three results computed THROUGH chunks, carries and fix-up passes (ints mod r)
    classes(layout)                  the seam classes an instance hits (the tables at `classes`)
    offsets_by_lengths, matrix_seams, chunk_counts, run_alignments, cadence, saturated, tuned     the instances

The replay exists so that the class labels are labels of an algorithm that computes the right thing (tests/test_r1cs_geometry_cpu.py compares it with
r1cs_model.py on every instance); the device is compared with r1cs_model.py alone (tests/test_gpu_r1cs_seams.py).  The constants below mirror the
kernel's: a retune there fails test_r1cs_geometry_cpu.py first, and the instances must then be derived again."""
import random
from collections import namedtuple

import r1cs_model as rm

R = rm.R
R1CS_CHUNK = 16          # merge-path items per lane
R1CS_FIX_FIRST = 4       # carries per lane in the first fix-up pass
R1CS_FIX_CHUNK = 32      # carries per lane in the later passes
CARRY_CADENCE = 6        # products between two carry passes over the 17 columns
LENGTHS = (0, 1, 2, 5, 6, 7, 14, 15, 16, 17, 31, 32, 33)       # row lengths around the cadence, the chunk and two chunks
CADENCE_COUNTS = (5, 6, 7, 11, 12, 13, 15)
CHUNK_COUNTS = (1, 4, 5, 128, 129, 4096, 4097)                 # the nt == 1 edges of one, two, three and four fix-up passes
MIN_CONS = 2             # the smallest num_cons the SNARK ever pads to

# segs: the pieces of rows a lane walks, in item order: (row, first non-zero, non-zeros in this chunk, the row end lies in this chunk);
# stores: the rows whose end lies in the chunk; carry: (the row the chunk ends in — nrows behind the last row end —, it holds a non-zero of that row)
Chunk = namedtuple("Chunk", "segs stores carry")
Layout = namedtuple("Layout", "nrows nnz row_end nchunks start_row chunks rows_per_matrix")
Csr = namedtuple("Csr", "nrows lengths idx val")


def _ceil(a, b):
    return -(-a // b)


def layout(nrows, row_lengths, rows_per_matrix=None):
    """Row g's non-zeros are followed by its row end, item row_end[g] + g of the merged list.  start_row[t] counts the row ends among the first
    16 t items (counted here; the kernel searches); a chunk is then walked item by item as a lane walks it."""
    assert len(row_lengths) == nrows
    row_end, s = [], 0
    for n in row_lengths:
        s += n
        row_end.append(s)
    nnz, total = s, nrows + s
    nchunks = _ceil(total, R1CS_CHUNK)
    start_row, g = [], 0
    for t in range(nchunks + 1):
        d = min(t * R1CS_CHUNK, total)
        while g < nrows and row_end[g] + g + 1 <= d:
            g += 1
        start_row.append(g)
    chunks = []
    for t in range(nchunks):
        d0 = t * R1CS_CHUNK
        d1 = min(d0 + R1CS_CHUNK, total)
        i = start_row[t]
        j = first = d0 - i
        cnt, segs, stores = 0, [], []
        for _ in range(d0, d1):
            assert i < nrows, "the merged list has no item behind the last row end"
            if j < row_end[i]:
                cnt += 1; j += 1
            else:
                segs.append((i, first, cnt, True)); stores.append(i)
                i += 1; first = j; cnt = 0
        if cnt:
            segs.append((i, first, cnt, False))
        chunks.append(Chunk(segs, stores, (i, cnt > 0)))
    return Layout(nrows, nnz, row_end, nchunks, start_row, chunks, rows_per_matrix)


def csr_copies(num_cons, num_vars, mats):
    """the two stable counting sorts of sbn_r1cs_upload: -> (row-major Csr, column-major Csr); columns >= 2 num_vars are dropped"""
    nz = 2 * num_vars
    by_row = [[] for _ in range(3 * num_cons)]
    by_col = [[] for _ in range(nz)]
    for m, (rows, cols, vals) in enumerate(mats):
        for r, c, v in zip(rows, cols, vals):
            if c >= nz:
                continue
            g = m * num_cons + r
            by_row[g].append((c, v)); by_col[c].append((g, v))
    out = []
    for lists in (by_row, by_col):
        flat = [e for row in lists for e in row]
        out.append(Csr(len(lists), [len(row) for row in lists], [e[0] for e in flat], [e[1] for e in flat]))
    return tuple(out)


def layouts(num_cons, num_vars, mats):
    """-> (the layout of the row-major copy, the layout of the column-major copy)"""
    rowm, colm = csr_copies(num_cons, num_vars, mats)
    return layout(rowm.nrows, rowm.lengths, num_cons), layout(colm.nrows, colm.lengths)


def fix_passes(carry_keys):
    """The loop of r1cs_spmv_table over the carries of one merge-path pass (one key per chunk, sorted).  One dict per k_r1cs_fix launch:
    n, F, keys, lanes = [dict(range=(a, b), adds=[(key, first, end)], hands_on=(key, first, end) or None)]; a run is a range of the pass's own input.
    A lane hands its last run on, unless the pass has one lane, which adds it too."""
    passes, keys, F = [], list(carry_keys), R1CS_FIX_FIRST
    while True:
        n = len(keys)
        nt = _ceil(n, F)
        lanes = []
        for t in range(nt):
            a, b = t * F, min(t * F + F, n)
            runs, s = [], a
            for e in range(a + 1, b):
                if keys[e] != keys[s]:
                    runs.append((keys[s], s, e)); s = e
            runs.append((keys[s], s, b))
            lanes.append(dict(range=(a, b), adds=runs if nt == 1 else runs[:-1], hands_on=None if nt == 1 else runs[-1]))
        passes.append(dict(n=n, F=F, keys=keys, lanes=lanes))
        if nt == 1:
            return passes
        keys, F = [ln["hands_on"][0] for ln in lanes], R1CS_FIX_CHUNK


def _replay_spmv(csr, lay, x):
    """y = M x through the chunks: a lane stores the rows it finishes, the carries go through the fix-up passes.  Every row is stored exactly once
    before anything is added to it, and no pass touches a row twice."""
    out = [None] * csr.nrows
    vals = []
    for ch in lay.chunks:
        carry = 0
        for row, first, cnt, ended in ch.segs:
            s = sum(csr.val[j] * x[csr.idx[j]] for j in range(first, first + cnt)) % R
            if ended:
                assert out[row] is None, f"row {row} stored twice"
                out[row] = s
            else:
                carry = s
        vals.append(carry)
    assert None not in out
    assert lay.chunks[-1].carry == (csr.nrows, False), "the last chunk ends on the last row end: its carry has nothing to add"
    for p in fix_passes([ch.carry[0] for ch in lay.chunks]):
        touched, nxt = set(), []
        for ln in p["lanes"]:
            for key, a, b in ln["adds"]:
                if key < csr.nrows:
                    assert key not in touched, f"two adds to row {key} in one pass"
                    touched.add(key)
                    out[key] = (out[key] + sum(vals[a:b])) % R
            if ln["hands_on"]:
                _, a, b = ln["hands_on"]
                nxt.append(sum(vals[a:b]) % R)
        vals = nxt
    return out


def replay_multiply(num_cons, num_vars, mats, z):
    assert len(z) == 2 * num_vars
    rowm, _ = csr_copies(num_cons, num_vars, mats)
    y = _replay_spmv(rowm, layout(rowm.nrows, rowm.lengths, num_cons), z)
    return tuple(y[m * num_cons:(m + 1) * num_cons] for m in range(3))


def replay_eval_table(num_cons, num_vars, mats, rx, rA, rB, rC):
    ex = rm.eq_evals(rx)
    assert len(ex) == num_cons
    x = [r * e % R for r in (rA, rB, rC) for e in ex]               # k_r1cs_scale3
    _, colm = csr_copies(num_cons, num_vars, mats)
    return _replay_spmv(colm, layout(colm.nrows, colm.lengths), x)


def replay_evaluate(num_cons, num_vars, mats, rx, ry):
    """k_r1cs_spmv<true>: every piece of a row that holds a non-zero goes, times eq(rx)[row mod num_cons], to the sum of matrix row // num_cons"""
    ex, ey = rm.eq_evals(rx), rm.eq_evals(ry)
    rowm, _ = csr_copies(num_cons, num_vars, mats)
    acc = [0, 0, 0]
    for ch in layout(rowm.nrows, rowm.lengths, num_cons).chunks:
        for row, first, cnt, _ in ch.segs:
            if cnt:
                s = sum(rowm.val[j] * ey[rowm.idx[j]] for j in range(first, first + cnt)) % R
                acc[row // num_cons] = (acc[row // num_cons] + s * ex[row % num_cons]) % R
    return tuple(acc)


def _runs(keys, nrows):
    """maximal runs of equal keys below nrows: [(key, first, length)]"""
    out, s = [], 0
    for e in range(1, len(keys) + 1):
        if e == len(keys) or keys[e] != keys[s]:
            if keys[s] < nrows:
                out.append((keys[s], s, e - s))
            s = e
    return out


def classes(lay):
    """The seam classes a layout hits, as a set of tuples.

    rows          ("row", start item mod 16, length)                 every row; ("long_row", g): row g is longer than a chunk
    chunks        ("chunks", nchunks), ("passes", k_r1cs_fix launches), ("last_chunk_items", 1 .. 16), ("chunk_of_row_ends",): sixteen row ends
    cadence       ("cadence", n): a row that starts at a chunk's first item and ends in that chunk after n non-zeros
                  ("cadence_tail", n): a row that came in from the chunk before ends after n non-zeros of this chunk
                  ("cadence_carry", n): a chunk ends n non-zeros into the row it leaves as its carry
    carry runs    ("carry_run", first chunk mod 4, length): a maximal run of chunks that leave the same row as their carry (what the first pass sees)
                  ("run_boundary", "lane_edge" | "inside_lane"): two runs of at least two carries each, of rows g and g + 1, meet on / inside a first-pass lane range
                  ("fix_run_crosses", p): in pass p (from 1) a run lies across two lane ranges; ("fix_run_crosses_off_edge", p): and starts inside one
    matrices      (row-major copy only) ("shared_chunk", m): one chunk holds non-zeros of matrix m's last row and of matrix m + 1's row 0
                  ("last_row_nonempty", m), ("row0_empty",) | ("row0_nonempty",)
    degenerate    ("single_row",): all non-zeros in one row of this copy; ("single_nonzero",)"""
    cls = set()
    nrows = lay.nrows
    length = lambda g: lay.row_end[g] - (lay.row_end[g - 1] if g else 0)
    first_nz = lambda g: lay.row_end[g - 1] if g else 0
    for g in range(nrows):
        cls.add(("row", (first_nz(g) + g) % R1CS_CHUNK, length(g)))
        if length(g) > R1CS_CHUNK:
            cls.add(("long_row", g))
    keys = [ch.carry[0] for ch in lay.chunks]
    passes = fix_passes(keys)
    cls |= {("chunks", lay.nchunks), ("passes", len(passes)), ("last_chunk_items", nrows + lay.nnz - R1CS_CHUNK * (lay.nchunks - 1))}
    nc = lay.rows_per_matrix
    for ch in lay.chunks:
        if len(ch.stores) == R1CS_CHUNK:
            cls.add(("chunk_of_row_ends",))
        for k, (row, first, cnt, ended) in enumerate(ch.segs):
            if k == 0 and cnt and ended:
                cls.add(("cadence" if first == first_nz(row) else "cadence_tail", cnt))
            if not ended:
                cls.add(("cadence_carry", cnt))
            if nc and k and cnt and row % nc == 0 and row // nc in (1, 2) and ch.segs[k - 1][2]:
                cls.add(("shared_chunk", row // nc - 1))
    runs = _runs(keys, nrows)
    for key, s, n in runs:
        cls.add(("carry_run", s % R1CS_FIX_FIRST, n))
    for (k0, s0, n0), (k1, s1, n1) in zip(runs, runs[1:]):
        if k1 == k0 + 1 and s1 == s0 + n0 and n0 >= 2 and n1 >= 2:
            cls.add(("run_boundary", "lane_edge" if s1 % R1CS_FIX_FIRST == 0 else "inside_lane"))
    for p, ps in enumerate(passes, 1):
        for key, s, n in _runs(ps["keys"], nrows):
            if s // ps["F"] != (s + n - 1) // ps["F"]:
                cls.add(("fix_run_crosses", p))
                if s % ps["F"]:
                    cls.add(("fix_run_crosses_off_edge", p))
    if nc:
        for m in range(3):
            if length((m + 1) * nc - 1):
                cls.add(("last_row_nonempty", m))
        cls.add(("row0_nonempty",) if length(0) else ("row0_empty",))
    if lay.nnz == 1:
        cls.add(("single_nonzero",))
    elif lay.nnz and sum(1 for g in range(nrows) if length(g)) == 1:
        cls.add(("single_row",))
    return cls


# ---- the instances -----------------------------------------------------------------------------------------------------------------

def _vals(rng, n):
    """mostly uniform, with 0, 1 and r - 1 among them"""
    return [(0, 1, R - 1)[k] if k < 3 else rng.randrange(R) for k in (rng.randrange(8) for _ in range(n))]


def _zip_stubs(num_cons, num_vars, grows, cols, vals, rng=None):
    """triplets from one global row (m * num_cons + row) and one column per non-zero; with rng the entries of each matrix come in random order
    (the upload sorts them back, stably: what a row or a column holds, and how much, does not change).  Duplicated (row, col) entries add."""
    assert len(grows) == len(cols) == len(vals) and all(g < 3 * num_cons for g in grows) and all(c < 2 * num_vars for c in cols)
    mats = [([], [], []) for _ in range(3)]
    order = list(range(len(grows)))
    if rng:
        rng.shuffle(order)
    for e in order:
        m, r = divmod(grows[e], num_cons)
        mats[m][0].append(r); mats[m][1].append(cols[e]); mats[m][2].append(vals[e])
    return mats


def _from_row_lengths(num_cons, num_vars, lengths, rng, cols=None, shuffle=True):
    """row-major lengths (global rows, the rest empty) -> triplets; columns cyclic over 0 .. 2 num_vars - 1 unless given"""
    assert len(lengths) <= 3 * num_cons
    grows = [g for g, n in enumerate(lengths) for _ in range(n)]
    if cols is None:
        cols = [j % (2 * num_vars) for j in range(len(grows))]
    return _zip_stubs(num_cons, num_vars, grows, cols, _vals(rng, len(grows)), rng if shuffle else None)


def offset_length_sequence():
    """row lengths under which every (start item mod 16, length in LENGTHS) pair occurs exactly once: a row of length n moves the start on by
    n + 1, so the pairs are the edges offset -> offset + n + 1 (mod 16) of a graph in which every offset has 13 edges out and 13 in; the sequence
    is an Euler circuit of it from offset 0 (always the unused length listed last; Hierholzer's splice where that gets stuck).  16 x 13 = 208
    rows, 16 x sum(LENGTHS) = 2,864 non-zeros: no row is wasted."""
    unused = {o: list(LENGTHS) for o in range(R1CS_CHUNK)}
    stack, circuit = [(0, None)], []
    while stack:
        o = stack[-1][0]
        if unused[o]:
            n = unused[o].pop()
            stack.append(((o + n + 1) % R1CS_CHUNK, n))
        else:
            circuit.append(stack.pop()[1])
    return circuit[-2::-1]                                             # the edges in walking order, without the start's None


def offsets_by_lengths(axis):
    """every (start offset, length) pair on the rows of one copy; the other copy gets what falls out of zipping the stubs.
    rows: the sequence on global rows 0 .. 207 of [A; B; C], one non-zero in every later row (so that every row of C can be tuned to a witness);
          num_cons = 128, num_vars = 64.
    cols: the sequence on columns 0 .. 207; num_vars = 128 is the smallest power of two with 2 num_vars >= 208, num_cons = 2 the smallest shape:
          the six rows of [A; B; C] each run over about thirty chunks."""
    assert axis in ("rows", "cols")
    rng = random.Random(f"offsets {axis}")
    seq = offset_length_sequence()
    if axis == "rows":
        num_cons, num_vars = 128, 64
        lengths = seq + [1] * (3 * num_cons - len(seq))
        return num_cons, num_vars, _from_row_lengths(num_cons, num_vars, lengths, rng)
    num_cons, num_vars = MIN_CONS, 128
    cols = [c for c, n in enumerate(seq) for _ in range(n)]
    grows = [j % (3 * num_cons) for j in range(len(cols))]
    return num_cons, num_vars, _zip_stubs(num_cons, num_vars, grows, cols, _vals(rng, len(cols)), rng)


SEAM_VARIANTS = {"seams_full_last_chunk": (0, True), "seams_lone_row_end": (1, False)}    # name -> ((nrows + nnz) mod 16, row 0 of A is non-empty)


def _seam_lengths(num_cons, pads, row0):
    a = [3 if row0 else 0, pads[0]] + [1 + g % 3 for g in range(2, 20)] + [0] * 40 + [2, 2, 2, 3]
    b = [3, pads[1]] + [g % 3 for g in range(2, num_cons - 1)] + [3]
    c = [3, pads[2]] + [1] * (num_cons - 3) + [2]
    assert len(a) == len(b) == len(c) == num_cons
    return a + b + c


def matrix_seams():
    """-> {name: (num_cons, num_vars, mats)}.  The two variants of SEAM_VARIANTS: the last rows of A, B and C are non-empty, those of A and B share
    a chunk with non-zeros of the next matrix's row 0, rows 20 .. 59 of A are empty (one chunk of row ends only), the columns num_vars (the constant)
    and 2 num_vars - 1 are longer than a chunk, every row of C holds a non-zero; the three lengths in rows 1 (at most 15) are searched, in order,
    for the first choice that puts the seams where they are wanted.  And three degenerate sets: one row, one column, one non-zero."""
    num_cons, num_vars = 64, 16
    out = {}
    for name, (mod, row0) in SEAM_VARIANTS.items():
        want = {("shared_chunk", 0), ("shared_chunk", 1), ("chunk_of_row_ends",), ("last_chunk_items", mod or R1CS_CHUNK)}
        pads = next(p for p in ((x, y, w) for x in range(16) for y in range(16) for w in range(16))
                    if want <= classes(layout(3 * num_cons, _seam_lengths(num_cons, p, row0), num_cons)))
        lengths = _seam_lengths(num_cons, pads, row0)
        rng = random.Random(name)
        nnz = sum(lengths)
        cols = [num_vars] * 20 + [2 * num_vars - 1] * 20 + [j % (2 * num_vars) for j in range(nnz - 40)]
        rng.shuffle(cols)
        out[name] = (num_cons, num_vars, _from_row_lengths(num_cons, num_vars, lengths, rng, cols))
    nc, nv = 16, 8
    rng = random.Random("degenerate")
    out["one_row"] = (nc, nv, _zip_stubs(nc, nv, [nc + 5] * 50, [j % (2 * nv) for j in range(50)], _vals(rng, 50)))
    out["one_col"] = (nc, nv, _zip_stubs(nc, nv, [j % (3 * nc) for j in range(50)], [3] * 50, _vals(rng, 50)))
    out["one_nonzero"] = (nc, nv, _zip_stubs(nc, nv, [3 * nc - 1], [2 * nv - 1], [rng.randrange(1, R)]))
    return out


def chunk_counts(n0):
    """an instance whose row-major copy has exactly n0 chunks, at num_cons = 2: 16 n0 - 5 items, six rows, row 0 of B over n0 // 2 chunks and more,
    row 0 of C over most of the rest, so that both halves of every pass's carries are runs across lane ranges"""
    num_cons, num_vars = MIN_CONS, 8
    nnz = R1CS_CHUNK * n0 - 5 - 3 * num_cons
    if n0 == 1:
        lengths = [1, 0, 2, 1, 0, 1]
    else:
        big = R1CS_CHUNK * (n0 // 2) + 8
        lengths = [3, 0, big, 2, nnz - 6 - big, 1]
    assert sum(lengths) == nnz and min(lengths) >= 0
    return num_cons, num_vars, _from_row_lengths(num_cons, num_vars, lengths, random.Random(f"chunks {n0}"))


RUN_SPANS = range(1, 10)
BIG_RUN = R1CS_FIX_FIRST * R1CS_FIX_CHUNK * 2 + 5       # chunks: two lanes of the second pass and a bit


class _Rows:
    """row lengths written front to back, with the position in the merged list"""

    def __init__(self):
        self.lengths, self.pos = [], 0

    def row(self, n):
        self.lengths.append(n); self.pos += n + 1

    def advance(self, chunk_mod, offset, mod=R1CS_FIX_FIRST):
        """filler rows until the next row starts `offset` items into a chunk whose index is chunk_mod (mod `mod`): empty rows, then rows of one chunk"""
        while self.pos % R1CS_CHUNK != offset:
            self.row(0)
        while self.pos // R1CS_CHUNK % mod != chunk_mod:
            self.row(R1CS_CHUNK - 1)


def run_alignments():
    """Rows that leave runs of 1 .. 9 equal carries starting at a chunk = 0, 1, 2, 3 (mod 4) — every way a run can lie across the first pass's lanes
    of four —; one row over BIG_RUN chunks behind a short row, whose run in the second pass starts inside a lane range and crosses two of them; two long
    rows back to back, meeting once on a first-pass lane edge and once inside a lane's range.  Every designed row starts three items into its chunk,
    so that its run starts with that chunk."""
    rw = _Rows()
    for a in range(R1CS_FIX_FIRST):
        for span in RUN_SPANS:
            rw.advance(a, 3)
            rw.row(R1CS_CHUNK * span)                                   # the row end lies `span` chunks on: `span` carries
    rw.advance(5 * R1CS_FIX_FIRST + 1, 0, R1CS_FIX_FIRST * R1CS_FIX_CHUNK)
    rw.row(2)                                                           # the short row; the big row starts 3 items into a chunk = 21 (mod 128)
    rw.row(R1CS_CHUNK * BIG_RUN)
    for first_chunk, span in ((1, 3), (1, 2)):                          # the second row's run starts at chunk 1 + span: = 0 (mod 4), then = 3
        rw.advance(first_chunk, 3)
        rw.row(R1CS_CHUNK * span); rw.row(R1CS_CHUNK * 3)
    num_vars = 32
    num_cons = MIN_CONS
    while 3 * num_cons < len(rw.lengths):
        num_cons *= 2
    return num_cons, num_vars, _from_row_lengths(num_cons, num_vars, rw.lengths, random.Random("runs"))


def cadence():
    """rows whose non-zeros inside ONE chunk number 5, 6, 7, 11, 12, 13 and 15 (around the carry pass every CARRY_CADENCE products, which must not
    stand in for `the row holds a non-zero`): as a whole row from a chunk's first item, as the tail of a row that fills the chunk before, and as the
    piece a chunk leaves as its carry"""
    rw = _Rows()
    for n in CADENCE_COUNTS:
        rw.advance(0, 0, 1); rw.row(n)
    for n in CADENCE_COUNTS:
        rw.advance(0, 0, 1); rw.row(R1CS_CHUNK + n)
    for n in CADENCE_COUNTS:
        rw.advance(0, R1CS_CHUNK - n, 1); rw.row(n + 3)
    num_cons, num_vars = 64, 8
    return num_cons, num_vars, _from_row_lengths(num_cons, num_vars, rw.lengths, random.Random("cadence"))


SAT_ROW = R1CS_FIX_FIRST * R1CS_FIX_CHUNK * R1CS_CHUNK * 2      # non-zeros: 256 chunks, 64 first-pass lanes, 2 second-pass lanes


def saturated():
    """-> {name: (num_cons, num_vars, mats, z)}: the largest canonical value wherever a lazy sum could run out of headroom.
    offsets_rm1       offsets_by_lengths("rows") with every value, and every entry of z, r - 1
    carry_rm1         one row of SAT_ROW non-zeros, row 0 of A: r - 1 at every non-zero j = 0 (mod 16), 0 elsewhere, z = 1: every chunk's carry is r - 1,
                      a first-pass lane sums 4 of them, a second-pass lane 32 such sums, the last pass 2 of those onto the stored row
    carry_rm1_stored  the same with one more non-zero (j = SAT_ROW: r - 1), so that the value the row's own lane stores is r - 1 as well"""
    nc, nv, mats = offsets_by_lengths("rows")
    out = {"offsets_rm1": (nc, nv, [(r, c, [R - 1] * len(v)) for r, c, v in mats], [R - 1] * (2 * nv))}
    num_cons, num_vars = MIN_CONS, 8
    for name, n in (("carry_rm1", SAT_ROW), ("carry_rm1_stored", SAT_ROW + 1)):
        vals = [R - 1 if j % R1CS_CHUNK == 0 else 0 for j in range(n)]
        mats = _zip_stubs(num_cons, num_vars, [0] * n, [j % (2 * num_vars) for j in range(n)], vals)
        out[name] = (num_cons, num_vars, mats, [1] * (2 * num_vars))
    return out


def tuned(num_cons, num_vars, mats, z, violate=()):
    """the same triplets with single values changed so that z satisfies every row but those of `violate`: where row i of C holds a non-zero on a
    column with z != 0, that value makes Cz[i] = Az[i] Bz[i] (+ 1 in a violated row); where it holds none, one value of B makes Bz[i] = 0.
    Values only: the geometry stays."""
    mats = [(list(r), list(c), list(v)) for r, c, v in mats]
    Az, Bz, Cz = rm.multiply_vec(num_cons, num_vars, mats, z)
    handle = {}
    for m in (1, 2):
        for e, (r, c) in enumerate(zip(mats[m][0], mats[m][1])):
            if c < 2 * num_vars and z[c] % R:
                handle.setdefault((m, r), e)
    for i in range(num_cons):
        if (2, i) in handle:
            e = handle[2, i]
            target = (Az[i] * Bz[i] + (i in violate)) % R
            mats[2][2][e] = (mats[2][2][e] + (target - Cz[i]) * pow(z[mats[2][1][e]], -1, R)) % R
        elif i in violate:
            assert Cz[i] == 0 and Az[i] * Bz[i] % R, f"row {i} cannot be violated"
        elif (Az[i] * Bz[i] - Cz[i]) % R:
            e = handle[1, i]
            mats[1][2][e] = (mats[1][2][e] - Bz[i] * pow(z[mats[1][1][e]], -1, R)) % R
    return mats


_INSTANCES = {}


def instances():
    """every instance once, by name: {name: (num_cons, num_vars, mats, z or None)}; z is given where the instance fixes it (saturated).  Shared by the CPU
    and the GPU tests; nobody changes what it returns."""
    if not _INSTANCES:
        for axis in ("rows", "cols"):
            _INSTANCES[f"offsets_{axis}"] = offsets_by_lengths(axis) + (None,)
        for name, inst in matrix_seams().items():
            _INSTANCES[name] = inst + (None,)
        for n0 in CHUNK_COUNTS:
            _INSTANCES[f"chunks_{n0}"] = chunk_counts(n0) + (None,)
        _INSTANCES["run_alignments"] = run_alignments() + (None,)
        _INSTANCES["cadence"] = cadence() + (None,)
        _INSTANCES.update(saturated())
    return _INSTANCES
