"""GPU: the merge-path SpMV of csrc/r1cs_kernels.cuh (k_r1cs_partition, k_r1cs_spmv<false|true>, k_r1cs_fix) at its chunk, carry and fix-up seams,
bit for bit against r1cs_model.py, on the deterministic instances of tests/r1cs_geometry.py (tests/test_r1cs_geometry_cpu.py shows that each of
them hits the seam it is named for): every (row start mod 16, row length) pair on either copy; the last rows of A and B in one chunk with the next
matrix's row 0, a last chunk of sixteen items and of the lone last row end, a chunk of row ends only; 1, 4, 5, 128, 129, 4096 and 4097 chunks with the
number of k_r1cs_fix launches each; runs of equal-row carries at every position against the fix-up lanes; rows of 5 .. 15 non-zeros inside one chunk
around the carry pass every 6 products; r - 1 in every carry of a row over two second-pass lanes.  test_gpu_r1cs.py draws its matrices at random and
keeps the top quarter of every matrix empty; this file is where those seams are pinned.

Not reached here, by design: a fifth fix-up pass and the grid-stride loop of k_r1cs_spmv<true> (test_r1cs_keyless_shape runs them), and the fe_reduce
inside fr_acc — it fires after 64 additions to one accumulator, a lane adds at most 16 for every chunk it walks (one per finished row or carry), and
every lane of these instances walks one chunk, so it cannot fire below about 4 x 262,144 chunks."""
import random

import pytest

import r1cs_geometry as g
import r1cs_model as rm
import snark_model as sm
from test_gpu_r1cs import _download, _log2, _rand, _upload

pytestmark = pytest.mark.gpu
R = rm.R
NAMES = sorted(g.instances())
SEAMS = sorted(g.SEAM_VARIANTS)
LAZY = ["cadence", "carry_rm1", "carry_rm1_stored", "offsets_rm1"]
TRIPLES = [(1, 1, 1), None, (0, 1, R - 1)]                         # None: a uniform triple
_DEV, _REF = {}, {}


def handle(ctx, name, mont=False):
    """the uploaded instance, once for the module"""
    if (name, mont) not in _DEV:
        nc, nv, mats = g.instances()[name][:3]
        _DEV[name, mont] = _upload(ctx, nc, nv, mats, mont=mont)
    return _DEV[name, mont]


@pytest.fixture(scope="module", autouse=True)
def _free_handles():
    yield
    for h in _DEV.values():
        h.free()
    _DEV.clear(); _REF.clear()


def _seed(name):
    return sum(name.encode()) * 131


def _bits(i, ell):
    """the 0 / 1 point at which eq picks entry i"""
    return [i >> (ell - 1 - k) & 1 for k in range(ell)]


def ref(name):
    """inputs and the model's results, once for the module: z; multiply; [(rx, r_A, r_B, r_C, table)]; [(rx, ry, A B C(rx, ry))]"""
    if name not in _REF:
        nc, nv, mats, z = g.instances()[name]
        lx, ly, s = _log2(nc), _log2(2 * nv), _seed(name)
        z = z or _rand(2 * nv, s)
        tables = []
        for i, tr in enumerate(TRIPLES):
            rx, (rA, rB, rC) = _rand(lx, s + 1 + i), tr or tuple(_rand(3, s + 7))
            tables.append((rx, rA, rB, rC, rm.eval_table(nc, nv, mats, rx, rA, rB, rC)))
        points = [(_rand(lx, s + 10), _rand(ly, s + 11)), ([1] * lx, [1] * ly), ([0] * lx, [0] * ly)]
        if name in g.SEAM_VARIANTS:
            # rx picks row num_cons - 1, then row 0; ry uniform (the whole row against eq(ry)), then 0 / 1 on a column the row holds in A, in B
            # and in C: single cells, where a sum fed to the wrong matrix's accumulator shows as a value in the wrong slot
            for row in (nc - 1, 0):
                points.append((_bits(row, lx), _rand(ly, s + 12 + row)))
                for rows, cols, vals in mats:
                    held = [c for r, c, v in zip(rows, cols, vals) if r == row and v]
                    if held:
                        points.append((_bits(row, lx), _bits(held[0], ly)))
        evals = [(rx, ry, rm.evaluate(nc, nv, mats, rx, ry)) for rx, ry in points]
        _REF[name] = dict(z=z, mult=rm.multiply_vec(nc, nv, mats, z), tables=tables, evals=evals)
    return _REF[name]


def _multiply(ctx, h, tz):
    return tuple(_download(ctx, t) for t in ctx.r1cs_multiply(h, tz))


def _check_multiply(ctx, h, name):
    tz = ctx.table_upload(rm.to_bytes(ref(name)["z"]))
    try:
        assert _multiply(ctx, h, tz) == ref(name)["mult"]
    finally:
        tz.free()


def _check_eval_table(ctx, h, name):
    nv = g.instances()[name][1]
    for i, (rx, rA, rB, rC, want) in enumerate(ref(name)["tables"]):
        t = ctx.r1cs_eval_table(h, rm.to_bytes(rx), *(rm.to_bytes([v]) for v in (rA, rB, rC)))
        assert len(t) == 2 * nv
        assert _download(ctx, t) == want, f"triple {i}"


def _check_evaluate(ctx, h, name):
    for i, (rx, ry, want) in enumerate(ref(name)["evals"]):
        got = tuple(rm.from_bytes(b"".join(ctx.r1cs_evaluate(h, rm.to_bytes(rx), rm.to_bytes(ry)))))
        assert got == want, f"point {i}: rx={rx if set(rx) <= {0, 1} else 'uniform'} ry={ry if set(ry) <= {0, 1} else 'uniform'}"


@pytest.mark.parametrize("name", NAMES)
def test_multiply(ctx, name):
    """Az, Bz, Cz in full: the rows a lane stores, the carries, every fix-up pass (row-major copy)"""
    _check_multiply(ctx, handle(ctx, name), name)


@pytest.mark.parametrize("name", NAMES)
def test_eval_table(ctx, name):
    """the phase-2 table in full at (1, 1, 1), a uniform triple and (0, 1, r - 1): the same kernels over the column-major copy"""
    _check_eval_table(ctx, handle(ctx, name), name)


@pytest.mark.parametrize("name", NAMES)
def test_evaluate(ctx, name):
    """A, B, C(rx, ry) at a uniform point, the all-ones and the all-zeros point; for the matrix seams also at the points that pick row num_cons - 1
    and row 0, against a uniform ry and against single columns"""
    if name in g.SEAM_VARIANTS:
        nc = g.instances()[name][0]
        picked = [e for e in ref(name)["evals"][3:] if set(e[1]) <= {0, 1}]
        assert len(picked) >= 5 and all(sum(1 for v in e[2] if v) >= 1 for e in picked), "the single cells are cells the matrices hold"
        assert {tuple(e[0]) for e in picked} == {tuple(_bits(nc - 1, _log2(nc))), tuple(_bits(0, _log2(nc)))}
    _check_evaluate(ctx, handle(ctx, name), name)


@pytest.mark.parametrize("n0", g.CHUNK_COUNTS)
def test_fix_launches(ctx, n0):
    """one sbn_r1cs_multiply over n0 chunks launches k_r1cs_fix as often as fix_passes says (1, 1, 2, 2, 3, 3, 4): the pass an instance is named
    for is a pass that ran"""
    name = f"chunks_{n0}"
    nc, nv, mats = g.instances()[name][:3]
    lay = g.layouts(nc, nv, mats)[0]
    assert lay.nchunks == n0
    want = len(g.fix_passes([ch.carry[0] for ch in lay.chunks]))
    h = handle(ctx, name)
    tz = ctx.table_upload(rm.to_bytes(ref(name)["z"]))
    ctx.sync()
    try:
        ctx.prof_enable(True); ctx.prof_reset()
        got = _multiply(ctx, h, tz)
        prof = {k: v[1] for k, v in ctx.prof_get().items()}
    finally:
        ctx.prof_enable(False); ctx.prof_reset()
        tz.free()
    assert got == ref(name)["mult"]
    assert (prof.get("k_r1cs_spmv"), prof.get("k_r1cs_fix")) == (1, want), prof


@pytest.mark.parametrize("name", LAZY)
def test_multiply_with_z_left_by_bind_top(ctx, name):
    """z is what sbn_bind_top leaves of a table of twice the length: lazy representatives of the same values, not what table_upload writes"""
    nv = g.instances()[name][1]
    z = ref(name)["z"]
    rng = random.Random(_seed(name) + 1)
    r = rng.randrange(2, R)
    lo = [rng.randrange(R) for _ in z]
    hi = [(a + (v - a) * pow(r, -1, R)) % R for a, v in zip(lo, z)]       # lo + r (hi - lo) = z
    t = ctx.table_upload(rm.to_bytes(lo + hi))
    try:
        ctx.bind_top(t, rm.to_bytes([r]))
        assert len(t) == 2 * nv and rm.from_bytes(ctx.table_download(t)) == z
        assert _multiply(ctx, handle(ctx, name), t) == ref(name)["mult"]
    finally:
        t.free()


@pytest.mark.parametrize("name", ["offsets_rows"] + SEAMS)
def test_is_sat(ctx, name):
    """the witness check over the same tables: values tuned (geometry untouched) so that the witness satisfies every row, then every row but row 0,
    one mid row and row num_cons - 1; verdict, count and first row against snark_model.is_sat"""
    nc, nv, mats = g.instances()[name][:3]
    z = ref(name)["z"][:nv] + [1] + ref(name)["z"][nv + 1:]
    vars_, inputs = z[:nv], z[nv + 1:]
    bad = [0, nc // 2 + 1, nc - 1]
    t = ctx.table_upload(rm.to_bytes(vars_))
    try:
        for violate in ([], bad):
            tuned = g.tuned(nc, nv, mats, z, violate)
            want = sm.is_sat(sm.Instance(nc, nv, nv - 1, tuned), vars_, inputs)
            assert want == ((False, 3, 0) if violate else (True, 0, None))
            h = _upload(ctx, nc, nv, tuned)
            try:
                sat, nb, fb = ctx.r1cs_is_sat(h, t, rm.to_bytes(inputs))
                assert (sat, nb) == want[:2] and (sat or fb == want[2]), violate
            finally:
                h.free()
    finally:
        t.free()


def test_mont_input(ctx):
    """the matrix seams uploaded as ark-ff Montgomery words (flags = 1)"""
    name = SEAMS[0]
    h = handle(ctx, name, mont=True)
    _check_multiply(ctx, h, name)
    _check_eval_table(ctx, h, name)
    _check_evaluate(ctx, h, name)
