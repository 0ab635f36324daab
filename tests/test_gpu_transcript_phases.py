"""GPU: the two device transcript steps (k_tr_sumcheck_step, k_tr_layer_step; csrc/transcript_kernels.cuh) at every STROBE phase and every
closing shape, exact against tests/transcript_model.py, the oracle's sc_prove_cubic_batched and tests/product_proof_model.py.
tests/test_transcript_plan_cpu.py sweeps the host's plans over the same space without a device; here the kernels execute them.

A phase is reached with a filler message (transcript_phase_lib._start): the short filler leaves pos_begin at the filler's own header (or 0 where it
crosses a block), the long one (166 bytes more) arrives at the same pos with pos_begin = 0.  Both variants run wherever a sweep is over phases.

Counts (asserted by the parametrisation below):
  a  first round, 2-entry tables      166 phases x 2 variants x {(1, 0), (18, 6)}; {(15, 6), (16, 6)} at pos 0, 76, 77, 78, 165;
                                      {(0, 24), (24, 0), (21, 3)} at the 17 phases 0, 10, .., 160
  b  first round + a round from 64    166 phases x 2 variants x {(2, 1), (18, 6)}, 4-entry tables; the five other shapes of (a) at pos 0, 76, 77, 78, 165
  c  opening boundary                 166 phases x 2 variants x {(1, 0), (2, 1), (18, 6), (24, 0), (1, 23)}, two layers
  d  closing boundaries               the 300 pairs (n_circ >= 1, n_circ + n_dotp <= 24) at two layers, the 24 with n_dotp = 0 at one layer as well
  e  edge values                      zero tables with claim 0, claim r - 1, tables of r - 1, at pos 77 and 78, 2- and 4-entry tables, 18 + 6 instances
sbn_sumcheck_prove hands its FIRST step one slot whatever the instance count (the sums sbn_sumcheck_begin has combined), so in (a) the step runs
with one slot at every phase; a step with n_par + n_seq slots (the second pass s += 21 from 22 slots on) runs from pos 64: the second round of
(b) and (e), and the one round behind every opening boundary of (c) and (d)."""
import pytest

import transcript_model as tm
from conftest import fr_bytes
from transcript_phase_lib import R, _case_inputs, _proof_against_model, _run, _start, _tables, _upload_circuits

pytestmark = pytest.mark.gpu

PHASES = list(range(tm.RATE))
N_CHUNKS = 16
CHUNKS = [PHASES[i * len(PHASES) // N_CHUNKS:(i + 1) * len(PHASES) // N_CHUNKS] for i in range(N_CHUNKS)]
assert len({p for ch in CHUNKS for p in ch}) == 166 and sum(len(ch) for ch in CHUNKS) == 166
EDGE_PHASES = [0, 76, 77, 78, 165]                       # two blocks, the last two-block phase but one, a round that ends on a block, three blocks, the last
TENTH_PHASES = PHASES[::10]
SLOT_EDGES = [(15, 6), (16, 6)]                          # 21 slots: the first pass alone; 22: the second pass begins
SLOT_SPLITS = [(0, 24), (24, 0), (21, 3)]
OPEN_SHAPES = [(1, 0), (2, 1), (18, 6), (24, 0), (1, 23)]
PAIRS = [(nc, nd) for nc in range(1, 25) for nd in range(0, 25 - nc)]
assert len(set(PAIRS)) == 300
PAIR_CHUNKS = [[p for p in PAIRS if p[0] == nc] for nc in range(1, 25)]
assert len({p for ch in PAIR_CHUNKS for p in ch}) == 300 and sum(len(ch) for ch in PAIR_CHUNKS) == 300


@pytest.fixture(scope="module")
def tabs(ctx):
    """sumcheck tables per (n_par, n_seq, logn, kind), made once: the calls only read them"""
    made = {}

    def get(n_par, n_seq, logn, kind="uniform"):
        key = (n_par, n_seq, logn, kind)
        if key not in made:
            made[key] = _tables(ctx, 2 * n_par + (1 if n_par else 0) + 3 * n_seq, 1 << logn, 9000 + 100 * n_par + 10 * n_seq + logn,
                                zero=kind == "zero", value=R - 1 if kind == "r-1" else None)
        return made[key]
    yield get
    for dev, _ in made.values():
        for t in dev:
            t.free()


@pytest.fixture(scope="module")
def pool(ctx):
    """24 product circuits and 23 dot-product circuits per depth, uploaded once; a shape takes the first n_circ and n_dotp of them"""
    made = {}

    def get(L):
        if L not in made:
            ins, dots = _case_inputs(24, 23, L, 7000 + L)
            layers, owned = _upload_circuits(ctx, ins)
            dtabs = [tuple(ctx.table_upload(fr_bytes(t)) for t in d) for d in dots]
            made[L] = (ins, dots, layers, dtabs, owned + [t for d in dtabs for t in d])
        return made[L][:4]
    yield get
    for entry in made.values():
        for t in entry[4]:
            t.free()


def _sumcheck_at(ctx, sbn, ol, tabs, n_par, n_seq, logn, pos, long_filler, kind="uniform", claim=None):
    _run(ctx, sbn, ol, n_par, n_seq, logn, 50000 + 300 * pos + 10 * n_par + n_seq, pos=pos, long_filler=long_filler, claim=claim,
         tables=tabs(n_par, n_seq, logn, kind))


def _proof_at(ctx, sbn, pool, n_circ, n_dotp, L, pos=None, long_filler=False):
    ins, dots, layers, dtabs = pool(L)
    if pos is None:
        tr, m = sbn.Transcript(b"product proof phases"), tm.Transcript(b"product proof phases")
    else:
        tr, m = _start(sbn, b"product proof phases", pos, long_filler)
    try:
        _proof_against_model(ctx, sbn, ins[:n_circ], dots[:n_dotp], layers[:n_circ], dtabs[:n_dotp], L, tr, m, (n_circ, n_dotp, L, pos, long_filler), verify=False)
    finally:
        tr.free()


# ---- a. k_tr_sumcheck_step, the first round ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("chunk", range(N_CHUNKS))
def test_first_round_every_phase(ctx, sbn, ol, tabs, chunk):
    """2-entry tables: one round, the call is the step alone"""
    for pos in CHUNKS[chunk]:
        for long_filler in (False, True):
            _sumcheck_at(ctx, sbn, ol, tabs, 1, 0, 1, pos, long_filler)
            _sumcheck_at(ctx, sbn, ol, tabs, 18, 6, 1, pos, long_filler)


@pytest.mark.parametrize("pos", EDGE_PHASES)
def test_first_round_slot_edges(ctx, sbn, ol, tabs, pos):
    for n_par, n_seq in SLOT_EDGES:
        for long_filler in (False, True):
            _sumcheck_at(ctx, sbn, ol, tabs, n_par, n_seq, 1, pos, long_filler)


@pytest.mark.parametrize("pos", TENTH_PHASES)
def test_first_round_slot_splits(ctx, sbn, ol, tabs, pos):
    for n_par, n_seq in SLOT_SPLITS:
        for long_filler in (False, True):
            _sumcheck_at(ctx, sbn, ol, tabs, n_par, n_seq, 1, pos, long_filler)


# ---- b. the first round, then a round from pos 64 -------------------------------------------------------------------------------------

@pytest.mark.parametrize("chunk", range(N_CHUNKS))
def test_two_rounds_every_phase(ctx, sbn, ol, tabs, chunk):
    """4-entry tables: masks_first, then masks_next with every instance's sums in a slot of its own, the claim carried between the steps"""
    for pos in CHUNKS[chunk]:
        for long_filler in (False, True):
            _sumcheck_at(ctx, sbn, ol, tabs, 2, 1, 2, pos, long_filler)
            _sumcheck_at(ctx, sbn, ol, tabs, 18, 6, 2, pos, long_filler)


@pytest.mark.parametrize("pos", EDGE_PHASES)
def test_two_rounds_slot_edges_and_splits(ctx, sbn, ol, tabs, pos):
    """21, 22 and 24 slots in the second round's step: the second pass of the combination at its edges, and every split of 24"""
    for n_par, n_seq in SLOT_EDGES + SLOT_SPLITS:
        for long_filler in (False, True):
            _sumcheck_at(ctx, sbn, ol, tabs, n_par, n_seq, 2, pos, long_filler)


# ---- c. k_tr_layer_step, the opening step ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("chunk", range(N_CHUNKS))
@pytest.mark.parametrize("shape", OPEN_SHAPES)
def test_opening_step_every_phase(ctx, sbn, pool, shape, chunk):
    """two layers: the opening step at the caller's phase, then (from pos 64) close + open, one sumcheck round on the weights that step wrote, close"""
    for pos in CHUNKS[chunk]:
        for long_filler in (False, True):
            _proof_at(ctx, sbn, pool, shape[0], shape[1], 2, pos, long_filler)


# ---- d. k_tr_layer_step, the closing steps --------------------------------------------------------------------------------------------

@pytest.mark.parametrize("chunk", range(len(PAIR_CHUNKS)))
def test_closing_steps_every_shape(ctx, sbn, pool, chunk):
    for n_circ, n_dotp in PAIR_CHUNKS[chunk]:
        _proof_at(ctx, sbn, pool, n_circ, n_dotp, 2)


def test_closing_steps_one_layer(ctx, sbn, pool):
    """one layer: no sumcheck, the opening boundary and the closing one back to back"""
    shapes = [p for p in PAIRS if p[1] == 0]
    assert len(shapes) == 24
    for n_circ, _ in shapes:
        _proof_at(ctx, sbn, pool, n_circ, 0, 1)


# ---- e. edge values through the step's field arithmetic -------------------------------------------------------------------------------

@pytest.mark.parametrize("pos", [77, 78])
@pytest.mark.parametrize("logn", [1, 2])
def test_edge_values(ctx, sbn, ol, tabs, pos, logn):
    _sumcheck_at(ctx, sbn, ol, tabs, 18, 6, logn, pos, False, kind="zero", claim=0)
    _sumcheck_at(ctx, sbn, ol, tabs, 18, 6, logn, pos, False, claim=R - 1)
    _sumcheck_at(ctx, sbn, ol, tabs, 18, 6, logn, pos, False, kind="r-1")
    _sumcheck_at(ctx, sbn, ol, tabs, 18, 6, logn, pos, False, kind="r-1", claim=R - 1)
