"""GPU: sbn_sumcheck_prove — the whole batched cubic sumcheck, transcript included, in one call — against a replay in Python.

The replay: the model transcript (tests/transcript_model.py), the CPU oracle's prove_cubic_batched loop for the sums and the final
claims, the reference's round logic (sumcheck.rs:269-301) in Python integers.  The oracle's loop takes its challenges up front, so
it is run on the challenges the device returned; the model then re-derives every round from the oracle's sums: round 0's sums
depend on no challenge, and round j + 1's are checked only after r_j was found equal, so the comparison is the sequential one."""
import pytest

import transcript_model as tm
from conftest import rand_scalars
from transcript_phase_lib import _begin, _check_against_replay, _int, _run, _split, _start, _tables

pytestmark = pytest.mark.gpu
R = tm.R_MOD


@pytest.mark.parametrize("pos", [0, 1, 77, 78, 82, 164, 165])
def test_device_transcript_start_phases(ctx, sbn, ol, pos):
    """2-entry tables: one round, so the call is the device transcript step alone, started at every kind of phase (a round that is two
    blocks, three blocks, one that ends exactly on a block, headers that straddle a block)"""
    _run(ctx, sbn, ol, 1, 0, 1, 100 + pos, pos=pos)
    _run(ctx, sbn, ol, 2, 1, 2, 300 + pos, pos=pos)


SHAPES = [(1, 0, 1), (1, 0, 2), (0, 1, 3), (3, 2, 8), (12, 6, 10), (12, 6, 15), (12, 6, 17), (16, 0, 17), (12, 6, 21)]


@pytest.mark.parametrize("n_par,n_seq,logn", SHAPES)
def test_prove_vs_replay(ctx, sbn, ol, n_par, n_seq, logn):
    _run(ctx, sbn, ol, n_par, n_seq, logn, 1000 + 37 * logn + n_par)


@pytest.mark.parametrize("n_par,n_seq,logn", [s for s in SHAPES if s[0] > 0])
def test_prove_begin_eq_vs_replay(ctx, sbn, ol, n_par, n_seq, logn):
    _run(ctx, sbn, ol, n_par, n_seq, logn, 2000 + 37 * logn + n_par, eq=True)


def test_prove_all_zero_tables(ctx, sbn, ol):
    _run(ctx, sbn, ol, 3, 2, 8, 3000, zero=True)
    _run(ctx, sbn, ol, 12, 6, 17, 3001, zero=True, claim=0)


def test_prove_claim_below_e0_wraps(ctx, sbn, ol):
    """claim = 0 with uniform tables: e1 = claim - e0 is negative before the reduction in every round's first step"""
    _run(ctx, sbn, ol, 3, 2, 8, 3100, claim=0)
    _run(ctx, sbn, ol, 12, 6, 10, 3101, claim=R - 1)


@pytest.mark.parametrize("n_par,n_seq,logn", [(1, 0, 1), (3, 2, 8), (12, 6, 10), (12, 6, 17), (0, 2, 12)])
def test_prove_equals_round_loop_with_host_transcript(ctx, sbn, ol, n_par, n_seq, logn):
    _run(ctx, sbn, ol, n_par, n_seq, logn, 4000 + logn, via_rounds=True)
    if n_par:
        _run(ctx, sbn, ol, n_par, n_seq, logn, 4100 + logn, via_rounds=True, eq=True)


def test_two_sumchecks_on_one_transcript(ctx, sbn, ol):
    n_par, n_seq = 4, 2
    tr, model = _start(sbn, b"two in a row", 40)
    for k, logn in enumerate((9, 16)):
        dev, host = _tables(ctx, 2 * n_par + 1 + 3 * n_seq, 1 << logn, 5000 + 50 * k)
        co = rand_scalars(n_par + n_seq, 5001 + k); claim = _int(rand_scalars(1, 5002 + k))
        st, _ = _begin(ctx, _split(dev, n_par, n_seq), co, None)
        polys, rs, finals = ctx.sumcheck_prove(st, tr, claim.to_bytes(32, "little"))
        st.free()
        _check_against_replay(ol, _split(host, n_par, n_seq), co, claim, model, polys, rs, finals)
        assert tr.state() == model.state()
        tr.append_message(b"between", b"sumchecks"); model.append_message(b"between", b"sumchecks")
        for t in dev:
            t.free()


def test_two_contexts_two_transcripts(ctx, sbn, ol):
    import threading
    other = sbn.Context(0)
    errs = []

    def work(cx, seed):
        try:
            for rep in range(2):
                _run(cx, sbn, ol, 5, 2, 13, seed + 10 * rep, pos=3 + seed % 100)
        except BaseException as e:      # noqa: BLE001 - reported by the main thread
            errs.append(e)
    try:
        ths = [threading.Thread(target=work, args=(cx, s)) for cx, s in ((ctx, 6000), (other, 6100))]
        for t in ths:
            t.start()
        for t in ths:
            t.join()
    finally:
        other.close()
    assert not errs, errs


def test_prove_errors(ctx, sbn):
    a, b, c2 = (ctx.table_upload(rand_scalars(8, s)) for s in (1, 2, 3))
    co = rand_scalars(1, 4)
    tr = sbn.Transcript(b"errors")
    before = tr.state()
    st, _ = ctx.sumcheck_begin([a], [b], c2, [], [], [], co)
    with pytest.raises(sbn.SbnError):
        ctx.sumcheck_prove(st, tr, R.to_bytes(32, "little"))             # claim not canonical
    assert tr.state() == before and len(st) == 8
    st.round(rand_scalars(1, 5))
    with pytest.raises(sbn.SbnError):
        ctx.sumcheck_prove(st, tr, bytes(32))                             # not a fresh state
    assert tr.state() == before
    st.free()
    for t in (a, b, c2):
        t.free()
