"""GPU: sbn_zk_sumcheck_prove_r1cs / sbn_zk_sumcheck_prove_quad against the literal model of the reference (tests/zk_sumcheck_model.py),
against a replay from the oracle's round sums at every kernel-variant edge of the fused round, against the round loop through the calls that
existed before them, and their edge cases and refusals."""
import random

import pytest

import zk_sumcheck_model as zm
from zk_sumcheck_model import R_MOD, Transcript

pytestmark = pytest.mark.gpu
KINDS = {"r1cs": (4, 4), "quad": (2, 3)}                    # tables, coefficients
LABEL_1, LABEL_N = b"gens_zk_gpu_pc", b"gens_zk_gpu_sc"


def _sbs(xs):
    return b"".join(zm.sb(x) for x in xs)


_GENS = {}


def _gens(ctx, n, l1=LABEL_1, ln=LABEL_N):
    """one (gens_1, gens_n) pair of handles per size and label for the whole module: the derived set is built once per pair"""
    key = (n, l1, ln)
    if key not in _GENS:
        b1, xy1 = ctx.gens_new(1, l1)
        bn, xyn = ctx.gens_new(n, ln)
        _GENS[key] = (b1, bn, zm.gens_1_of(xy1), zm.split_gens(xyn, n))
    return _GENS[key]


@pytest.fixture(scope="module", autouse=True)
def _free_gens():
    yield
    for b1, bn, _, _ in _GENS.values():
        b1.free(); bn.free()
    _GENS.clear()


def _claim(kind, tabs):
    if kind == "r1cs":
        return sum(t * (a * b - c) for t, a, b, c in zip(*tabs)) % R_MOD
    return zm.dot(*tabs)


def _case(kind, length, seed, zero=False):
    nt, n = KINDS[kind]
    rng = random.Random(seed)
    rounds = length.bit_length() - 1
    tabs = [[0 if zero else rng.randrange(R_MOD) for _ in range(length)] for _ in range(nt)]
    blind_claim = 0 if zero else rng.randrange(R_MOD)
    rnd = [0 if zero else rng.randrange(R_MOD) for _ in range(rounds * (n + 4))]
    return tabs, _claim(kind, tabs), blind_claim, rnd


def _call(ctx, kind, ts, b1, bn, claim, blind_claim, rnd, tr):
    fn = ctx.zk_sumcheck_prove_r1cs if kind == "r1cs" else ctx.zk_sumcheck_prove_quad
    return fn(*ts, b1, bn, zm.sb(claim), zm.sb(blind_claim), _sbs(rnd), tr)


def _model(kind, tr, rnd, claim, blind_claim, tabs, g1, gn):
    return (zm.prove_r1cs if kind == "r1cs" else zm.prove_quad)(tr, rnd, claim, blind_claim, *tabs, g1, gn)


def _device(ctx, sbn, kind, tabs, b1, bn, claim, blind_claim, rnd, label=b"zk gpu"):
    ts = [ctx.table_upload(_sbs(t)) for t in tabs]
    tr = sbn.Transcript(label)
    try:
        out = _call(ctx, kind, ts, b1, bn, claim, blind_claim, rnd, tr)
        assert all(len(t) == 1 for t in ts)                  # bound in place down to one entry ...
        assert [ctx.table_read0(t) for t in ts] == [out[2][32 * i:32 * i + 32] for i in range(len(ts))]     # ... which is the final claim
        return out, tr.state()
    finally:
        for t in ts:
            t.free()


@pytest.mark.parametrize("kind", ["r1cs", "quad"])
@pytest.mark.parametrize("length", [2, 4, 8, 16, 1 << 10])
def test_bit_exact_against_the_model(ctx, sbn, kind, length):
    """2: one round, the plain eval launch only; 4: the first fused bind; 2^10: several rounds"""
    nt, n = KINDS[kind]
    b1, bn, g1, gn = _gens(ctx, n)
    tabs, claim, blind_claim, rnd = _case(kind, length, 500 + length)
    tm = Transcript(b"zk gpu")
    want, want_r, want_fin, want_blind = _model(kind, tm, rnd, claim, blind_claim, tabs, g1, gn)
    (proof, r, fin, blind), state = _device(ctx, sbn, kind, tabs, b1, bn, claim, blind_claim, rnd)
    assert r == _sbs(want_r)
    assert proof == zm.proof_bytes(want)
    assert fin == _sbs(want_fin) and blind == zm.sb(want_blind)
    assert state == tm.state()
    tv = Transcript(b"zk gpu")
    got = zm.verify(tv, zm.proof_from_bytes(proof, n), zm.commit_one(claim, blind_claim, g1), length.bit_length() - 1, n - 1, g1, gn)
    assert got is not None and _sbs(got[1]) == r and tv.state() == state


# sbn_sc_bind_eval_r1cs / _quad (sc_bind_eval_common, abi_tables.inc) switch on q = len / 4: q <= 128 the four-lanes-per-index kernel, up to
# single_max / 2 = 8192 the lane-per-index kernel (one block: results straight to the mailbox; from q = 512 two blocks and the ticketed fold),
# above that the streaming k_sc_bind_eval_pf.  The first bind of a call at length L runs at q = L / 4; the lengths below are the smallest on
# each side of every switch.
EDGES = [1 << 9, 1 << 10, 1 << 11, 1 << 15, 1 << 16]


@pytest.mark.parametrize("kind", ["r1cs", "quad"])
@pytest.mark.parametrize("length", EDGES)
def test_replay_from_the_oracles_round_sums_at_the_kernel_variant_edges(ctx, sbn, ol, kind, length):
    import numpy as np
    nt, n = KINDS[kind]
    b1, bn, g1, gn = _gens(ctx, n)
    rounds = length.bit_length() - 1
    rng = random.Random(length)
    mem = ctx.dev_alloc(32 * length * nt)
    ctx.scalars_synthetic(0x2b5c + length, 0, length * nt, mem)
    raw = ctx.dev_download(mem, 32 * length * nt)
    host = [np.frombuffer(raw, dtype=np.uint8)[32 * length * i:32 * length * (i + 1)] for i in range(nt)]
    ts = [ctx.table_upload(h.tobytes()) for h in host]
    ctx.dev_free(mem)
    blind_claim = rng.randrange(R_MOD)
    rnd = [rng.randrange(R_MOD) for _ in range(rounds * (n + 4))]
    claim = rng.randrange(R_MOD)                            # (neither prover checks the claim: e1 = claim - e0 is taken on trust)
    tr = sbn.Transcript(b"zk replay")
    try:
        proof, r, fin, _ = _call(ctx, kind, ts, b1, bn, claim, blind_claim, rnd, tr)
        state = tr.state()
        if length >= 1 << 16:
            ctx.prof_enable(True); ctx.prof_reset()
            ts2 = [ctx.table_upload(h.tobytes()) for h in host]
            try:
                again = _call(ctx, kind, ts2, b1, bn, claim, blind_claim, rnd, sbn.Transcript(b"zk replay"))
                prof = ctx.prof_get()
            finally:
                ctx.prof_enable(False)
                for t in ts2:
                    t.free()
            assert again[0] == proof and again[1] == r
            assert prof["k_sc_bind_eval_%s_stream" % kind][1] >= 1      # the streaming kernel was reached
            assert prof["k_zk_round_tail"][1] == rounds
    finally:
        for t in ts:
            t.free()
    orc = ol.sc_prove_r1cs if kind == "r1cs" else ol.sc_prove_quad
    evals, finals = orc(*host, r)
    sums = [[zm.ib(e[32 * k:32 * k + 32]) for k in range(len(e) // 32)] for e in evals]
    tm = Transcript(b"zk replay")
    want, want_r = zm.replay(tm, rnd, claim, blind_claim, sums, g1, gn)
    assert _sbs(want_r) == r
    assert zm.proof_bytes(want) == proof
    assert b"".join(finals) == fin
    assert tm.state() == state


def _round_loop(ctx, sbn, kind, ts, b1, bn, claim, blind_claim, rnd, tr):
    """either prover assembled by the caller from the calls that existed before: sbn_sc_eval_*, sbn_sc_bind_eval_*, sbn_bind_top,
    sbn_unipoly_from_evals, one-row sbn_commit_rows, sbn_transcript_*, with the caller's own Fr arithmetic"""
    nt, n = KINDS[kind]
    rounds = len(ts[0]).bit_length() - 1
    ev_fn, be_fn = (ctx.sc_eval_r1cs, ctx.sc_bind_eval_r1cs) if kind == "r1cs" else (ctx.sc_eval_quad, ctx.sc_bind_eval_quad)
    com_n = lambda xs, b: ctx.commit_rows(bn, _sbs(xs), zm.sb(b), 1, n)[0]          # noqa: E731
    com_1 = lambda x, b: ctx.commit_rows(b1, zm.sb(x), zm.sb(b), 1, 1)[0]           # noqa: E731
    blinds_poly, blinds_evals = rnd[:rounds], rnd[rounds:2 * rounds]
    pos = 2 * rounds
    comm_claim = com_1(claim, blind_claim)
    proof, rs = b"", b""
    sums = ev_fn(*ts)
    for j in range(rounds):
        e = [zm.ib(sums[32 * k:32 * k + 32]) for k in range(n - 1)]
        co_b = sbn.unipoly_from_evals(_sbs([e[0], claim - e[0]] + e[1:]))
        co = [zm.ib(co_b[32 * k:32 * k + 32]) for k in range(n)]
        comm_poly = com_n(co, blinds_poly[j])
        tr.append_message(b"comm_poly", sbn.g1_compress(comm_poly))
        rj_b = tr.challenge_scalar(b"challenge_nextround"); rj = zm.ib(rj_b)
        if len(ts[0]) >= 4:
            sums = be_fn(*ts, rj_b)
        else:
            for t in ts:
                ctx.bind_top(t, rj_b)
        ev = zm.ib(sbn.unipoly_eval(co_b, rj_b))
        comm_eval = com_1(ev, blinds_evals[j])
        tr.append_message(b"comm_claim_per_round", sbn.g1_compress(comm_claim)); tr.append_message(b"comm_eval", sbn.g1_compress(comm_eval))
        w = [zm.ib(tr.challenge_scalar(b"combine_two_claims_to_one")) for _ in range(2)]
        target = (w[0] * claim + w[1] * ev) % R_MOD
        blind = (w[0] * (blind_claim if j == 0 else blinds_evals[j - 1]) + w[1] * blinds_evals[j]) % R_MOD
        a = zm.a_vector(w, rj, n)
        d_vec, r_delta, r_beta = rnd[pos:pos + n], rnd[pos + n], rnd[pos + n + 1]
        pos += n + 2
        tr.append_message(b"protocol-name", b"dot product proof")
        tr.append_message(b"Cx", sbn.g1_compress(comm_poly))
        tr.append_message(b"Cy", sbn.g1_compress(com_1(target, blind)))
        for s in a:
            tr.append_message(b"a", zm.sb(s))
        delta, beta = com_n(d_vec, r_delta), com_1(zm.dot(a, d_vec), r_beta)
        tr.append_message(b"delta", sbn.g1_compress(delta)); tr.append_message(b"beta", sbn.g1_compress(beta))
        c = zm.ib(tr.challenge_scalar(b"c"))
        z = [(c * x + d) % R_MOD for x, d in zip(co, d_vec)]
        proof += sbn.g1_compress(comm_poly) + sbn.g1_compress(comm_eval) + sbn.g1_compress(delta) + sbn.g1_compress(beta)
        proof += _sbs(z) + zm.sb(c * blinds_poly[j] + r_delta) + zm.sb(c * blind + r_beta)
        rs += rj_b
        claim, comm_claim = ev, comm_eval
    return proof, rs, b"".join(ctx.table_read0(t) for t in ts), zm.sb(blinds_evals[-1])


@pytest.mark.parametrize("kind", ["r1cs", "quad"])
@pytest.mark.parametrize("length", [1 << 12, 1 << 16])
def test_same_bytes_as_the_round_loop_through_the_earlier_abi(ctx, sbn, kind, length):
    nt, n = KINDS[kind]
    b1, bn, _, _ = _gens(ctx, n)
    rng = random.Random(length + 1)
    rounds = length.bit_length() - 1
    mem = ctx.dev_alloc(32 * length * nt)
    ctx.scalars_synthetic(0x77aa + length, 0, length * nt, mem)
    raw = ctx.dev_download(mem, 32 * length * nt)
    ctx.dev_free(mem)
    claim, blind_claim = rng.randrange(R_MOD), rng.randrange(R_MOD)
    rnd = [rng.randrange(R_MOD) for _ in range(rounds * (n + 4))]
    t1 = [ctx.table_upload(raw[32 * length * i:32 * length * (i + 1)]) for i in range(nt)]
    t2 = [ctx.table_upload(raw[32 * length * i:32 * length * (i + 1)]) for i in range(nt)]
    tr, tl = sbn.Transcript(b"zk loop"), sbn.Transcript(b"zk loop")
    try:
        one = _call(ctx, kind, t1, b1, bn, claim, blind_claim, rnd, tr)
        loop = _round_loop(ctx, sbn, kind, t2, b1, bn, claim, blind_claim, rnd, tl)
        assert one == loop
        assert tr.state() == tl.state()
    finally:
        for t in t1 + t2:
            t.free()


@pytest.mark.parametrize("kind", ["r1cs", "quad"])
def test_all_zero_tables_blinds_and_rnd_commit_to_infinity(ctx, sbn, ol, kind):
    nt, n = KINDS[kind]
    b1, bn, g1, gn = _gens(ctx, n)
    tabs, claim, blind_claim, rnd = _case(kind, 8, 1, zero=True)
    tm = Transcript(b"zk zero")
    want, want_r, want_fin, _ = _model(kind, tm, rnd, claim, blind_claim, tabs, g1, gn)
    assert all(p == zm.INF for p in want["comm_polys"] + want["comm_evals"]) and ol.g1_compress(zm.INF)[31] == 0x40
    (proof, r, fin, blind), state = _device(ctx, sbn, kind, tabs, b1, bn, claim, blind_claim, rnd, label=b"zk zero")
    assert proof == zm.proof_bytes(want) and r == _sbs(want_r) and fin == bytes(32 * nt) and blind == bytes(32)
    assert state == tm.state()


def _polyeval_once(ctx, sbn, bases, seed):
    import polyeval_model as pm
    ell = 6
    rng = random.Random(seed)
    Z = [rng.randrange(R_MOD) for _ in range(1 << ell)]
    r = [rng.randrange(R_MOD) for _ in range(ell)]
    rnd = [rng.randrange(R_MOD) for _ in range(3 + 2 * (ell - ell // 2))]
    t = ctx.table_upload(_sbs(Z))
    tr = sbn.Transcript(b"zk polyeval")
    try:
        return ctx.polyeval_prove(bases, t, _sbs(r), zm.sb(pm.dot(Z, pm.eq_evals(r))), _sbs(rnd), tr), tr.state()
    finally:
        t.free()


def test_results_do_not_depend_on_what_the_context_ran_before(sbn):
    """the mailbox and the derived generator sets are shared with sbn_polyeval_prove: each call, behind the other on one context, gives what it
    gives on a fresh context"""
    tabs, claim, blind_claim, rnd = _case("r1cs", 64, 77)

    def fresh():
        c = sbn.Context(0)
        b1, _ = c.gens_new(1, LABEL_1); b4, _ = c.gens_new(4, LABEL_N); pe, _ = c.gens_new(8 + 1, b"gens_zk_gpu_pe")
        return c, b1, b4, pe

    def done(c, *bases):
        for b in bases:
            b.free()
        c.close()

    c, b1, b4, pe = fresh()
    try:
        zk_alone = _device(c, sbn, "r1cs", tabs, b1, b4, claim, blind_claim, rnd)
    finally:
        done(c, b1, b4, pe)
    c, b1, b4, pe = fresh()
    try:
        pe_alone = _polyeval_once(c, sbn, pe, 5)
        zk_after_pe = _device(c, sbn, "r1cs", tabs, b1, b4, claim, blind_claim, rnd)
        pe_after_zk = _polyeval_once(c, sbn, pe, 5)
    finally:
        done(c, b1, b4, pe)
    assert zk_after_pe == zk_alone
    assert pe_after_zk == pe_alone


def test_two_generator_pairs_used_alternately_give_each_pairs_own_bytes(ctx, sbn):
    kind, n = "quad", 3
    pa = _gens(ctx, n)
    pb = _gens(ctx, n, b"gens_zk_gpu_pc2", b"gens_zk_gpu_sc2")
    px = (pb[0], pa[1], pb[2], pa[3])                        # the other gens_1 with the first gens_n: a third pair on pa's gens_n handle
    tabs, claim, blind_claim, rnd = _case(kind, 16, 31)
    want = []
    for _, _, g1, gn in (pa, pb, px):
        tm = Transcript(b"zk gpu")
        p, r, _, _ = _model(kind, tm, rnd, claim, blind_claim, tabs, g1, gn)
        want.append((zm.proof_bytes(p), _sbs(r), tm.state()))
    assert len({w[0] for w in want}) == 3
    for k in (0, 1, 2, 0, 2, 1, 0):
        b1, bn, _, _ = (pa, pb, px)[k]
        (proof, r, _, _), state = _device(ctx, sbn, kind, tabs, b1, bn, claim, blind_claim, rnd)
        assert (proof, r, state) == want[k]


@pytest.mark.parametrize("kind", ["r1cs", "quad"])
def test_every_refusal_leaves_the_transcript_and_the_tables_unchanged(ctx, sbn, kind):
    nt, n = KINDS[kind]
    b1, bn, _, _ = _gens(ctx, n)
    tabs, claim, blind_claim, rnd = _case(kind, 8, 3)
    ts = [ctx.table_upload(_sbs(t)) for t in tabs]
    short = ctx.table_upload(_sbs(tabs[0][:4]))
    # tables of 6 entries: rows 0 .. 2 of the 4 x 2 view of an 8-entry table through the identity addresses (sbn_gather_merge_rows returns
    # nrows * R entries for any nrows)
    addr = ctx.dev_alloc(4 * 8)
    ctx.dev_upload(addr, b"".join(i.to_bytes(4, "little") for i in range(8)))
    six = [ctx.gather_merge_rows([t], [addr], 8, 2, 0, 1, 3) for t in ts]
    assert all(len(t) == 6 for t in six) and [ctx.table_download(t) for t in six] == [_sbs(t[:6]) for t in tabs]
    one = [ctx.table_upload(_sbs(t[:1])) for t in tabs]
    wrong_n, _ = ctx.gens_new(n + 1, LABEL_N)
    two, _ = ctx.gens_new(2, LABEL_1)
    noh_n = ctx.bases_upload(ctx.bases_download(bn, 0, n))
    noh_1 = ctx.bases_upload(ctx.bases_download(b1, 0, 1))
    bad = bytes(31) + b"\xff"                                 # >= r
    tr = sbn.Transcript(b"zk gpu")
    before = tr.state()
    fn = sbn.lib().sbn_zk_sumcheck_prove_r1cs if kind == "r1cs" else sbn.lib().sbn_zk_sumcheck_prove_quad
    import ctypes as C
    buf = lambda k: (C.c_uint8 * k)()                        # noqa: E731

    def raw(tables, g1, gn_, cl, bc, rn, trh, outs=None):
        outs = outs or [buf(1024), buf(128), buf(128), buf(32)]
        return fn(ctx.h, *[t.h if t is not None else None for t in tables], g1, gn_, cl, bc, rn, trh, *outs)

    good = dict(tables=ts, g1=b1.h, gn_=bn.h, cl=zm.sb(claim), bc=zm.sb(blind_claim), rn=_sbs(rnd), trh=tr.h)
    cases = [dict(tables=ts[:-1] + [short]), dict(tables=six), dict(tables=ts[:-1] + [six[-1]]), dict(tables=[six[0]] + ts[1:]), dict(tables=one), dict(tables=ts[:-1] + [ts[0]]), dict(tables=ts[:-1] + [None]),
             dict(gn_=wrong_n.h), dict(gn_=noh_n.h), dict(g1=two.h), dict(g1=noh_1.h), dict(g1=None), dict(gn_=None),
             dict(cl=bad), dict(bc=bad), dict(cl=None), dict(bc=None), dict(rn=None), dict(trh=None),
             dict(rn=bad + _sbs(rnd[1:])), dict(rn=_sbs(rnd[:-1]) + bad), dict(rn=_sbs(rnd[:7]) + bad + _sbs(rnd[8:]))]
    cases += [dict(outs=[None if k == i else x for k, x in enumerate([buf(1024), buf(128), buf(128), buf(32)])]) for i in range(4)]
    try:
        for kw in cases:
            a = dict(good); a.update(kw)
            assert raw(**a) == -1, kw                        # SBN_EINVAL
            assert tr.state() == before
            assert [ctx.table_download(t) for t in ts] == [_sbs(t) for t in tabs]
            assert [ctx.table_download(t) for t in six] == [_sbs(t[:6]) for t in tabs]
        out = _call(ctx, kind, ts, b1, bn, claim, blind_claim, rnd, tr)      # and the good call moves both
        assert tr.state() != before and all(len(t) == 1 for t in ts) and len(out[1]) == 32 * 3
    finally:
        for t in ts + one + six + [short]:
            t.free()
        ctx.dev_free(addr)
        for b in (wrong_n, two, noh_n, noh_1):
            b.free()
