"""GPU: a context's results must not depend on what it ran before.

sbn_ctx carries state from call to call ("What a context carries between calls"): workspace buffers that only grow, ticket counters and
a mailbox with a self-reset contract, the d_bad / h_bad pair, a pool that hands table buffers back with their old contents, side streams and
events, the profiling switch, the caller's stream, and the lazily built parts of a generator handle.  The other GPU modules exercise that state by
accident, on one session-wide context in collection order.  Here every test creates and closes its own context, so the state in front of the
predecessor is known, runs a predecessor, and then a small "victim" job whose expected value comes from the CPU references alone
(tests/ctx_state_jobs.py).  Everything is compared bit for bit.

  P0  no predecessor: the victim itself is right, so every later failure points at state
  P1  the same kind of job, 2x to 4x larger (more rows / instances / circuits too), every scalar and table entry r - 1, everything freed.  The pool
      rule: pool_get reuses a cached buffer whose size lies in [bytes, 2 bytes], so P1 also frees r - 1 tables of exactly the victim's table sizes and
      of twice them (ctx_state_jobs.stock_pool) — the victim's requests are served with another job's field elements, not with fresh zeros
  P2  a call of the same kind that fails, then the victim; and a failing call followed by a victim of a different kind
  P3  every other kind: the catalogue forwards, reversed and in a seeded shuffle on one context
  P4  profiling on, then off (the mailbox spin is skipped while it is on)
  P5  the caller's stream: sbn_ctx_set_stream with a torch stream and back to NULL, and an ordering test that would read zeros if the library ran
      anywhere but on the stream it was given
and one generator handle taken through every consumer that builds something on it lazily, in two orders and from two contexts."""
import random
import time

import pytest

import ctx_state_jobs as jobs
import oracle_lib
import polyeval_model as pem
import transcript_model as tm
from conftest import fr_bytes, rand_scalars

pytestmark = pytest.mark.gpu

IDS = ["V1", "V2", "V3", "V4", "V4c", "V5", "V6", "V7", "V8", "V8c", "V9", "V9j", "V10", "V11", "V12", "V13"]
DEFAULT_IDS = [i for i in IDS if i not in ("V2", "V3")]
# a failing call of one kind in front of a victim of another: every victim once as the victim and once as the failing call
CROSS = [("V1", "V6"), ("V13", "V1"), ("V4", "V9"), ("V9", "V4"), ("V5", "V7"), ("V6", "V13"), ("V10", "V8"), ("V8", "V10"), ("V11", "V12"), ("V12", "V11"),
         ("V7", "V4c"), ("V4c", "V5"), ("V9j", "V8c"), ("V1", "V9j"), ("V13", "V2"), ("V6", "V3"), ("V2", "V5"), ("V3", "V9"), ("V8c", "V1")]


@pytest.fixture(scope="module")
def cat(sbn):
    """the catalogue with every expected value in place: the CPU side once per module (about 5 s), V8c's layer loop on a context of its own"""
    victims = {v.id: v for v in jobs.catalogue()}
    assert list(victims) == IDS
    for v in victims.values():
        if not v.device_reference:
            v.expected()
    v8c = victims["V8c"]
    if v8c._expected is None:
        c = sbn.Context(0)
        try:
            v8c.loop_reference(c)
        finally:
            c.close()
    return victims


def _differs(got, want, path="result"):
    """the first place where two nested results differ (None when they are equal): an assertion message that stays short for megabyte values"""
    if isinstance(want, (tuple, list)) and isinstance(got, (tuple, list)):
        if len(got) != len(want):
            return f"{path}: {len(got)} items, expected {len(want)}"
        for i, (g, w) in enumerate(zip(got, want)):
            d = _differs(g, w, f"{path}[{i}]")
            if d:
                return d
        return None
    if got == want:
        return None
    if isinstance(want, (bytes, bytearray)) and isinstance(got, (bytes, bytearray)) and len(got) == len(want):
        at = next(i for i in range(len(want)) if got[i] != want[i])
        return f"{path}: bytes differ from offset {at} (entry {at // 32}): {bytes(got[at - at % 32:at - at % 32 + 32]).hex()} != {bytes(want[at - at % 32:at - at % 32 + 32]).hex()}"
    return f"{path}: {str(got)[:100]} != {str(want)[:100]}"


def _check(v, ctx, mp, what, **kw):
    d = _differs(v.run(ctx, mp, **kw), v.expected())
    assert d is None, f"{v.id} {what}: {d}"


@pytest.mark.parametrize("vid", IDS)
def test_p0_fresh_context(sbn, cat, monkeypatch, vid):
    v = cat[vid]
    ctx = jobs.make_context(sbn, monkeypatch, v.settings)
    try:
        _check(v, ctx, monkeypatch, "on a fresh context")
        _check(v, ctx, monkeypatch, "after itself")
        ctx.prof_enable(True); ctx.prof_reset()
        _check(v, ctx, monkeypatch, "with profiling on")
        v.check_path(ctx.prof_get())                        # the path the victim is in the catalogue for was the path taken
    finally:
        ctx.close()


@pytest.mark.parametrize("vid", IDS)
def test_p1_larger_extreme_job_then_freed(sbn, cat, monkeypatch, vid):
    """the same entry points at 2x to 4x the size with r - 1 everywhere, everything freed, tables of the victim's sizes and of twice them freed on top
    (the pool serves a request of `bytes` from any cached buffer in [bytes, 2 bytes]): the victim runs inside the larger job's leftovers"""
    v = cat[vid]
    ctx = jobs.make_context(sbn, monkeypatch, v.settings)
    try:
        v.p1(ctx, monkeypatch)
        jobs.stock_ladder(ctx)                              # the slabs' sizes are the library's own: a buffer at every power of two matches any of them
        _check(v, ctx, monkeypatch, "after its larger r - 1 predecessor")
    finally:
        ctx.close()


@pytest.mark.parametrize("vid", IDS)
def test_p2_failed_call_then_same_kind(sbn, cat, monkeypatch, vid):
    v = cat[vid]
    ctx = jobs.make_context(sbn, monkeypatch, v.settings)
    try:
        v.p2(ctx, monkeypatch, sbn.SbnError)
        _check(v, ctx, monkeypatch, "after a failed call of its own kind")
    finally:
        ctx.close()


@pytest.mark.parametrize("fail_id,vid", CROSS, ids=[f"{a}-then-{b}" for a, b in CROSS])
def test_p2_failed_call_then_other_kind(sbn, cat, monkeypatch, fail_id, vid):
    v = cat[vid]
    # the context of whichever of the two needs its own settings (a failed two-level-sort or GLV MSM only happens on such a context)
    ctx = jobs.make_context(sbn, monkeypatch, v.settings if v.settings != "default" else cat[fail_id].settings)
    try:
        cat[fail_id].p2(ctx, monkeypatch, sbn.SbnError)
        _check(v, ctx, monkeypatch, f"after a failed {fail_id} call")
    finally:
        ctx.close()


def test_p3_every_kind_in_three_orders(sbn, cat, monkeypatch):
    """the catalogue forwards, reversed and in a seeded shuffle on ONE context, every result checked every time"""
    order = [cat[i] for i in DEFAULT_IDS]
    shuffled = list(order); random.Random(20261017).shuffle(shuffled)
    ctx = jobs.make_context(sbn, monkeypatch)
    try:
        for name, seq in (("forwards", order), ("reversed", order[::-1]), ("shuffled", shuffled)):
            for k, v in enumerate(seq):
                _check(v, ctx, monkeypatch, f"{name}, after {seq[k - 1].id if k else 'the previous pass'}")
    finally:
        ctx.close()


@pytest.mark.parametrize("settings,ids", [("sort2", ["V2", "V4", "V5", "V2"]), ("glv", ["V3", "V5", "V4", "V3"])])
def test_p3_sort2_and_glv_contexts_among_other_kinds(sbn, cat, monkeypatch, settings, ids):
    """V2 and V3 need contexts of their own: each between other kinds of bucket jobs on its context"""
    ctx = jobs.make_context(sbn, monkeypatch, settings)
    try:
        for k, i in enumerate(ids):
            d = _differs(cat[i].run(ctx, monkeypatch), cat[i].expected())
            assert d is None, f"{i} at position {k} on the {settings} context: {d}"
    finally:
        ctx.close()


def test_p4_profiling_on_then_off(sbn, cat, monkeypatch):
    """with profiling on the mailbox spin is skipped and every wait is a stream synchronisation: the same bytes, and the same again once it is off"""
    order = [cat[i] for i in DEFAULT_IDS]
    ctx = jobs.make_context(sbn, monkeypatch)
    try:
        ctx.prof_enable(True)
        for v in order:
            ctx.prof_reset()
            _check(v, ctx, monkeypatch, "with profiling on")
            v.check_path(ctx.prof_get())
        ctx.prof_enable(False)
        for v in order:
            _check(v, ctx, monkeypatch, "with profiling off again")
    finally:
        ctx.prof_enable(False)
        ctx.close()


def test_p5a_callers_stream_and_back(sbn, cat, monkeypatch, ol):
    """sbn_ctx_set_stream with a torch stream, the catalogue, sbn_ctx_set_stream(NULL), the catalogue again; a table and a generator handle made before each
    switch are still valid after it"""
    import torch
    order = [cat[i] for i in DEFAULT_IDS]
    ctx = jobs.make_context(sbn, monkeypatch)
    s = torch.cuda.Stream()
    tb, tb1 = rand_scalars(1 << 10, 2500), rand_scalars(1 << 10, 2502)
    sc = rand_scalars(300, 2501)
    gxy = ol.gens_new(300, b"gens_ctx_state_stream")[0]
    want = (ol.msm_pippenger(sc, gxy[:64 * 300], 8), False)
    try:
        t0 = ctx.table_upload(tb)
        b0, _ = ctx.gens_new(300, b"gens_ctx_state_stream", want_points=False)
        ctx.set_stream(s.cuda_stream)
        assert ctx.table_download(t0) == tb and ctx.msm_bases(b0, sc) == want
        t1 = ctx.table_upload(tb1)
        for v in order:
            _check(v, ctx, monkeypatch, "on the caller's stream")
        ctx.set_stream(0)
        assert ctx.table_download(t0) == tb and ctx.table_download(t1) == tb1 and ctx.msm_bases(b0, sc) == want
        for v in order:
            _check(v, ctx, monkeypatch, "back on the context's own stream")
        for x in (t0, t1, b0):
            x.free()
    finally:
        ctx.set_stream(0)
        ctx.close()


CHAIN_MATMULS = 60           # fp32 4096 x 4096 x 4096 products queued in front of the copy that writes the real input: 58 ms on an MI355X


def _queue_chain(torch, a):
    x = a
    for _ in range(CHAIN_MATMULS):
        x = torch.mm(x, a)
        x = x * (1.0 / 64.0)
    return x


def ordering_run(sbn, v, mp, on_callers_stream=True):
    """the sequence of test_p5b -> (result, ms of the queued chain, ms of the victim call alone).  on_callers_stream=False is the hand-run control: the
    context stays on its own stream, where nothing orders it behind the copy"""
    import torch
    ctx = jobs.make_context(sbn, mp)
    s = torch.cuda.Stream()
    bases = None
    try:
        if v.id == "V1":
            real = torch.frombuffer(bytearray(v.sc), dtype=torch.uint8).cuda()
            bases = ctx.bases_upload(v.pts)
            kw = lambda t: {"scalars_dev": t.data_ptr(), "bases": bases}
        else:
            real = torch.cat([torch.from_numpy(h.copy()) for h in v.host]).cuda()
            kw = lambda t: {"tables_dev": t.data_ptr()}
        buf = torch.zeros_like(real)
        a = torch.randn((4096, 4096), dtype=torch.float32, device="cuda") * (1.0 / 64.0)
        _queue_chain(torch, a)                              # the first product of a process loads its kernels: not part of the timed chain
        torch.cuda.synchronize()
        if on_callers_stream:
            ctx.set_stream(s.cuda_stream)
        # once on the real input: the workspace is grown and the pool holds the victim's buffers, so the call below allocates nothing (an allocation
        # may wait for the whole device, which would hide a library that runs on the wrong stream)
        t = time.perf_counter()
        d = _differs(v.run(ctx, mp, **kw(real)), v.expected())
        assert d is None, f"{v.id} on its real device input: {d}"
        v.run(ctx, mp, **kw(real))
        own_ms = 1e3 * (time.perf_counter() - t) / 2
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with torch.cuda.stream(s):
            e0.record(s)
            keep = _queue_chain(torch, a)
            e1.record(s)
            buf.copy_(real, non_blocking=True)
            got = v.run(ctx, mp, **kw(buf))                 # at once: no host synchronisation between the copy and the call
        torch.cuda.synchronize()
        del keep
        return got, e0.elapsed_time(e1), own_ms
    finally:
        if bases is not None:
            bases.free()
        ctx.set_stream(0)
        ctx.close()


@pytest.mark.parametrize("vid", ["V1", "V7"])
def test_p5b_library_runs_on_the_callers_stream(sbn, cat, monkeypatch, vid, record_property):
    """The victim's device input starts as zeros.  On a torch stream s, a chain of torch kernels is queued in front of the copy that writes the real
    scalars, and the library is called at once, with no host synchronisation.  Its result must be the expected one: had the library run anywhere but on
    s, it would have read the zeros.  The call is made allocation-free by a warm-up run, because an allocation can wait for the whole device.

    Hand-run control (ordering_run(..., on_callers_stream=False), the context left on its own stream): V1 returned the identity and V7 the all-zero-table
    proof, the zero-input answers, so this test can fail.  Measured on an MI355X with torch events: the chain of 60 fp32 4096^3 products takes 58 ms; the
    victim call by itself (host wall time, the mean of the two warm-up runs with their frees and the comparison: an upper figure) takes 0.7 ms (V1) and 3.4 ms (V7, its 36 table copies included): the queued work is 79 and 17 times
    the call it holds back.  Both figures are printed and recorded as properties on every run."""
    got, chain_ms, own_ms = ordering_run(sbn, cat[vid], monkeypatch)
    record_property("chain_ms", chain_ms); record_property("victim_ms", own_ms)
    print(f"p5b {vid}: chain {chain_ms:.1f} ms, victim call {own_ms:.2f} ms")
    d = _differs(got, cat[vid].expected())
    assert d is None, f"{vid} did not wait for the work queued on the caller's stream: {d}"
    assert chain_ms > 10 * own_ms, f"the queued work ({chain_ms:.1f} ms) no longer dwarfs the victim call ({own_ms:.2f} ms): lengthen CHAIN_MATMULS"


# ---- one generator handle through every consumer that builds something on it ---------------------------------------------------------------------

HLABEL = b"gens_ctx_state_handle"
HN = 257                      # gens_new(257): 257 G points and h; as an opening's generator set: 256 G, Q_base, h


class _HandleOracle:
    """inputs and CPU expectations of the consumer steps, computed once (both orders and both contexts use the same generator label)"""
    _inst = None

    @classmethod
    def get(cls):
        if cls._inst is None:
            cls._inst = cls()
        return cls._inst

    def __init__(self):
        ol = oracle_lib
        self.gxy = ol.gens_new(HN, HLABEL)[0]
        G, h = self.gxy[:64 * HN], self.gxy[64 * HN:]
        self.sc = jobs.with_edges(rand_scalars(HN, 2601))
        self.msm = (ol.msm_pippenger(self.sc, G, 8), False)
        self.Z1, self.bl1 = rand_scalars(3 * HN, 2602), rand_scalars(3, 2603)
        self.rows1 = ol.commit_rows(self.Z1, self.bl1, 3, HN, G, h, 8)
        self.Z2, self.bl2 = jobs.with_edges(rand_scalars(3 * HN, 2604), at=HN), rand_scalars(3, 2605)
        self.rows2 = ol.commit_rows(self.Z2, self.bl2, 3, HN, G, h, 8)
        # the opening: ell = 16, 256 x 256
        rng = random.Random(2606)
        n = HN - 1
        self.ell = 16
        self.pZ = [rng.randrange(jobs.R) for _ in range(1 << self.ell)]
        self.pr = [rng.randrange(jobs.R) for _ in range(self.ell)]
        self.pbl = [rng.randrange(jobs.R) for _ in range(256)]
        self.pbz = rng.randrange(jobs.R)
        self.prnd = [rng.randrange(jobs.R) for _ in range(3 + 2 * 8)]
        self.pZr = pem.dot(self.pZ, pem.eq_evals(self.pr))
        m = tm.Transcript(b"ctx state handle")
        want, Cy, Cx = pem.prove(m, pem.split_gens(self.gxy, n), self.pZ, self.pbl, self.pr, self.pZr, self.pbz, self.prnd)
        self.opening = (pem.proof_bytes(want), Cx, Cy, m.state())
        # the bullet reduction over the first 256 generators with Q = q_scale * Q_base
        self.Qb = self.gxy[64 * n:64 * n + 64]
        self.qs = rand_scalars(1, 2607)
        self.ba, self.bb, self.bblind = rand_scalars(n, 2608), rand_scalars(n, 2609), rand_scalars(1, 2610)
        self.bvec, us = rand_scalars(16, 2611), rand_scalars(8, 2612)
        self.bullet = ol.bullet_prove(self.gxy[:64 * n], ol.g1_mul(self.Qb, self.qs), h, self.ba, self.bb, self.bblind, self.bvec, us)
        # split_at(100) and scale
        self.mid = 100
        self.zl, self.zr, self.zs, self.b1 = rand_scalars(self.mid, 2613), rand_scalars(HN - self.mid, 2614), rand_scalars(HN, 2615), rand_scalars(1, 2616)
        self.left = ol.commit(self.zl, self.b1, G[:64 * self.mid], h)
        self.right = ol.commit(self.zr, self.b1, G[64 * self.mid:], h)
        self.s = rand_scalars(1, 2617)
        scaled = b"".join(ol.g1_mul(G[64 * i:64 * i + 64], self.s) for i in range(HN))
        self.scaled = ol.commit(self.zs, self.b1, scaled, h)


def _step_glv_msm(sbn, ctx, b, o):
    assert ctx.msm_bases(b, o.sc) == o.msm
    job = ctx.prof_last_job()
    assert job["slots"] == 2 * HN * job["W"], job                 # the GLV path: d_glv now exists on the handle


def _step_commit(sbn, ctx, b, o):
    assert ctx.commit_rows(b, o.Z1, o.bl1, 3, HN)[0] == o.rows1   # builds the window table, uniq and its CSR (unless the lookup table is there)


def _step_precompute_commit(sbn, ctx, b, o):
    assert 7 <= ctx.bases_precompute(b, 64 << 20) <= 17
    assert ctx.commit_rows(b, o.Z2, o.bl2, 3, HN)[0] == o.rows2
    assert ctx.commit_rows(b, o.Z1, o.bl1, 3, HN)[0] == o.rows1


def _step_bullet_and_opening(sbn, ctx, b, o):
    n = HN - 1
    Gn, G1 = ctx.bases_split_at(b, n)
    ta, tb = ctx.table_upload(o.ba), ctx.table_upload(o.bb)
    try:
        st, Gamma = ctx.bullet_begin_scaled(Gn, o.Qb, o.qs, ta, tb, o.bblind)        # builds bullet_ext on the derived handle
        try:
            assert Gamma == o.bullet["Gamma"]
            L, _, Rp, _, _, _ = ctx.bullet_cross(st, o.bvec[:32], o.bvec[32:64])
            assert L == o.bullet["L"][:64] and Rp == o.bullet["R"][:64]
        finally:
            st.free()
    finally:
        for x in (ta, tb, Gn, G1):
            x.free()
    t = ctx.table_upload(fr_bytes(o.pZ))
    tr = sbn.Transcript(b"ctx state handle")
    try:
        proof, Cx, Cy = ctx.polyeval_prove(b, t, fr_bytes(o.pr), pem.sb(o.pZr), fr_bytes(o.prnd), tr, blinds=fr_bytes(o.pbl), blind_Zr=pem.sb(o.pbz))
        assert (proof, Cx, Cy, tr.state()) == o.opening
    finally:
        tr.free(); t.free()


def _step_split_and_scale(sbn, ctx, b, o):
    left, right = ctx.bases_split_at(b, o.mid)
    scaled = ctx.bases_scale(b, o.s)
    try:
        assert ctx.commit_rows(left, o.zl, o.b1, 1, o.mid)[0] == o.left
        assert ctx.commit_rows(right, o.zr, o.b1, 1, HN - o.mid)[0] == o.right
        assert ctx.commit_rows(scaled, o.zs, o.b1, 1, HN)[0] == o.scaled
    finally:
        for x in (left, right, scaled):
            x.free()


STEPS = [_step_glv_msm, _step_commit, _step_precompute_commit, _step_bullet_and_opening, _step_split_and_scale]
GLV_SMALL = {"SBN_SORT2_MIN": "512"}          # 2 x 257 half-scalars reach the two-level sort, which the GLV path needs


@pytest.mark.parametrize("order", ["forwards", "reversed"])
def test_handle_through_every_consumer(sbn, monkeypatch, ol, order):
    """one gens_new(257) handle: a GLV MSM (d_glv), a blinded row commit (window table, uniq + CSR), bases_precompute and commits (d_comb), the bullet
    reduction and a whole opening (bullet_ext), split_at / scale with a commit on each derived handle — and on a second fresh handle the same in reverse.
    Which lazily built parts exist when a call arrives differs between the orders; every result equals the oracle's in both"""
    o = _HandleOracle.get()
    ctx = jobs.make_context(sbn, monkeypatch, "glv", GLV_SMALL)
    try:
        b, gxy = ctx.gens_new(HN, HLABEL)
        try:
            assert gxy == o.gxy
            for step in (STEPS if order == "forwards" else STEPS[::-1]):
                step(sbn, ctx, b, o)
            for step in STEPS:                                      # and again with every part in place
                step(sbn, ctx, b, o)
        finally:
            b.free()
    finally:
        ctx.close()


def test_handle_shared_by_two_contexts(sbn, monkeypatch):
    """a third handle: the second context's first use comes after the first context built every lazy part"""
    o = _HandleOracle.get()
    c1 = jobs.make_context(sbn, monkeypatch, "glv", GLV_SMALL)
    c2 = jobs.make_context(sbn, monkeypatch, "glv", GLV_SMALL)
    try:
        b, _ = c1.gens_new(HN, HLABEL, want_points=False)
        try:
            for step in STEPS:
                step(sbn, c1, b, o)
            for step in STEPS[::-1]:
                step(sbn, c2, b, o)
            for step in STEPS:
                step(sbn, c1, b, o)
        finally:
            b.free()
    finally:
        c2.close(); c1.close()
