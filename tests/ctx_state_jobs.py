"""The job catalogue of tests/test_gpu_ctx_state.py: small "victim" jobs, one per kind of entry point, and the predecessors that try to leave
state behind for them in a context.

Every victim has
  expected()       its result from the CPU references only (oracle_lib, pyref and the *_model modules), computed once and cached;
  run(ctx, mp)     the same job through the library on `ctx`, returned in the shape expected() has.  Everything the job makes (tables,
                   handles, states, raw device memory) is freed before it returns.  `mp` is pytest's monkeypatch: overrides the library
                   reads on every call (SBN_MSM_C, SBN_COMMIT_CHUNK_BYTES) are set around the call and removed again;
  p1(ctx, mp)      the same entry points at 2x to 4x the size (and more rows / instances / circuits where those size the workspace), every scalar
                   and table entry r - 1, everything freed afterwards: the workspace high-water mark ends above the victim's extent and the
                   table pool holds buffers the victim's requests match;
  p2(ctx, mp, E)   a call of the same kind that fails (E = SbnError), asserted with pytest.raises.
V8c is the exception for expected(): the Python model is too slow for 2^17-entry circuits, so its expected value is the layer loop through
sbn_sumcheck_begin_eq + sbn_sumcheck_round with the transcript on the host (loop_reference), run once on a context of its own.

stock_pool(ctx, sizes) implements the pool rule of P1: pool_get hands out any cached buffer whose size lies in [bytes, 2 bytes], so tables of exactly the
victim's table sizes and of twice them, filled with r - 1, are made and freed before the victim runs."""
import ctypes as C
import random

import numpy as np
import pytest

import dense_model as dm
import kzg_model as km
import oracle_lib as ol
import polyeval_model as pem
import product_proof_model as ppm
import pyref
import r1cs_model as rm
import transcript_model as tm
from conftest import fr_bytes, rand_scalars
from test_gpu_dense import SHAPES as DENSE_SHAPES, _instance as dense_instance
from test_gpu_r1cs import _instance as r1cs_instance

R = pyref.R
TOP = (R - 1).to_bytes(32, "little")
BAD = R.to_bytes(32, "little")                     # the smallest non-canonical scalar
G_XY = (1).to_bytes(32, "little") + (2).to_bytes(32, "little")
S0 = 0x1234567890abcdef1234567890abcdef
DSTEP = 0x0fedcba987654321
EDGES = [0, 1, R - 1, (1 << 253) % R]


def _int(b):
    return int.from_bytes(b, "little")


def _ints(b):
    return [int.from_bytes(b[32 * i:32 * i + 32], "little") for i in range(len(b) // 32)]


def wide_scalars(n, seed):
    """n canonical scalars of 253 bits as bytes (numpy: fast at hundreds of thousands)"""
    rng = np.random.default_rng(seed)
    k = rng.integers(0, 2**64, size=(n, 4), dtype=np.uint64)
    k[:, 3] &= np.uint64((1 << 61) - 1)
    return k.tobytes()


def with_edges(sc, at=0):
    sc = bytearray(sc)
    for i, v in enumerate(EDGES):
        sc[32 * (at + i):32 * (at + i + 1)] = v.to_bytes(32, "little")
    return bytes(sc)


def with_bad(sc):
    """a copy with a scalar >= r in the middle"""
    n = len(sc) // 32
    bad = bytearray(sc); bad[32 * (n // 2):32 * (n // 2) + 32] = BAD
    return bytes(bad)


def top_table(n):
    """n entries r - 1 as a numpy array (one host array serves every upload of that length)"""
    return np.frombuffer(TOP * n, dtype=np.uint8)


def tiled_bases(n, distinct, seed):
    dl = rand_scalars(distinct, seed)
    pts = ol.g1_mul_gen_batch(dl, 8)
    reps = (n + distinct - 1) // distinct
    return (pts * reps)[:64 * n], (dl * reps)[:32 * n]


def dlog_sum(scal, first, n):
    """sum_i k_i (S0 + (first + i) DSTEP) mod r: the discrete log of an MSM over sbn_bases_synthetic's points"""
    k16 = np.frombuffer(scal, dtype="<u2").reshape(n, 16).astype(np.int64)
    idx = np.arange(first, first + n, dtype=np.int64)
    sk, sik = 0, 0
    for j in range(16):
        col = k16[:, j]
        sk += int(col.sum()) << (16 * j)
        sik += (int((col * (idx & 0xFFFF)).sum()) + (int((col * (idx >> 16)).sum()) << 16)) << (16 * j)
    return (S0 * sk + DSTEP * sik) % R


def stock_pool(ctx, sizes):
    """tables of every length in `sizes` and of twice it, all entries r - 1, made and then freed: what pool_get will hand to the next requests of those sizes"""
    made = []
    for n in sorted(set(sizes)):
        for m in (n, 2 * n):
            made += [ctx.table_upload(top_table(m)) for _ in range(2)]
    for t in made:
        t.free()


LADDER_TOP = 21


def stock_ladder(ctx):
    """one r - 1 buffer of every power of two from 32 B to 64 MiB (2^21 entries), made and then freed.  The working slabs of the sumcheck, the product proof,
    the bullet reduction and the opening come from the pool as well, at sizes only the library's own formulas know (V6 about 1.2 MB, V7 about 54 MB, V8 about
    38 KB, V8c about 29 MB); with a buffer at every power of two, any request up to 64 MiB finds one in [bytes, 2 bytes] and is served with r - 1 entries"""
    made = [ctx.table_upload(top_table(1 << k)) for k in range(LADDER_TOP + 1)]
    for t in made:
        t.free()


COMB_KERNELS = ("k_sc_comb_eval", "k_sc_eval_mixed", "k_sc_comb_bind_eval", "k_sc_comb_bind_eval_first", "k_sc_round_mixed", "k_sc_round_mixed_first")


def launches(ran, name):
    """launches of kernel `name` in a prof_get() result (0 if it never ran)"""
    return ran.get(name, (0.0, 0))[1]


def dev_u32(ctx, arr, keep):
    p = ctx.dev_alloc(arr.nbytes); keep.append(p)
    ctx.dev_upload(p, arr.tobytes())
    return p


class Victim:
    id = "?"
    settings = "default"          # which context the job needs: "default", "sort2" (SBN_SORT2_MIN=1024) or "glv" (+ SBN_MSM_GLV=1)
    pool_sizes = ()               # lengths of the tables the job takes from the pool
    device_reference = False
    _expected = None

    def expected(self):
        if self._expected is None:
            self._expected = self.compute()
        return self._expected

    def compute(self):
        raise NotImplementedError

    def check_path(self, ran):
        """ran: prof_get() of one run() with profiling on -> asserts the kernels of the path the victim is in the catalogue for"""

    def __repr__(self):
        return self.id


# ---- V1 .. V3: single MSMs ----------------------------------------------------------------------------------------------------------

class V1(Victim):
    """sbn_msm, n = 3001: the c = 7 rule of small single MSMs, one-level sort; 256 distinct bases tiled, edge scalars"""
    id = "V1"
    n = 3001

    def __init__(self):
        self.pts, self.dl = tiled_bases(self.n, 256, 1101)
        self.sc = with_edges(rand_scalars(self.n, 1102))

    def compute(self):
        return ol.msm_pippenger(self.sc, self.pts, 8), False

    def run(self, ctx, mp, scalars_dev=None, bases=None):
        if scalars_dev is not None:                        # P5(b): the caller's resident bases, scalars read from the caller's device buffer
            return ctx.msm_bases_dev(bases, scalars_dev, self.n)
        out = ctx.msm(self.sc, self.pts)
        assert ctx.prof_last_job()["c"] == 7
        return out

    def check_path(self, ran):
        assert launches(ran, "k_hist_lds") == 1 and launches(ran, "k_scatter_lds") == 1 and not any(k.startswith("k_s2_") for k in ran), ran    # the one-level sort

    def p1(self, ctx, mp):
        ctx.msm(TOP * (4 * self.n), self.pts * 4)

    def p2(self, ctx, mp, E):
        with pytest.raises(E, match="canonical"):
            ctx.msm(with_bad(self.sc), self.pts)


class V2(Victim):
    """sbn_msm through the two-level sort: SBN_SORT2_MIN=1024 at creation, SBN_MSM_C=17, n = 8193 (one chunk of 8192 + 1)"""
    id = "V2"
    settings = "sort2"
    n = 8193

    def __init__(self):
        self.pts, self.dl = tiled_bases(self.n, 4096, 1201)
        self.sc = with_edges(rand_scalars(self.n, 1202))

    def compute(self):
        return ol.g1_mul(G_XY, ol.fr_dot(self.sc, self.dl)), False

    def _msm(self, ctx, mp, sc, pts):
        mp.setenv("SBN_MSM_C", "17")
        try:
            out = ctx.msm(sc, pts)
        finally:
            mp.delenv("SBN_MSM_C")
        return out

    def run(self, ctx, mp):
        out = self._msm(ctx, mp, self.sc, self.pts)
        assert ctx.prof_last_job()["c"] == 17
        return out

    def check_path(self, ran):
        assert launches(ran, "k_s2_hist") == 1 and launches(ran, "k_s2_scatter") == 1 and launches(ran, "k_s2_place") == 1, ran                  # the two-level sort ...
        assert "k_hist_lds" not in ran and "k_scatter_lds" not in ran and "k_glv_split" not in ran, ran                                          # ... and not the one-level one

    def p1(self, ctx, mp):
        self._msm(ctx, mp, TOP * (4 * self.n), self.pts * 4)

    def p2(self, ctx, mp, E):
        with pytest.raises(E, match="canonical"):
            self._msm(ctx, mp, with_bad(self.sc), self.pts)


class V3(Victim):
    """sbn_msm_bases over the GLV endomorphism: SBN_MSM_GLV=1 and SBN_SORT2_MIN=1024 at creation, resident synthetic bases, n = 3001"""
    id = "V3"
    settings = "glv"
    n, first = 3001, 3

    def __init__(self):
        self.sc = with_edges(wide_scalars(self.n, 1301))

    def compute(self):
        return ol.g1_mul(G_XY, dlog_sum(self.sc, self.first, self.n).to_bytes(32, "little")), False

    def _msm(self, ctx, n, sc):
        b = ctx.bases_synthetic(n, self.first, S0.to_bytes(32, "little"), DSTEP.to_bytes(32, "little"))
        try:
            return ctx.msm_bases(b, sc)
        finally:
            b.free()

    def run(self, ctx, mp):
        out = self._msm(ctx, self.n, self.sc)
        job = ctx.prof_last_job()
        assert 13 <= job["c"] <= 17 and job["slots"] == 2 * self.n * job["W"]          # 2n half-scalars per window: the GLV path
        return out

    def check_path(self, ran):
        assert launches(ran, "k_glv_split") == 1 and launches(ran, "k_glv_table") == 1 and launches(ran, "k_s2_scatter") == 1, ran

    def p1(self, ctx, mp):
        self._msm(ctx, 4 * self.n, TOP * (4 * self.n))

    def p2(self, ctx, mp, E):
        with pytest.raises(E):
            self._msm(ctx, self.n, with_bad(self.sc))


# ---- V4, V4c, V5: row commitments ---------------------------------------------------------------------------------------------------

class V4(Victim):
    """sbn_commit_rows from a host pointer, bucket path: 5 x 1000 over gens_r1cs_sat (equal bases merged), blinds, a zero and a constant row"""
    id = "V4"
    L, Rn, label = 5, 1000, b"gens_r1cs_sat"
    lookup_bytes = p1_lookup_bytes = 0
    chunk_rows = 0
    p1_L, p1_R = 15, 4000

    def __init__(self):
        L, Rn = self.L, self.Rn
        self.gxy = ol.gens_new(Rn, self.label)[0]
        Z = bytearray(with_edges(rand_scalars(L * Rn, 1400 + Rn), at=3 * Rn))
        Z[32 * Rn:64 * Rn] = bytes(32 * Rn)
        Z[64 * Rn:96 * Rn] = Z[64 * Rn:64 * Rn + 32] * Rn
        self.Z = bytes(Z); self.bl = rand_scalars(L, 1401 + Rn)

    def compute(self):
        out = ol.commit_rows(self.Z, self.bl, self.L, self.Rn, self.gxy[:64 * self.Rn], self.gxy[64 * self.Rn:], 8)
        return out, bytes(int(out[64 * i:64 * i + 64] == bytes(64)) for i in range(self.L))

    def _commit(self, ctx, mp, Rn, L, Z, bl, check_gens=False, lookup_bytes=None):
        b, gxy = ctx.gens_new(Rn, self.label, want_points=check_gens)
        try:
            if check_gens:
                assert gxy == self.gxy
            lookup_bytes = self.lookup_bytes if lookup_bytes is None else lookup_bytes
            if lookup_bytes:
                ctx.bases_precompute(b, lookup_bytes)
            if self.chunk_rows:
                mp.setenv("SBN_COMMIT_CHUNK_BYTES", str(self.chunk_rows * Rn * 32))
            try:
                return ctx.commit_rows(b, Z, bl, L, Rn)
            finally:
                if self.chunk_rows:
                    mp.delenv("SBN_COMMIT_CHUNK_BYTES")
        finally:
            b.free()

    def run(self, ctx, mp):
        return self._commit(ctx, mp, self.Rn, self.L, self.Z, self.bl, check_gens=True)

    def check_path(self, ran):
        chunks = -(-self.L // self.chunk_rows) if self.chunk_rows else 1
        if self.lookup_bytes:
            assert launches(ran, "k_comb_rows") + launches(ran, "k_comb_rows_const") >= 1 and "k_sort_rows" not in ran, ran      # d_comb was built and used: no bucket sort of the rows
        else:
            assert launches(ran, "k_sort_rows") == chunks and "k_comb_rows" not in ran, ran       # the bucket path, once per chunk (SBN_COMMIT_CHUNK_BYTES is read on every call)

    def p1(self, ctx, mp):
        self._commit(ctx, mp, self.p1_R, self.p1_L, TOP * (self.p1_L * self.p1_R), TOP * self.p1_L, lookup_bytes=self.p1_lookup_bytes)

    def p2(self, ctx, mp, E):
        with pytest.raises(E, match="canonical"):
            self._commit(ctx, mp, self.Rn, self.L, with_bad(self.Z), self.bl)


class V4c(V4):
    """V4 through the chunked host path (SBN_COMMIT_CHUNK_BYTES = 2 rows: two staging buffers, copy_stream, z_consumed): 3 chunks, the last ragged"""
    id = "V4c"
    chunk_rows = 2


class V5(V4):
    """sbn_commit_rows by the fixed-base lookup table: 9 x 64 over gens_r1cs_eval after sbn_bases_precompute(8 MB)"""
    id = "V5"
    L, Rn, label = 9, 64, b"gens_r1cs_eval"
    lookup_bytes, p1_lookup_bytes = 8 << 20, 64 << 20
    p1_L, p1_R = 36, 256


# ---- V6, V7: the batched cubic sumcheck in one call ---------------------------------------------------------------------------------

class V6(Victim):
    """sbn_sumcheck_begin + sbn_sumcheck_prove, 2^10-entry tables, 12 par + 6 seq: single-launch rounds (tickets and the host mailbox)"""
    id = "V6"
    logn, n_par, n_seq = 10, 12, 6
    p1_logn, p1_par, p1_seq = 12, 16, 8
    label = b"ctx state sumcheck"

    def __init__(self):
        n = 1 << self.logn
        self.ntab = 2 * self.n_par + 1 + 3 * self.n_seq
        self.pool_sizes = (n,)
        raw = np.frombuffer(wide_scalars(self.ntab * n, 1600 + self.logn), dtype=np.uint8).reshape(self.ntab, 32 * n).copy()
        for k in range(self.ntab):                        # full-width values too: r - 1 at a few places of every table
            for i in (k % n, (7 * k + 3) % n):
                raw[k, 32 * i:32 * i + 32] = np.frombuffer(TOP, dtype=np.uint8)
        self.host = [raw[k] for k in range(self.ntab)]
        self.co = rand_scalars(self.n_par + self.n_seq, 1601 + self.logn)
        self.claim = _int(rand_scalars(1, 1602 + self.logn))

    def _split(self, lst, n_par, n_seq):
        o = 2 * n_par + 1
        return lst[:n_par], lst[n_par:2 * n_par], lst[2 * n_par], lst[o:o + n_seq], lst[o + n_seq:o + 2 * n_seq], lst[o + 2 * n_seq:]

    def compute(self):
        """sequential on the CPU: round j's sums come from the oracle's loop run on the challenges found so far (they depend on r_0 .. r_{j-1}
        only), the round polynomial and r_j from the model transcript"""
        parts = self._split(self.host, self.n_par, self.n_seq)
        model = tm.Transcript(self.label)
        e, polys, rs = self.claim, [], []
        for j in range(self.logn):
            ch = b"".join(rs) + bytes(32 * (self.logn - j))
            _, comb, _ = ol.sc_prove_cubic_batched(*parts, self.co, ch, 8)
            e0, e2, e3 = (_int(comb[j][32 * k:32 * k + 32]) for k in range(3))
            cj, rj, e = tm.sumcheck_round_step(model, e, e0, e2, e3)
            polys.append([c.to_bytes(32, "little") for c in cj]); rs.append(rj.to_bytes(32, "little"))
        _, _, fin = ol.sc_prove_cubic_batched(*parts, self.co, b"".join(rs), 8)
        return polys, rs, fin, model.state()

    def _prove(self, ctx, tabs, n_par, n_seq, co, claim, sbn_mod):
        try:
            tr = sbn_mod.Transcript(self.label)
            st, _ = ctx.sumcheck_begin(*self._split(tabs, n_par, n_seq), co)
            try:
                polys, rs, fin = ctx.sumcheck_prove(st, tr, claim)
            finally:
                st.free()
            state = tr.state(); tr.free()
            return polys, rs, fin, state
        finally:
            for t in tabs:
                t.free()

    def run(self, ctx, mp, tables_dev=None):
        import spartan_bn254_amd as sbn_mod
        n = 1 << self.logn
        if tables_dev is not None:                         # P5(b): the tables are copies of the caller's device buffer
            tabs = [ctx.table_from_dev(tables_dev + 32 * n * k, n) for k in range(self.ntab)]
        else:
            tabs = [ctx.table_upload(h) for h in self.host]
        return self._prove(ctx, tabs, self.n_par, self.n_seq, self.co, self.claim.to_bytes(32, "little"), sbn_mod)

    def check_path(self, ran):
        assert launches(ran, "k_tr_sumcheck_step") == self.logn, ran                                  # the transcript on the device, once per round
        if self.logn < 16:                                                                            # scaled per-instance path, single-launch rounds only
            assert launches(ran, "k_sc_scale") == 1 and launches(ran, "k_sc_bind_eval_cubic") == self.logn - 1, ran
            assert not any(k in ran for k in COMB_KERNELS) and "k_sc_bind_eval_cubic_stream" not in ran, ran
        else:                                                                                         # the combined kernels: coefficients folded in at the first bind
            assert launches(ran, "k_sc_comb_eval") == 1 and launches(ran, "k_sc_first_uv") == 1 and "k_sc_scale" not in ran, ran
            assert launches(ran, "k_sc_round_mixed_first") + launches(ran, "k_sc_comb_bind_eval_first") == 1, ran

    def p1(self, ctx, mp):
        import spartan_bn254_amd as sbn_mod
        n = 1 << self.p1_logn
        top = top_table(n)
        tabs = [ctx.table_upload(top) for _ in range(2 * self.p1_par + 1 + 3 * self.p1_seq)]
        self._prove(ctx, tabs, self.p1_par, self.p1_seq, TOP * (self.p1_par + self.p1_seq), TOP, sbn_mod)
        stock_pool(ctx, self.pool_sizes)

    def p2(self, ctx, mp, E):
        """the argument errors of test_stateful_sumcheck_errors and test_prove_errors, after a round has run on the state"""
        import spartan_bn254_amd as sbn_mod
        a, b, c2 = (ctx.table_upload(rand_scalars(8, s)) for s in (1, 2, 3))
        short = ctx.table_upload(rand_scalars(4, 4))
        tr = sbn_mod.Transcript(b"errors")
        try:
            with pytest.raises(E):
                ctx.sumcheck_begin([a], [short], c2, [], [], [], rand_scalars(1, 5))
            with pytest.raises(E):
                ctx.sumcheck_begin([a], [b], c2, [], [], [], BAD)
            st, _ = ctx.sumcheck_begin([a], [b], c2, [], [], [], rand_scalars(1, 5))
            with pytest.raises(E):
                ctx.sumcheck_prove(st, tr, BAD)
            with pytest.raises(E):
                st.round(BAD)
            st.round(rand_scalars(1, 6))
            with pytest.raises(E):
                ctx.sumcheck_prove(st, tr, bytes(32))           # not a fresh state
            with pytest.raises(E):
                st.finish()                                       # variables left
            st.free()
        finally:
            tr.free()
            for t in (a, b, c2, short):
                t.free()


class V7(V6):
    """the same at 2^16 entries, 13 par + 3 seq: the combined kernels (coefficients folded into A at the first bind), then the streaming and single-launch rounds"""
    id = "V7"
    logn, n_par, n_seq = 16, 13, 3
    p1_logn, p1_par, p1_seq = 17, 16, 8


# ---- V8, V8c: the layered product-circuit argument ----------------------------------------------------------------------------------

def _raw_product_proof(sbn_mod, ctx, layers, n, L, dtabs, tr):
    arr = (C.c_void_p * (n * L))(*[layers[i][j].h for i in range(n) for j in range(L)])
    mk = lambda k: (C.c_void_p * max(1, len(dtabs)))(*[d[k].h for d in dtabs])
    bufs = [(C.c_uint8 * 65536)() for _ in range(4)]
    return sbn_mod.lib().sbn_product_proof_prove(ctx.h, arr, C.c_size_t(n), C.c_size_t(L), mk(0), mk(1), mk(2), C.c_size_t(len(dtabs)), tr.h if tr else None, *bufs)


class V8(Victim):
    """sbn_product_circuit_many + sbn_product_proof_prove, 12 circuits of 2^6 and 6 dot-product circuits: PLAIN layers only"""
    id = "V8"
    n_circ, n_dotp, L = 12, 6, 6
    label = b"ctx state product proof"

    def __init__(self):
        N, h = 1 << self.L, 1 << (self.L - 1)
        self.pool_sizes = tuple(1 << k for k in range(1, self.L + 1))
        vals = pyref.prng_scalars(self.n_circ * N + 3 * self.n_dotp * h, 1800)
        vals[5] = R - 1; vals[N + 1] = 1
        self.ins = [vals[i * N:(i + 1) * N] for i in range(self.n_circ)]
        o = self.n_circ * N
        self.dots = [tuple(vals[o + (3 * k + t) * h:o + (3 * k + t + 1) * h] for t in range(3)) for k in range(self.n_dotp)]

    def compute(self):
        m = tm.Transcript(self.label)
        want = ppm.prove(m, [ppm.product_circuit(v) for v in self.ins], self.dots)
        return ppm.proof_to_flat(want) + (m.state(),)

    def _prove(self, ctx, ins, dtabs):
        import spartan_bn254_amd as sbn_mod
        owned = list(ins) + [t for d in dtabs for t in d]
        try:
            pcs = ctx.product_circuit_many(ins)
            owned += [t for pc in pcs for t in pc]
            layers = [[ins[i]] + pcs[i][:-1] for i in range(len(ins))]
            tr = sbn_mod.Transcript(self.label)
            got = ctx.product_proof_prove(layers, dtabs, tr)
            state = tr.state(); tr.free()
            return got + (state,)
        finally:
            for t in owned:
                t.free()

    def run(self, ctx, mp):
        ins = [ctx.table_upload(fr_bytes(v)) for v in self.ins]
        dtabs = [tuple(ctx.table_upload(fr_bytes(t)) for t in d) for d in self.dots]
        return self._prove(ctx, ins, dtabs)

    def check_path(self, ran):
        assert launches(ran, "k_tr_layer_step") == self.L + 1, ran
        if self.L < 16:                                                                               # PLAIN layers only
            assert not any(k in ran for k in COMB_KERNELS) and "k_pp_unscale" not in ran and "k_sc_first_uv" not in ran, ran
        else:                                                                                         # a COMB layer: combined kernels, and the coefficients taken out again
            assert launches(ran, "k_sc_comb_eval") >= 1 and launches(ran, "k_sc_comb_bind_eval_first") + launches(ran, "k_sc_round_mixed_first") >= 1, ran
            assert launches(ran, "k_pp_unscale") >= 1 and launches(ran, "k_sc_first_uv") >= 1, ran

    def p1(self, ctx, mp):
        N = 1 << (self.L + 2)
        ins = [ctx.table_upload(top_table(N)) for _ in range(16)]
        dtabs = [tuple(ctx.table_upload(top_table(N // 2)) for _ in range(3)) for _ in range(7)]
        self._prove(ctx, ins, dtabs)
        stock_pool(ctx, self.pool_sizes)

    def p2(self, ctx, mp, E):
        """the argument errors of test_errors_leave_the_transcript_alone, after a good call on the same tables"""
        import spartan_bn254_amd as sbn_mod
        ins = [ctx.table_upload(rand_scalars(16, 70 + i)) for i in range(2)]
        pcs = ctx.product_circuit_many(ins)
        layers = [[ins[i]] + pcs[i][:-1] for i in range(2)]
        dtabs = [tuple(ctx.table_upload(rand_scalars(8, 80 + k)) for k in range(3))]
        tr = sbn_mod.Transcript(b"errors")
        try:
            assert _raw_product_proof(sbn_mod, ctx, layers, 2, 4, dtabs, tr) == 0
            before = tr.state()
            swapped = [list(layers[0]), list(layers[1])]; swapped[0][1], swapped[0][2] = swapped[0][2], swapped[0][1]
            assert _raw_product_proof(sbn_mod, ctx, swapped, 2, 4, dtabs, tr) == -1 and tr.state() == before
            assert _raw_product_proof(sbn_mod, ctx, layers, 2, 4, dtabs, None) == -1
            with pytest.raises(E):
                ctx.product_proof_prove([layers[0][:3], layers[1][:3]], dtabs, tr)      # the dot-product circuits no longer fit the depth
            assert tr.state() == before
        finally:
            tr.free()
            for t in ins + [t for pc in pcs for t in pc] + list(dtabs[0]):
                t.free()


class V8c(V8):
    """sbn_product_proof_prove with COMB layers: 8 circuits of 2^17 (the coefficient inversion runs on pp_stream beside the layer's sumcheck); inputs
    from sbn_scalars_synthetic, the expected value from loop_reference on a context of its own"""
    id = "V8c"
    n_circ, n_dotp, L = 8, 0, 17
    device_reference = True
    seed = 0x5BA27A2B4E254 + 1850

    def __init__(self):
        self.pool_sizes = (1 << 17, 1 << 16)

    def _inputs(self, ctx):
        import torch
        N = 1 << self.L
        x = torch.empty((self.n_circ * N, 8), dtype=torch.int32, device="cuda")
        mem = x.data_ptr()
        ctx.scalars_synthetic(self.seed, 0, self.n_circ * N, mem)
        ctx.sync()
        ins = [ctx.table_from_dev(mem + 32 * N * i, N) for i in range(self.n_circ)]
        del x
        return ins

    def compute(self):
        raise RuntimeError("V8c: set the expected value with loop_reference() first")

    def loop_reference(self, ctx):
        """ProductCircuitEvalProofBatched::prove written with sbn_sumcheck_begin_eq + sbn_sumcheck_round and the host transcript, as
        test_gpu_product_proof.py builds it (there with sbn_sumcheck_prove inside)"""
        import spartan_bn254_amd as sbn
        ins = self._inputs(ctx)
        pcs = ctx.product_circuit_many(ins)
        layers = [[ins[i]] + pcs[i][:-1] for i in range(self.n_circ)]
        n, L = self.n_circ, self.L
        tr = sbn.Transcript(self.label)
        try:
            tops = [ctx.table_halves(layers[i][L - 1]) for i in range(n)]
            ctv = [a * b % R for a, b in zip(_ints(b"".join(ctx.table_read0_many([t[0] for t in tops]))), _ints(b"".join(ctx.table_read0_many([t[1] for t in tops]))))]
            for t in tops:
                t[0].free(); t[1].free()
            rand, polys, claims = [], b"", b""
            for layer in range(L - 1, -1, -1):
                halves = [ctx.table_halves(layers[i][layer]) for i in range(n)]
                A, B = [h[0] for h in halves], [h[1] for h in halves]
                coeffs = [tr.challenge_scalar(b"rand_coeffs_next_layer") for _ in ctv]
                e = sum(a * _int(c) for a, c in zip(ctv, coeffs)) % R
                if len(A[0]) == 1:
                    fin = ctx.table_read0_many(A) + ctx.table_read0_many(B)
                    rs = []
                else:
                    st, ev = ctx.sumcheck_begin_eq(A, B, fr_bytes(rand), [], [], [], b"".join(coeffs))
                    rs = []
                    for _ in range(len(rand)):
                        e0, e2, e3 = (_int(ev[32 * k:32 * k + 32]) for k in range(3))
                        cj = sbn.unipoly_from_evals(fr_bytes([e0, (e - e0) % R, e2, e3]))
                        tr.append_message(b"poly", b"UniPoly_begin")
                        for k in range(4):
                            tr.append_scalar(b"coeff", cj[32 * k:32 * k + 32])
                        tr.append_message(b"poly", b"UniPoly_end")
                        rj = tr.challenge_scalar(b"challenge_nextround")
                        e = _int(sbn.unipoly_eval(cj, rj))
                        polys += cj; rs.append(_int(rj))
                        ev = st.round(rj)
                    fin = st.finish()
                    st.free()
                lefts, rights = fin[:n], fin[n:2 * n]
                for a, b in zip(lefts, rights):
                    tr.append_message(b"claim_prod_left", a); tr.append_message(b"claim_prod_right", b)
                claims += b"".join(lefts) + b"".join(rights)
                r_layer = _int(tr.challenge_scalar(b"challenge_r_layer"))
                ctv = [(a + r_layer * (b - a)) % R for a, b in zip(_ints(b"".join(lefts)), _ints(b"".join(rights)))]
                rand = [r_layer] + rs
                for h in halves:
                    h[0].free(); h[1].free()
            self._expected = (polys, claims, fr_bytes(rand), fr_bytes(ctv), tr.state())
        finally:
            tr.free()
            for t in ins + [t for pc in pcs for t in pc]:
                t.free()
        return self._expected

    def run(self, ctx, mp):
        return self._prove(ctx, self._inputs(ctx), [])

    def p1(self, ctx, mp):
        N = 1 << (self.L + 1)
        top = top_table(N)
        self._prove(ctx, [ctx.table_upload(top) for _ in range(12)], [])
        stock_pool(ctx, self.pool_sizes)


# ---- V9, V9j: the Hyrax opening -----------------------------------------------------------------------------------------------------

class V9(Victim):
    """sbn_polyeval_prove, ell = 8 with blinds (16 x 16), over a generator set made for the call"""
    id = "V9"
    ell = 8
    p1_ell = 10
    LABEL = b"gens_ctx_state_polyeval"

    def __init__(self):
        rng = random.Random(1900 + self.ell)
        self.ml, self.mr = pem.factored_lens(self.ell)
        self.pool_sizes = (1 << self.ell, 1 << self.mr, 1 << self.ml)
        self.Z = [rng.randrange(R) for _ in range(1 << self.ell)]
        self.Z[3] = R - 1; self.Z[4] = 0
        self.r = [rng.randrange(R) for _ in range(self.ell)]
        self.blinds = [rng.randrange(R) for _ in range(1 << self.ml)]
        self.blind_Zr = rng.randrange(R)
        self.rnd = [rng.randrange(R) for _ in range(3 + 2 * self.mr)]
        self.Zr = pem.dot(self.Z, pem.eq_evals(self.r))

    def _gens_host(self, n):
        return pem.split_gens(ol.gens_new(n + 1, self.LABEL)[0], n)

    def compute(self):
        m = tm.Transcript(b"ctx state polyeval")
        want, Cy, Cx = pem.prove(m, self._gens_host(1 << self.mr), self.Z, self.blinds, self.r, self.Zr, self.blind_Zr, self.rnd)
        return pem.proof_bytes(want), Cx, Cy, m.state()

    def _open(self, ctx, n, Zb, r, Zr, rnd, blinds, blind_Zr, gens_n=None):
        import spartan_bn254_amd as sbn_mod
        bases, _ = ctx.gens_new((n if gens_n is None else gens_n) + 1, self.LABEL, want_points=False)
        t = ctx.table_upload(Zb)
        tr = sbn_mod.Transcript(b"ctx state polyeval")
        try:
            proof, Cx, Cy = ctx.polyeval_prove(bases, t, r, Zr, rnd, tr, blinds=blinds, blind_Zr=blind_Zr)
            return proof, Cx, Cy, tr.state()
        finally:
            tr.free(); t.free(); bases.free()

    def _args(self):
        return fr_bytes(self.Z), fr_bytes(self.r), pem.sb(self.Zr), fr_bytes(self.rnd), fr_bytes(self.blinds), pem.sb(self.blind_Zr)

    def run(self, ctx, mp):
        return self._open(ctx, 1 << self.mr, *self._args())

    def check_path(self, ran):
        assert launches(ran, "k_polyeval_front") == 1 and launches(ran, "k_polyeval_close") == 1 and launches(ran, "k_bullet_prep") == self.mr, ran

    def p1(self, ctx, mp):
        ml, mr = pem.factored_lens(self.p1_ell)
        self._open(ctx, 1 << mr, top_table(1 << self.p1_ell), TOP * self.p1_ell, TOP, TOP * (3 + 2 * mr), TOP * (1 << ml), TOP)
        stock_pool(ctx, self.pool_sizes)

    def p2(self, ctx, mp, E):
        Zb, r, Zr, rnd, blinds, blind_Zr = self._args()
        with pytest.raises(E):
            self._open(ctx, 1 << self.mr, Zb, r, Zr, rnd[:-32] + BAD, blinds, blind_Zr)          # a bad rnd entry
        with pytest.raises(E):
            self._open(ctx, 1 << self.mr, Zb, r, Zr, rnd, blinds, blind_Zr, gens_n=(1 << self.mr) - 1)   # one generator too few


class V9j(Victim):
    """sbn_joint_opening_prove: 8 polynomials of 2^3 entries reduced to one opening (ell = 6)"""
    id = "V9j"
    count, ell_r = 8, 3
    LABEL = V9.LABEL
    labels = (b"evals_ops_val", b"challenge_combine_n_to_one", b"joint_claim_eval")

    def __init__(self):
        rng = random.Random(1950)
        self.ell = (self.count.bit_length() - 1) + self.ell_r
        self.n = 1 << pem.factored_lens(self.ell)[1]
        self.pool_sizes = (1 << self.ell, self.n)
        polys = [[rng.randrange(R) for _ in range(1 << self.ell_r)] for _ in range(self.count)]
        polys[2][1] = R - 1
        self.r = [rng.randrange(R) for _ in range(self.ell_r)]
        self.evals = [pem.dot(p, pem.eq_evals(self.r)) for p in polys]
        self.Z = [x for p in polys for x in p]
        self.rnd = [rng.randrange(R) for _ in range(3 + 2 * (self.n.bit_length() - 1))]

    def compute(self):
        m = tm.Transcript(b"ctx state joint")
        gens = pem.split_gens(ol.gens_new(self.n + 1, self.LABEL)[0], self.n)
        ch, claim, want, Cy, Cx = pem.prove_single(m, gens, self.Z, self.r, self.evals, self.rnd, self.labels)
        return fr_bytes(ch), pem.sb(claim), pem.proof_bytes(want), Cx, Cy, m.state()

    def _open(self, ctx, gens_n, Zb, evals, r, rnd):
        import spartan_bn254_amd as sbn_mod
        bases, _ = ctx.gens_new(gens_n + 1, self.LABEL, want_points=False)
        t = ctx.table_upload(Zb)
        tr = sbn_mod.Transcript(b"ctx state joint")
        try:
            return ctx.joint_opening_prove(bases, t, evals, self.labels, r, rnd, tr) + (tr.state(),)
        finally:
            tr.free(); t.free(); bases.free()

    def run(self, ctx, mp):
        return self._open(ctx, self.n, fr_bytes(self.Z), fr_bytes(self.evals), fr_bytes(self.r), fr_bytes(self.rnd))

    def check_path(self, ran):
        assert launches(ran, "k_polyeval_front") == 1 and launches(ran, "k_polyeval_close") == 1 and launches(ran, "k_bullet_prep") == self.n.bit_length() - 1, ran

    def p1(self, ctx, mp):
        count = 32
        ell = 5 + self.ell_r
        n = 1 << pem.factored_lens(ell)[1]
        self._open(ctx, n, top_table(1 << ell), TOP * count, TOP * self.ell_r, TOP * (3 + 2 * (n.bit_length() - 1)))
        stock_pool(ctx, self.pool_sizes)

    def p2(self, ctx, mp, E):
        with pytest.raises(E):
            self._open(ctx, self.n - 1, fr_bytes(self.Z), fr_bytes(self.evals), fr_bytes(self.r), fr_bytes(self.rnd))     # one generator too few
        with pytest.raises(E):
            self._open(ctx, self.n, fr_bytes(self.Z), fr_bytes(self.evals), fr_bytes(self.r), fr_bytes(self.rnd[:-1]) + BAD)


# ---- V10: KZG -----------------------------------------------------------------------------------------------------------------------

class V10(Victim):
    """sbn_poly_div_linear and sbn_kzg_open at n = 1025 (one tile + 1), sbn_kzg_open_batched with lens [5, 1000, 64], an SRS of 2049 powers from tau.
    1025 coefficients leave a quotient of exactly 2^10 entries and no padding, so a polynomial of 2050 coefficients is divided too: its quotient table
    has 4096 entries, the three tiles of the division write 3072 of them, and the call has to fill the last 1024 with zeros"""
    id = "V10"
    tau = 0x1234567890abcdef1234567890abcdef
    srs_n, n = 2049, 1025
    lens = [5, 1000, 64]
    n_pad = 2050

    def __init__(self):
        self.pool_sizes = (2048, 1024, 8, 64, 4096)
        self.padded = km.from_bytes(rand_scalars(self.n_pad, 2003))
        self.vals = km.from_bytes(rand_scalars(self.n, 2000)); self.vals[7] = R - 1
        self.polys = [km.from_bytes(rand_scalars(m, 2010 + i)) for i, m in enumerate(self.lens)]
        rng = random.Random(2001)
        self.z, self.gamma = rng.randrange(R), rng.randrange(R)

    @staticmethod
    def _padded(vals, seed):
        """vals in a table of the next power of two, the entries past len(vals) non-zero junk"""
        L = 1 << max(0, (len(vals) - 1).bit_length())
        junk = [j or 1 for j in km.from_bytes(rand_scalars(L - len(vals), seed))] if L > len(vals) else []
        return km.to_bytes(list(vals) + junk)

    def compute(self):
        pw, x = [], 1
        for _ in range(self.srs_n):
            pw.append(x); x = x * self.tau % R
        pts = ol.g1_mul_gen_batch(km.to_bytes(pw), 8)
        y = km.evaluate_poly(self.vals, self.z)
        q = km.compute_quotient(self.vals, self.z, y)
        pi = ol.msm_pippenger(km.to_bytes(q), pts[:64 * len(q)], 8)
        evs, _, qb = km.batch_prove(self.polys, self.z, self.gamma)
        pib = ol.msm_pippenger(km.to_bytes(qb), pts[:64 * len(qb)], 8)
        y2 = km.evaluate_poly(self.padded, self.z)
        q2 = km.compute_quotient(self.padded, self.z, y2)
        return (km.to_bytes([y]), km.to_bytes(q + [0] * (1024 - len(q))), (km.to_bytes([y]), pi, False), ([km.to_bytes([e]) for e in evs], pib, False),
                km.to_bytes([y2]), km.to_bytes(q2 + [0] * (4096 - len(q2))))

    def _all(self, ctx, srs_n, tab_bytes, n, batch_bytes, lens, z, gamma, pad_bytes, n_pad):
        srs = ctx.kzg_srs_from_tau(km.to_bytes([self.tau]), srs_n)
        t = ctx.table_upload(tab_bytes)
        tabs = [ctx.table_upload(b) for b in batch_bytes]
        tp = ctx.table_upload(pad_bytes)
        qs = []
        try:
            ev, q = ctx.poly_div_linear(t, n, z); qs.append(q)
            qb = ctx.table_download(q)
            opened, batched = ctx.kzg_open(srs, t, n, z), ctx.kzg_open_batched(srs, tabs, lens, z, gamma)
            ev2, q2 = ctx.poly_div_linear(tp, n_pad, z); qs.append(q2)          # a quotient table longer than the division's tiles: the tail is the call's zero fill
            return ev, qb, opened, batched, ev2, ctx.table_download(q2)
        finally:
            for x in tabs + [t, tp] + [q for q in qs if q is not None]:
                x.free()
            srs.free()

    def run(self, ctx, mp):
        return self._all(ctx, self.srs_n, self._padded(self.vals, 2002), self.n, [self._padded(p, 2020 + i) for i, p in enumerate(self.polys)],
                         self.lens, km.to_bytes([self.z]), km.to_bytes([self.gamma]), self._padded(self.padded, 2004), self.n_pad)

    def check_path(self, ran):
        assert launches(ran, "k_kzg_div_tiles") >= 3 and launches(ran, "k_kzg_combine") == 1, ran      # the multi-tile divisions (1025 twice, 2050) and the batched opening

    def p1(self, ctx, mp):
        self._all(ctx, 8193, top_table(8192), 4097, [top_table(32), top_table(4096), top_table(256)], [20, 4000, 256], TOP, TOP, top_table(16384), 8194)
        stock_pool(ctx, self.pool_sizes)

    def p2(self, ctx, mp, E):
        """KZG reads no caller scalars but z and gamma (the polynomials are tables): the non-canonical scalar is z / gamma, after a good commit on the same
        handles; and an opening whose quotient does not fit the SRS"""
        srs = ctx.kzg_srs_from_tau(km.to_bytes([self.tau]), 100)
        t = ctx.table_upload(rand_scalars(256, 5))
        try:
            ctx.kzg_commit(srs, t, 100)
            with pytest.raises(E):
                ctx.kzg_open(srs, t, 50, BAD)
            with pytest.raises(E):
                ctx.poly_div_linear(t, 50, BAD)
            with pytest.raises(E):
                ctx.kzg_open_batched(srs, [t], [16], km.to_bytes([3]), BAD)
            with pytest.raises(E):
                ctx.kzg_open(srs, t, 102, km.to_bytes([5]))
        finally:
            t.free(); srs.free()


# ---- V11, V12: the R1CS matrices and their dense representation -------------------------------------------------------------------

class V11(Victim):
    """sbn_r1cs_multiply, sbn_r1cs_eval_table and sbn_r1cs_evaluate at (num_cons, num_vars) = (2^10, 2^9) of test_gpu_r1cs.py"""
    id = "V11"
    nc, nv = 1 << 10, 1 << 9

    def __init__(self):
        self.pool_sizes = (self.nc, 2 * self.nv)
        self.mats = r1cs_instance(self.nc, self.nv, 2100)
        self.z = rm.from_bytes(rand_scalars(2 * self.nv, 2101))
        lx, ly = self.nc.bit_length() - 1, (2 * self.nv).bit_length() - 1
        self.rx = rm.from_bytes(rand_scalars(lx, 2102)); self.ry = rm.from_bytes(rand_scalars(ly, 2103))
        self.rabc = rm.from_bytes(rand_scalars(3, 2104))

    def compute(self):
        return (tuple(rm.multiply_vec(self.nc, self.nv, self.mats, self.z)), rm.eval_table(self.nc, self.nv, self.mats, self.rx, *self.rabc),
                tuple(rm.evaluate(self.nc, self.nv, self.mats, self.rx, self.ry)))

    @staticmethod
    def _upload(ctx, nc, nv, mats):
        return ctx.r1cs_upload(nc, nv, [(np.array(r, np.uint32), np.array(c, np.uint32), rm.to_bytes(v)) for r, c, v in mats])

    def _all(self, ctx, nc, nv, mats, zb, rx, ry, rabc):
        h = self._upload(ctx, nc, nv, mats)
        tz = ctx.table_upload(zb)
        made = []
        try:
            made += ctx.r1cs_multiply(h, tz)
            made.append(ctx.r1cs_eval_table(h, rx, *rabc))
            return (tuple(rm.from_bytes(ctx.table_download(t)) for t in made[:3]), rm.from_bytes(ctx.table_download(made[3])),
                    tuple(rm.from_bytes(b"".join(ctx.r1cs_evaluate(h, rx, ry)))))
        finally:
            for t in made + [tz]:
                t.free()
            h.free()

    def run(self, ctx, mp):
        return self._all(ctx, self.nc, self.nv, self.mats, rm.to_bytes(self.z), rm.to_bytes(self.rx), rm.to_bytes(self.ry), [rm.to_bytes([v]) for v in self.rabc])

    def check_path(self, ran):
        assert launches(ran, "k_r1cs_spmv") >= 1 and launches(ran, "k_r1cs_spmv_eval") == 1 and launches(ran, "k_r1cs_scale3") == 1, ran

    def p1(self, ctx, mp):
        nc, nv = 4 * self.nc, 4 * self.nv
        mats = [(r, c, [R - 1] * len(v)) for r, c, v in r1cs_instance(nc, nv, 2110)]
        self._all(ctx, nc, nv, mats, top_table(2 * nv), TOP * (nc.bit_length() - 1), TOP * ((2 * nv).bit_length() - 1), [TOP] * 3)
        stock_pool(ctx, self.pool_sizes)

    def p2(self, ctx, mp, E):
        """the argument errors of test_r1cs_errors_leave_context_usable"""
        nc, nv = 1 << 4, 1 << 3
        good = r1cs_instance(nc, nv, 3)
        with pytest.raises(E):
            self._upload(ctx, nc, nv, [(good[0][0] + [nc], good[0][1] + [0], good[0][2] + [1])] + good[1:])
        rows, cols, vals = good[1]
        with pytest.raises(E):
            ctx.r1cs_upload(nc, nv, [([], [], b""), (np.array(rows + [0], np.uint32), np.array(cols + [0], np.uint32), rm.to_bytes(vals) + BAD), ([], [], b"")])
        h = self._upload(ctx, nc, nv, good)
        tz = ctx.table_upload(rand_scalars(nv, 4))
        try:
            with pytest.raises(E):
                ctx.r1cs_multiply(h, tz)
            with pytest.raises(E):
                ctx.r1cs_eval_table(h, rand_scalars(4, 1), BAD, TOP, TOP)
            with pytest.raises(E):
                ctx.r1cs_evaluate(h, rand_scalars(5, 1), rand_scalars(4, 2))
        finally:
            tz.free(); h.free()


class V12(Victim):
    """sbn_dense_build at the shape b3_x_lt_y of test_gpu_dense.py (three matrices, 300 / 1 / 513 entries, 2^9 cells): every u32 array, comb_ops, comb_mem"""
    id = "V12"
    shape = next(sh for sh in DENSE_SHAPES if sh[0] == "b3_x_lt_y")
    p1_shape = ("p1", 10, 12, [(9000, "uniform"), (4096, "uniform"), (4097, "uniform")])

    def __init__(self):
        _, self.nx, self.ny, _ = self.shape
        self.mats = dense_instance(self.shape, 2200)

    def compute(self):
        d = dm.Dense(self.nx, self.ny, self.mats)
        u32 = []
        for side in (0, 1):
            for k in range(d.batch):
                u32 += [list(d.addr[side][k]), list(d.read_ts[side][k])]
            u32.append(list(d.audit_ts[side]))
        return (d.N, d.cells, d.batch), u32, rm.to_bytes(d.comb_ops), rm.to_bytes(d.comb_mem)

    @staticmethod
    def _build(ctx, nx, ny, mats):
        return ctx.dense_build(nx, ny, [(np.array(r, np.uint32), np.array(c, np.uint32), rm.to_bytes(v)) for r, c, v in mats])

    def _all(self, ctx, nx, ny, mats):
        h = self._build(ctx, nx, ny, mats)
        try:
            get = lambda p, n: np.frombuffer(ctx.dev_download(p, 4 * n), np.uint32).tolist()
            u32 = []
            for side in (0, 1):
                for k in range(h.batch):
                    u32 += [get(h.addr_dev(side, k), h.num_ops), get(h.read_ts_dev(side, k), h.num_ops)]
                u32.append(get(h.audit_ts_dev(side), h.num_cells))
            return (h.num_ops, h.num_cells, h.batch), u32, ctx.table_download(h.comb_ops), ctx.table_download(h.comb_mem)
        finally:
            h.free()

    def run(self, ctx, mp):
        return self._all(ctx, self.nx, self.ny, self.mats)

    def check_path(self, ran):
        assert launches(ran, "k_dense_tables") == 1 and launches(ran, "k_dense_scatter") >= 1, ran

    def p1(self, ctx, mp):
        _, nx, ny, _ = self.p1_shape
        mats = [(r, c, [R - 1] * len(v)) for r, c, v in dense_instance(self.p1_shape, 2210)]
        self._all(ctx, nx, ny, mats)
        stock_pool(ctx, (16 * 1024, 2 * 512))            # the victim's comb_ops and comb_mem

    def p2(self, ctx, mp, E):
        """the argument errors of test_dense_errors_leave_context_usable"""
        nx, ny, cells = 3, 4, 16
        good = dense_instance(("e", nx, ny, [(20, "uniform"), (9, "uniform")]), 3)
        r, c, v = good[1]
        with pytest.raises(E, match="row 16 >= num_cells 16"):
            self._build(ctx, nx, ny, [good[0], (r + [cells], c + [0], v + [1])])
        with pytest.raises(E, match="value >= r"):
            ctx.dense_build(nx, ny, [(np.array(good[0][0], np.uint32), np.array(good[0][1], np.uint32), rm.to_bytes(good[0][2])),
                                     (np.array(r + [0], np.uint32), np.array(c + [0], np.uint32), rm.to_bytes(v) + BAD)])
        with pytest.raises(E, match="batch=0"):
            ctx.dense_build(nx, ny, [])


# ---- V13: the table calls -----------------------------------------------------------------------------------------------------------

class V13(Victim):
    """sbn_gather_merge (3 x 2^7 addresses: 384 entries padded to 512), sbn_hash_layer_pair, sbn_table_bound, sbn_table_evaluate_many (5 tables) and
    sbn_eq_evals(13), every result downloaded"""
    id = "V13"
    count, n, cells = 3, 1 << 7, 1 << 7

    def __init__(self):
        self.pool_sizes = (512, 128, 1024, 32, 64, 1 << 13)
        rng = np.random.default_rng(2300)
        self.mem = [with_edges(rand_scalars(self.cells, 2301 + k)) for k in range(self.count)]
        self.addr = [rng.integers(0, self.cells, size=self.n, dtype=np.uint32) for _ in range(self.count)]
        self.ts = rng.integers(0, 50, size=self.n, dtype=np.uint32)
        self.g, self.tau = rand_scalars(1, 2305), rand_scalars(1, 2306)
        self.Zb, self.Lv = rand_scalars(32 * 32, 2307), rand_scalars(32, 2308)
        self.ev_tabs = [rand_scalars(64, 2310 + i) for i in range(5)]
        self.ev_r = rand_scalars(6, 2320)
        self.eq_r = rand_scalars(13, 2321)

    def compute(self):
        gm = b"".join(b"".join(self.mem[k][32 * int(i):32 * int(i) + 32] for i in self.addr[k]) for k in range(self.count))
        gm += bytes(32 * (512 - self.count * self.n))
        deref0 = gm[:32 * self.n]
        chi = ol.eq_evals(self.ev_r)
        return (gm, ol.hash_layer(self.addr[0], deref0, self.ts, 0, self.g, self.tau), ol.hash_layer(self.addr[0], deref0, self.ts, 1, self.g, self.tau),
                ol.bound(self.Zb, self.Lv, 32, 32), b"".join(ol.fr_dot(x, chi) for x in self.ev_tabs), ol.eq_evals(self.eq_r))

    def _all(self, ctx, mems, addrs, n, ts, Zb, Lv, Ls, ev_tabs, ev_r, eq_r):
        keep, live = [], []
        try:
            mt = [ctx.table_upload(m) for m in mems]; live += mt
            ap = [dev_u32(ctx, a, keep) for a in addrs]
            tp = dev_u32(ctx, ts, keep)
            gm = ctx.gather_merge(mt, ap, n); live.append(gm)
            v0 = ctx.table_slice(gm, 0, n); live.append(v0)
            rd, wr = ctx.hash_layer_pair(ap[0], v0, tp, 0, tp, 1, self.g, self.tau); live += [rd, wr]
            tZ, tL = ctx.table_upload(Zb), ctx.table_upload(Lv); live += [tZ, tL]
            bd = ctx.table_bound(tZ, tL); live.append(bd)
            assert len(bd) == len(Zb) // 32 // Ls
            et = [ctx.table_upload(x) for x in ev_tabs]; live += et
            evs = ctx.table_evaluate_many(et, ev_r)
            eq = ctx.eq_evals(eq_r); live.append(eq)
            return ctx.table_download(gm), ctx.table_download(rd), ctx.table_download(wr), ctx.table_download(bd), evs, ctx.table_download(eq)
        finally:
            for t in reversed(live):
                t.free()
            for p in keep:
                ctx.dev_free(p)

    def run(self, ctx, mp):
        out = self._all(ctx, self.mem, self.addr, self.n, self.ts, self.Zb, self.Lv, 32, self.ev_tabs, self.ev_r, self.eq_r)
        assert len(out[0]) == 32 * 512
        return out

    def check_path(self, ran):
        assert launches(ran, "k_gather_merge") == 1 and launches(ran, "k_hash_layer") == 1 and launches(ran, "k_bound_fold") == 1, ran

    def p1(self, ctx, mp):
        n, cells = 4 * self.n, 4 * self.cells
        rng = np.random.default_rng(2350)
        self._all(ctx, [top_table(cells)] * 6, [rng.integers(0, cells, size=n, dtype=np.uint32) for _ in range(6)], n, np.full(n, 0xffffffff, np.uint32),
                  top_table(64 * 64), top_table(64), 64, [top_table(256)] * 10, TOP * 8, TOP * 15)
        stock_pool(ctx, self.pool_sizes)

    def p2(self, ctx, mp, E):
        keep = []
        mt = ctx.table_upload(self.mem[0])
        try:
            bad = self.addr[0].copy(); bad[self.n // 2] = self.cells              # one address past the table, in the middle
            with pytest.raises(E):
                ctx.gather_merge([mt], [dev_u32(ctx, bad, keep)], self.n)
        finally:
            mt.free()
            for p in keep:
                ctx.dev_free(p)


_CATALOGUE = None


def catalogue():
    """every victim, built once per process (the inputs are fixed; the expected values are computed on first use)"""
    global _CATALOGUE
    if _CATALOGUE is None:
        _CATALOGUE = [cls() for cls in (V1, V2, V3, V4, V4c, V5, V6, V7, V8, V8c, V9, V9j, V10, V11, V12, V13)]
    return _CATALOGUE


def by_id(vid):
    return next(v for v in catalogue() if v.id == vid)


def default_victims():
    """the victims that share the default context settings (V2 and V3 need contexts of their own)"""
    return [v for v in catalogue() if v.settings == "default"]


CONTEXT_ENV = {"default": {}, "sort2": {"SBN_SORT2_MIN": "1024"}, "glv": {"SBN_MSM_GLV": "1", "SBN_SORT2_MIN": "1024"}}


def make_context(sbn, mp, settings="default", extra=None):
    """a fresh context whose creation-time settings are `settings` (set with monkeypatch around sbn_ctx_create, as test_gpu_glv.py::_ctx does)"""
    env = dict(CONTEXT_ENV[settings]); env.update(extra or {})
    for k in ("SBN_MSM_GLV", "SBN_SORT2_MIN", "SBN_MSM_C", "SBN_COMMIT_CHUNK_BYTES"):
        mp.delenv(k, raising=False)
    for k, v in env.items():
        mp.setenv(k, v)
    try:
        return sbn.Context(0)
    finally:
        for k in env:
            mp.delenv(k)
