"""GPU: what a failed call leaves behind ("table lifetime").  The failures here are the ones the library reports as SBN_EINVAL after it
has already made device tables: sbn_gather_merge behind its gather, the two sparse evaluation proofs behind the hashed sets and every product
layer.  After each, on the same context, the same call with good inputs must return the bytes a fresh context returns, and a table the test made
before the failure must still hold its contents: nothing the failed call released was still in use, or was released twice.  Every comparison is
bit-exact."""
import random

import numpy as np
import pytest

import r1cs_model as rm
import sparse_eval_loop as loop
import sparse_eval_model as sem
from sparse_eval_model import R

pytestmark = pytest.mark.gpu
LABEL = b"gens_table_lifetime"
TR_LABEL = b"table lifetime gpu"
TAU = random.Random(1366).randrange(1, R)


def _u32_dev(c, arr):
    p = c.dev_alloc(4 * len(arr))
    c.dev_upload(p, np.ascontiguousarray(arr, dtype=np.uint32).tobytes())
    return p


def _on_a_fresh_context(sbn, run):
    c = sbn.Context(0)
    try:
        return run(c)
    finally:
        c.close()


def test_gather_merge_with_an_address_outside_its_memory(ctx, sbn):
    """2 memories of 8 cells, 16 addresses each; address 5 of the second memory is 8"""
    rng = np.random.default_rng(1)
    mems_b = [rm.random_vals(rng, 8).tobytes() for _ in range(2)]
    addr = [rng.integers(0, 8, 16, dtype=np.uint32) for _ in range(2)]
    bad = addr[1].copy(); bad[5] = 8

    def gather(c, second):
        mems = [c.table_upload(b) for b in mems_b]
        ptrs = [_u32_dev(c, addr[0]), _u32_dev(c, second)]
        try:
            t = c.gather_merge(mems, ptrs, 16)
            try:
                return c.table_download(t)
            finally:
                t.free()
        finally:
            for t in mems:
                t.free()
            for p in ptrs:
                c.dev_free(p)
    want = _on_a_fresh_context(sbn, lambda c: gather(c, addr[1]))
    assert len(want) == 32 * 32
    canary_b = rm.random_vals(rng, 32).tobytes()                # the size of the table the failed call makes and gives back
    canary = ctx.table_upload(canary_b)
    try:
        with pytest.raises(sbn.SbnError, match="rc=-1.*1 addresses are outside their memory table"):
            gather(ctx, bad)
        assert gather(ctx, addr[1]) == want
        assert ctx.table_download(canary) == canary_b
    finally:
        canary.free()


@pytest.mark.parametrize("build", ["hyrax", "kzg"])
@pytest.mark.parametrize("batch", [1, 3])
def test_sparse_eval_with_a_wrong_evaluation(ctx, sbn, build, batch):
    """evals[0] off by one: refused at sparse_mlpoly_full.rs:1366, behind the two eq tables, the derefs table, 4 batch + 4 hashed sets and all their
    product layers.  batch = 1 and 3: one and several circuits per side"""
    nx = ny = 3
    N = 16
    shape = sem.Shape(nx, ny, N, batch)
    kinds = ("ops", "mem", "derefs") if build == "hyrax" else ("ops", "mem")
    rng = np.random.default_rng(10 * batch + len(build))
    mats = loop.random_mats(nx, ny, N, batch, 7 + batch)
    rx, ry = rm.random_vals(rng, nx).tobytes(), rm.random_vals(rng, ny).tobytes()
    n_rnd = (sbn.sparse_eval_sizes if build == "hyrax" else sbn.sparse_eval_kzg_sizes)(nx, ny, N, batch)[0]
    rnd = rm.random_vals(rng, n_rnd).tobytes()

    class Setup:
        def __init__(self, c):
            self.c = c
            self.dense = c.dense_build(nx, ny, mats)
            self.gens = [c.gens_new(shape.R(k) + 1, LABEL + b"_" + k.encode(), want_points=False)[0] for k in kinds]
            if build == "kzg":
                self.gens += [c.kzg_srs_from_tau(sem.pm.sb(TAU), (1 << shape.ell["derefs"]) + 1), None]        # no derefs key

        def prove(self, evals):
            tr = sbn.Transcript(TR_LABEL)
            call = self.c.sparse_eval_prove if build == "hyrax" else self.c.sparse_eval_prove_kzg
            return call(self.dense, rx, ry, evals, *self.gens, rnd, tr), tr.state()

        def free(self):
            for h in [self.dense] + self.gens:
                if h is not None:
                    h.free()

    def reference(c, evals):
        s = Setup(c)
        try:
            return s.prove(evals)
        finally:
            s.free()
    canary_b = rm.random_vals(rng, N // 2).tobytes()            # the size of a first product layer
    canary = ctx.table_upload(canary_b)
    s = Setup(ctx)
    try:
        evals = loop.evals_of(sbn, ctx, s.dense, rx, ry)
        want = _on_a_fresh_context(sbn, lambda c: reference(c, evals))
        wrong = sem.pm.sb(int.from_bytes(evals[:32], "little") + 1) + evals[32:]
        with pytest.raises(sbn.SbnError, match=r"rc=-1.*!= evals\[0\].*sparse_mlpoly_full.rs:1366"):
            s.prove(wrong)
        assert s.prove(evals) == want
        assert ctx.table_download(canary) == canary_b
    finally:
        s.free()
        canary.free()


# the layers up to 2048 entries come from one launch (the tail), those above from one streaming launch each: 2 and 4 entries are the tail alone with
# one and two layers, 4096 the streaming launch and the tail behind it
@pytest.mark.parametrize("n", [2, 4, 4096])
def test_product_circuit_many_hands_out_every_layer(ctx, sbn, n):
    """4 tables: every layer handle comes back non-null with its length, and freeing them all and repeating gives the same bytes.  That a failed call
    leaves every entry of the caller's array null is not run here (it takes a failed launch or allocation): the call fills the array at its
    successful end only, which is read off product_circuit_many_locked, not tested"""
    rng = np.random.default_rng(n)
    ins = [ctx.table_upload(rm.random_vals(rng, n).tobytes()) for _ in range(4)]

    def circuits():
        pcs = ctx.product_circuit_many(ins)
        try:
            assert [[t.h.value is not None and len(t) for t in pc] for pc in pcs] == [[n >> (k + 1) for k in range(n.bit_length() - 1)]] * 4
            return [[ctx.table_download(t) for t in pc] for pc in pcs]
        finally:
            for pc in pcs:
                for t in pc:
                    t.free()
    try:
        first = circuits()
        assert circuits() == first
    finally:
        for t in ins:
            t.free()
