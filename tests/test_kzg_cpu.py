"""CPU: the KZG entry points are declared and bound, and the pure-int model of the reference's opening arithmetic (kzg_model.py)
satisfies q(x)(x - z) + p(z) = p(x) — the relation the device division is checked against on the GPU (test_gpu_kzg.py)."""
import os
import random
import re

import pytest

from conftest import ROOT
import kzg_model as km

ENTRY_POINTS = ["sbn_kzg_srs_upload", "sbn_kzg_srs_from_tau", "sbn_kzg_commit", "sbn_poly_div_linear", "sbn_kzg_open", "sbn_kzg_open_batched"]
METHODS = ["kzg_srs_upload", "kzg_srs_from_tau", "kzg_commit", "poly_div_linear", "kzg_open", "kzg_open_batched"]


def test_header_declares_kzg_entry_points():
    src = open(os.path.join(ROOT, "include", "sbn254.h")).read()
    for name in ENTRY_POINTS:
        assert re.search(r"\bint\s+" + name + r"\s*\(", src), name


def test_binding_exposes_kzg_entry_points(sbn):
    for name in ENTRY_POINTS:
        assert name in sbn.EXPORTED_SYMBOLS, name
    for m in METHODS:
        assert callable(getattr(sbn.Context, m, None)), m


def _check_division(p, z, x):
    y = km.evaluate_poly(p, z)
    q = km.compute_quotient(p, z, y)
    assert len(q) == max(len(p) - 1, 0)
    assert (km.evaluate_poly(q, x) * (x - z) + y - km.evaluate_poly(p, x)) % km.R == 0


@pytest.mark.parametrize("n", [0, 1, 2, 3, 5, 17, 64, 100, 1025])
def test_model_division_identity(n):
    rng = random.Random(n)
    for z in (0, 1, km.R - 1, rng.randrange(km.R)):
        p = [rng.randrange(km.R) for _ in range(n)]
        _check_division(p, z, rng.randrange(km.R))
        _check_division([km.R - 1] * n, z, rng.randrange(km.R))


def test_model_empty_and_constant():
    assert km.evaluate_poly([], 5) == 0 and km.compute_quotient([], 5, 0) == []
    assert km.evaluate_poly([7], 5) == 7 and km.compute_quotient([7], 5, 7) == []


@pytest.mark.parametrize("lens", [[1], [3, 1, 4], [0, 5], [64, 63, 65, 2, 1, 0, 7]])
def test_model_batch_identity(lens):
    rng = random.Random(sum(lens) + len(lens))
    polys = [[rng.randrange(km.R) for _ in range(n)] for n in lens]
    for gamma in (0, 1, rng.randrange(km.R)):
        z, x = rng.randrange(km.R), rng.randrange(km.R)
        evals, y, q = km.batch_prove(polys, z, gamma)
        assert evals == [km.evaluate_poly(p, z) for p in polys]
        comb = km.combine(polys, gamma)
        assert y == km.evaluate_poly(comb, z)
        assert (km.evaluate_poly(q, x) * (x - z) + y - km.evaluate_poly(comb, x)) % km.R == 0
