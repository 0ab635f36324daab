#!/usr/bin/env python3
"""Writes tests/golden/pairing_kat.json from tests/pairing_model.py: the G2 points, G1 points and GT bytes of the GPU tests' pairing cases
(tests/test_gpu_pairing.py, tests/test_gpu_kzg_verify.py).  Data only; about a minute of pure-Python pairings.

    python tests/golden/make_pairing_golden.py
"""
import json
import os
import random
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import pairing_model as pm  # noqa: E402

TAU = 0x1d2c3b4a59687766554433221100ffeeddccbbaa99887766554433221100f1e2 % pm.R


def main():
    rng = random.Random(20260121)
    g2 = {"gen": pm.G2, "tau": pm.g2_mul(pm.G2, TAU), "tau1": pm.g2_mul(pm.G2, (TAU + 1) % pm.R)}
    for s in (1, 2, 3):
        g2["s%d" % s] = pm.g2_from_seed(s)
    a, b = rng.randrange(1, pm.R), rng.randrange(1, pm.R)
    g2["b_s1"] = pm.g2_mul(g2["s1"], b)
    assert all(pm.g2_in_subgroup(q) for q in g2.values())
    off = [pm.g2_curve_point(s) for s in (11, 12)]                       # on E', outside the r-torsion
    assert all(pm.g2_on_curve(q) and not pm.g2_in_subgroup(q) for q in off)
    pts = [pm.G1] + [pm.g1_mul(pm.G1, rng.randrange(1, pm.R)) for _ in range(4)]
    hx = lambda P: pm.g1_bytes(P).hex()

    def case(name, terms):
        f = pm.pairing_product([(P, g2[q]) for (P, q) in terms])
        return {"name": name, "terms": [[hx(P), q] for (P, q) in terms], "gt": pm.gt_bytes(f).hex(), "is_one": f == pm.F12_ONE}

    aP = pm.g1_mul(pts[1], a)
    cases = [
        case("gen", [(pts[0], "gen")]),
        case("pair1", [(pts[1], "s1")]),
        case("pair2", [(pts[2], "s2")]),
        case("pair3", [(pts[3], "tau")]),
        case("two", [(pts[1], "s1"), (pts[2], "s2")]),
        case("three", [(pts[1], "s1"), (pts[2], "s2"), (pts[3], "s3")]),
        case("four", [(pts[1], "s1"), (pts[2], "s2"), (pts[3], "s3"), (pts[4], "tau")]),
        case("identity_term", [(pts[1], "s1"), (None, "s2"), (pts[3], "s3")]),
        case("only_identity", [(None, "gen")]),
        case("empty", []),
        case("cancel", [(aP, "s1"), (pm.g1_neg(aP), "s1")]),
        case("same_handle_twice", [(pts[1], "s2"), (pts[2], "s2")]),
        case("aP_bQ", [(aP, "b_s1")]),
    ]
    by = {c["name"]: c for c in cases}
    assert by["cancel"]["is_one"] and by["empty"]["is_one"] and by["only_identity"]["is_one"] and not by["gen"]["is_one"]
    assert by["identity_term"]["gt"] == pm.gt_bytes(pm.pairing_product([(pts[1], g2["s1"]), (pts[3], g2["s3"])])).hex()
    e_pq = pm.pairing(pts[1], g2["s1"])
    assert pm.gt_bytes(e_pq).hex() == by["pair1"]["gt"]
    out = {
        "tau": "%064x" % TAU,
        "g2": {k: pm.g2_bytes(v).hex() for k, v in g2.items()},
        "g2_off_subgroup": [pm.g2_bytes(q).hex() for q in off],
        "cases": cases,
        "bilinear": {"a": "%064x" % a, "b": "%064x" % b, "case": "aP_bQ", "gt_pow_ab": pm.gt_bytes(pm.f12_pow(e_pq, a * b % pm.R)).hex()},
    }
    assert out["bilinear"]["gt_pow_ab"] == by["aP_bQ"]["gt"]
    with open(os.path.join(HERE, "pairing_kat.json"), "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
