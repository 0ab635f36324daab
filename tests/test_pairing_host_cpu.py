"""CPU: pairing_host.hpp (the host half of the pairing: G2 parsing, the subgroup test, the NAF schedule, the line tables) against the literal
model of tests/pairing_model.py.  tests/pairing_host_check.cpp includes the header alone and is built with g++ under ASan + UBSan as a
stand-alone program, as tests/test_sparse_verify_host_cpu.py builds its checker.  Also here: the generated constants are what their generator
writes, and the new entry points are exported, bound with the header's arity and refuse a call without a context."""
import ctypes as C
import os
import re
import subprocess
import sys

import pytest

from conftest import ROOT, golden
import pairing_model as pm

KAT = golden("pairing_kat.json")
NEW_SYMBOLS = ["sbn_g2_prepare", "sbn_g2_lines_free", "sbn_pairing_products", "sbn_kzg_verify", "sbn_kzg_verify_batched", "sbn_sparse_eval_verify_kzg"]
OK, NOT_CANONICAL, IDENTITY, OFF_CURVE, NOT_IN_SUBGROUP = range(5)


@pytest.fixture(scope="module")
def check(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("pairing_host") / "pairing_host_check")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        os.path.join(ROOT, "tests", "pairing_host_check.cpp"), "-o", exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr

    def run(commands):
        r = subprocess.run([exe], input="".join(c + "\n" for c in commands), capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
        lines = r.stdout.splitlines()
        assert lines[-1] == "PAIRING HOST CHECK DONE" and len(lines) == len(commands) + 1
        return lines[:-1]
    return run


@pytest.fixture(scope="module")
def schedule(check):
    s = [{"+": 1, "-": -1, "0": 0}[c] for c in check(["naf"])[0]]
    return s


def test_the_headers_schedule_is_the_naf_of_6u_plus_2(schedule):
    assert schedule == pm.schedule_naf()
    assert sum(d * 2**i for i, d in enumerate(reversed(schedule))) == pm.ATE
    assert all(not (a and b) for a, b in zip(schedule, schedule[1:]))


def test_line_tables_are_the_models_bytes(check, schedule):
    tau = int(KAT["tau"], 16)
    pts = [pm.G2, pm.g2_mul(pm.G2, tau)] + [pm.g2_from_seed(s) for s in (1, 2, 3)]
    assert pm.g2_bytes(pts[1]).hex() == KAT["g2"]["tau"]
    out = check(["table " + pm.g2_bytes(p).hex() for p in pts])
    for p, line in zip(pts, out):
        canon, sq, dev = line.split()
        table = pm.line_table(p, schedule)
        assert len(table) == 88
        assert bytes.fromhex(canon) == pm.line_table_bytes(table)
        assert sq == "".join(str(l[0]) for l in table)
        # the device image: the same values times 2^261 (fp.cuh's Montgomery form), canonical
        want = b"".join((c * (1 << 261) % pm.Q).to_bytes(32, "little") for (_, nl, cc) in table for c in (nl[0], nl[1], cc[0], cc[1]))
        assert bytes.fromhex(dev) == want


def test_the_subgroup_test_agrees_with_the_literal_one_on_points_of_both_kinds(check):
    inside = [pm.g2_from_seed(s) for s in range(20, 25)]
    outside = [pm.g2_curve_point(s) for s in range(20, 25)]
    assert all(pm.g2_in_subgroup(p) for p in inside) and all(pm.g2_on_curve(p) and not pm.g2_in_subgroup(p) for p in outside)
    got = check(["parse " + pm.g2_bytes(p).hex() for p in inside + outside])
    assert got == [str(OK)] * 5 + [str(NOT_IN_SUBGROUP)] * 5
    assert check(["table " + pm.g2_bytes(outside[0]).hex()]) == ["refused %d" % NOT_IN_SUBGROUP]


def test_refusals(check):
    g = pm.g2_bytes(pm.G2)
    off_curve = g[:96] + pm.g2_bytes(pm.g2_from_seed(1))[96:]
    cmds, want = [], []
    for part in range(4):                                                              # each coordinate part in turn, at q and at q + its value
        v = int.from_bytes(g[32 * part:32 * part + 32], "little")
        for bad in (pm.Q, v + pm.Q, 2**256 - 1):
            cmds.append("parse " + (g[:32 * part] + bad.to_bytes(32, "little") + g[32 * part + 32:]).hex()); want.append(str(NOT_CANONICAL))
    cmds += ["parse " + bytes(128).hex(), "parse " + off_curve.hex(), "parse " + g.hex()]
    want += [str(IDENTITY), str(OFF_CURVE), str(OK)]
    mont = b"".join((int.from_bytes(g[32 * i:32 * i + 32], "little") * (1 << 256) % pm.Q).to_bytes(32, "little") for i in range(4))
    cmds += ["mont " + mont.hex(), "mont " + g.hex()]
    want += [str(OK), str(OFF_CURVE)]
    assert check(cmds) == want


def test_the_constants_file_is_what_its_generator_writes():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gen_pairing_consts.py"), "--print"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert open(os.path.join(ROOT, "spartan-bn254_amd", "csrc", "pairing_consts.inc")).read() == r.stdout


def _header_arity():
    src = open(os.path.join(ROOT, "include", "sbn254.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    out = {}
    for name in NEW_SYMBOLS:
        m = re.search(r"\b(?:int|void)\s+" + name + r"\s*\(([^;]*?)\)\s*;", src, flags=re.S)
        assert m, f"{name} is not declared in include/sbn254.h"
        out[name] = len([a for a in m.group(1).split(",") if a.strip()])
    return out


def test_the_entry_points_are_exported_bound_and_refuse_a_call_without_a_context(sbn):
    arity = _header_arity()
    assert arity == {"sbn_g2_prepare": 4, "sbn_g2_lines_free": 2, "sbn_pairing_products": 7, "sbn_kzg_verify": 8, "sbn_kzg_verify_batched": 10,
                     "sbn_sparse_eval_verify_kzg": 18}
    L = sbn.lib()
    for name in NEW_SYMBOLS:
        assert name in sbn.EXPORTED_SYMBOLS and hasattr(L, name)
        assert len(getattr(L, name).argtypes) == arity[name], name
    # without a context every call is SBN_EINVAL and leaves its outputs as they were (no device is touched: this runs without a GPU)
    g = pm.g2_bytes(pm.G2)
    G1 = pm.g1_bytes(pm.G1)
    out = C.c_void_p(0x1234)
    assert L.sbn_g2_prepare(None, g, 0, C.byref(out)) == -1 and out.value == 0x1234
    one, gt, acc = (C.c_uint8 * 1)(9), (C.c_uint8 * 384)(*([9] * 384)), C.c_int(9)
    cnt = (C.c_uint32 * 1)(1)
    fake = (C.c_void_p * 1)(0x1000)                                                    # never dereferenced: the context is tested first
    assert L.sbn_pairing_products(None, G1, fake, cnt, C.c_size_t(1), one, gt) == -1
    assert bytes(one) == b"\x09" and bytes(gt) == b"\x09" * 384
    s = (5).to_bytes(32, "little")
    assert L.sbn_kzg_verify(None, 0x1000, 0x1000, G1, s, s, G1, C.byref(acc)) == -1 and acc.value == 9
    assert L.sbn_kzg_verify_batched(None, 0x1000, 0x1000, G1, C.c_size_t(1), s, s, s, G1, C.byref(acc)) == -1 and acc.value == 9
    z = C.c_size_t
    assert L.sbn_sparse_eval_verify_kzg(None, z(1), z(1), z(2), z(2), z(1), 0x1000, 0x1000, s, s, s, 0x1000, 0x1000, 0x1000, 0x1000, s, 0x1000, C.byref(acc)) == -1 and acc.value == 9
    L.sbn_g2_lines_free(None, None)
