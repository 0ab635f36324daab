"""CPU: csrc/ptau_host.hpp — the section table and the header section of a .ptau file, and its two G2 points out of Montgomery form through
g2_parse_checked — against the literal model of tests/ptau_model.py.  tests/ptau_host_check.cpp includes the header alone and is built with g++ under
ASan + UBSan as a stand-alone program; it is fed one case per line, each copied into a buffer of exactly its length, and compared line by line."""
import os
import subprocess

import pytest

import pairing_model as pm
import ptau_model as ptm
from conftest import ROOT
from test_ptau_model_cpu import g2_refusals, kat, scan_refusals      # noqa: F401  (kat is a fixture)


@pytest.fixture(scope="module")
def check(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("ptau_host") / "ptau_host_check")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        os.path.join(ROOT, "tests", "ptau_host_check.cpp"), "-o", exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr

    def run(kind, cases, lines_per_case=None):
        """-> the words of each result line"""
        text = "".join(f"{kind} {bytes(f).hex() or '-'}\n" for f in cases)
        r = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]                # a sanitizer report ends the program with another status
        lines = r.stdout.splitlines()
        want = len(cases) if lines_per_case is None else sum(lines_per_case)
        assert lines[-1] == "PTAU HOST CHECK DONE" and len(lines) == want + 1
        return [ln.split() for ln in lines[:-1]]
    return run


def model_line(data):
    """the line ptau_host_check prints for a file, from the model"""
    try:
        s = ptm.scan(data)
        o = s["off_g2"]
        t = ptm.g2_read(data[o + 128:o + 256])
        g = ptm.g2_read(data[o:o + 128])
    except ptm.PtauError as e:
        return ["refused", e.reason]
    return ["ok"] + [str(s[k]) for k in ("power", "ceremony_power", "n_g1", "n_g2", "off_g1", "off_g2")] + [pm.g2_bytes(g).hex(), pm.g2_bytes(t).hex()]


def test_the_fixture_in_both_section_orders(check, kat):          # noqa: F811
    files = [kat["file"], kat["permuted"], kat["file"] + b"\xff" * 7, ptm.write_ptau(3, kat["tau"], powers=kat["g1"], ceremony_power=28)]
    got = check("ptau", files)
    for f, g in zip(files, got):
        assert model_line(f)[0] == "ok" and g == model_line(f)
        assert (g[7], g[8]) == (kat["g2"].hex(), kat["tau_g2"].hex())                 # the G2 conversion against the fixture's canonical points
    assert got[0][1:5] == ["3", "3", "15", "8"] and got[3][2] == "28" and got[1][5:7] != got[0][5:7]
    assert got[2] == got[0]


def test_every_prefix_of_the_fixture(check, kat):                 # noqa: F811
    for f in (kat["file"], kat["permuted"]):
        got = check("prefixes", [f], lines_per_case=[len(f)])
        assert len(got) == len(f) == 3280
        for n, g in enumerate(got):
            assert g[0] == "refused" and g == model_line(f[:n]), n


def test_every_scan_refusal_overflow_cases_included(check, kat):  # noqa: F811
    cases = list(scan_refusals(kat))
    assert {w for w, _ in cases} == set(ptm.SCAN_REASONS)
    got = check("ptau", [f for _, f in cases] + [b""])
    for (why, f), g in zip(cases, got):
        assert g == ["refused", why] == model_line(f), why
    assert got[-1] == ["refused", "short"]


def test_every_g2_refusal(check, kat):                            # noqa: F811
    cases = list(g2_refusals(kat))
    assert {w for w, _ in cases} == set(ptm.G2_REASONS)
    got = check("g2", [b for _, b in cases])
    for (why, _), g in zip(cases, got):
        assert g == ["refused", why], why
    # the same through a whole file, in either position; a bad tauG2[2] changes nothing
    f = kat["file"]
    files = [ptm.replace_g2(f, at, b) for at in (0, 1) for _, b in cases]
    got = check("ptau", files + [ptm.replace_g2(f, 2, cases[0][1])])
    for fl, (why, _), g in zip(files, cases + cases, got):
        assert g == ["refused", why] == model_line(fl)
    assert got[-1] == model_line(f)


def test_g2_points_convert_to_their_canonical_bytes(check):
    pts, P = [], None
    for _ in range(16):
        P = pm.g2_add(P, pm.G2)
        pts.append(P)
    got = check("g2", [ptm.g2_bytes(P) for P in pts])
    for P, g in zip(pts, got):
        assert g == ["ok", pm.g2_bytes(P).hex()]
