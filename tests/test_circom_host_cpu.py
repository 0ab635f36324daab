"""CPU: csrc/circom_host.hpp — the section scan of a circom .r1cs file, the walk over its entry counts and the span of a .wtns file's values — against the
literal model of tests/circom_model.py.  tests/circom_host_check.cpp includes the header alone and is built with g++ under ASan + UBSan as a stand-alone
program; it is fed one file per line, copied into a buffer of exactly the file's length, and compared line by line."""
import os
import subprocess

import pytest

import circom_model as cm
from conftest import ROOT, golden

R = cm.R_MOD
H = bytes.fromhex
SHAPE = dict(n_wires=7, n_pub_out=1, n_pub_in=2, n_prv_in=1, n_labels=11)
CONS = [([(4, 1), (0, R - 1)], [(5, 2)], [(6, 3)]), ([(1, 5)], [(2, 6), (3, 7), (0, 8)], [(0, 9)])]


@pytest.fixture(scope="module")
def check(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("circom_host") / "circom_host_check")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        os.path.join(ROOT, "tests", "circom_host_check.cpp"), "-o", exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr

    def run(kind, files):
        """-> the words of each file's result line"""
        text = "".join(f"{kind} {bytes(f).hex() or '-'}\n" for f in files)
        r = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]                # a sanitizer report ends the program with another status
        lines = r.stdout.splitlines()
        assert lines[-1] == "CIRCOM HOST CHECK DONE" and len(lines) == len(files) + 1
        return [ln.split() for ln in lines[:-1]]
    return run


def model_line(data):
    """the line circom_host_check prints for a .r1cs file, from the model"""
    try:
        r = cm.read_r1cs(data)
    except cm.CircomError as e:
        return ["refused", e.args[0]]
    _, nv, ni, ncp, nvp = cm.shape(r)
    rf, mf = cm.walk_arrays(r)
    nnz = [sum(r["counts"][m::3]) for m in range(3)]
    hs = _header_fields(data, r)
    return ["ok", "32", *map(str, hs), str(r["num_constraints"]), str(r["num_pub_inputs"]), str(r["payload_off"]), str(r["payload_len"]), str(nv), str(ni), str(ncp), str(nvp),
            *map(str, nnz), "|", *map(str, rf), "|", *map(str, mf)]


def _header_fields(data, r):
    """nWires, nPubOut, nPubIn, nPrvIn, nLabels read where the format puts them: behind the first section of type 1"""
    off = 12
    while True:
        t, size = int.from_bytes(data[off:off + 4], "little"), int.from_bytes(data[off + 4:off + 12], "little")
        off += 12
        if t == 1:
            break
        off += size
    q = off + 36
    vals = [int.from_bytes(data[q + 4 * i:q + 4 * i + 4], "little") for i in range(4)] + [int.from_bytes(data[q + 16:q + 24], "little")]
    assert vals[0] == r["num_variables"] and vals[1] + vals[2] == r["num_pub_inputs"] and vals[3] == r["num_prv_inputs"] and vals[4] == r["num_labels"]
    return vals


def test_golden_file(check):
    g = golden("circom_kat.json")
    data = H(g["r1cs"])
    got = check("r1cs", [data])[0]
    assert got == model_line(data)
    bar = [i for i, w in enumerate(got) if w == "|"]
    assert [int(x) for x in got[bar[0] + 1:bar[1]]] == g["run_first"] and [int(x) for x in got[bar[1] + 1:]] == g["mat_first"]
    assert [int(got[9]), int(got[10])] == [g["payload_off"], g["payload_len"]]
    assert [int(x) for x in got[11:15]] == [g["shape"][k] for k in ("num_vars", "num_inputs", "num_cons_padded", "num_vars_padded")]
    w = check("wtns", [H(g["wtns"])])[0]
    vals, off = cm.read_wtns(H(g["wtns"]))
    assert w == ["ok", str(off), str(len(vals))] and [str(v) for v in vals] == g["witness"]


ORDERS = {
    "header_first": dict(section_order=(1, 2, 3)),
    "constraints_first": dict(section_order=(2, 1)),
    "wire_map_between": dict(section_order=(1, 3, 2)),
    "unknown_type_between": dict(section_order=(2, 77, 1), extra_sections={77: b"\xaa" * 10}),
    "odd_section_in_front": dict(section_order=(9, 1, 2), extra_sections={9: b"\x01\x02\x03"}),      # the payload is unaligned in the file
    "a_second_header_and_constraints": dict(section_order=(1, 2, 1, 2)),
}


def test_section_orders_and_run_shapes(check):
    files = [cm.write_r1cs(SHAPE, CONS, **kw) for kw in ORDERS.values()]
    empty_ends = [([], [(1, 1)], []), ([(2, 2), (3, 3)], [], [(4, 4)]), ([(5, 5)], [(6, 6)], [])]          # the first and the last run are empty
    files.append(cm.write_r1cs(SHAPE, empty_ends))
    files.append(cm.write_r1cs(SHAPE, [([], [], [])] * 4))                                               # no entries at all
    files.append(cm.write_r1cs(SHAPE, []))                                                               # no constraints
    files.append(cm.write_r1cs(dict(SHAPE, n_wires=4), [([(0, 1)], [], [])]))                           # nWires = 1 + num_pub_inputs: no variable
    # section 2 longer than its walk: the rest is ignored, as the reference ignores it
    n = cm.read_r1cs(files[0])["payload_len"]
    files.append(cm.write_r1cs(SHAPE, CONS, section_order=(1, 2, 3), constraints_size=n + 20))
    got = check("r1cs", files)
    for f, g in zip(files, got):
        want = model_line(f)
        assert want[0] == "ok" and g == want
    offs = {int(g[9]) for g in got[:5]}
    assert len(offs) >= 4 and any(o % 4 for o in offs)                                                   # the payload at several offsets, an unaligned one among them


def _refusals():
    big = 1 << 40
    yield "magic", cm.write_r1cs(SHAPE, CONS, magic=b"r1cx")
    yield "version", cm.write_r1cs(SHAPE, CONS, version=2)
    yield "field_size", cm.write_r1cs(SHAPE, CONS, field_size=64)
    yield "no_header", cm.write_r1cs(SHAPE, CONS, section_order=(2, 3))
    yield "no_constraints", cm.write_r1cs(SHAPE, CONS, section_order=(1, 3))
    yield "io", cm.write_r1cs(SHAPE, CONS, section_order=(1, 2))[:-1]                                    # the last record is cut
    yield "io", cm.write_r1cs(SHAPE, CONS, section_order=(3, 1, 2))[:30]
    yield "io", cm.write_r1cs(SHAPE, CONS, section_order=(1, 3), num_sections=5)                         # more sections announced than there are, none of type 2
    # an empty section of type 77 (0x4d) in front whose size field is rewritten to 2^40: the skip lands far past the end
    yield "io", cm.write_r1cs(SHAPE, CONS, section_order=(77, 1, 2), extra_sections={77: b""}).replace(b"\x4d\x00\x00\x00" + bytes(8), b"\x4d\x00\x00\x00" + big.to_bytes(8, "little"))
    yield "wires", cm.write_r1cs(dict(SHAPE, n_wires=3), CONS)
    yield "prime", cm.write_r1cs(SHAPE, CONS, prime=R + 2)
    yield "prime", cm.write_r1cs(SHAPE, CONS, prime=0x30644e72e131a029b85045b68181585d97816a916871ca8d3c208c16d87cfd47)      # the base field's
    yield "section_end", cm.write_r1cs(SHAPE, CONS, section_order=(1, 2, 3), constraints_size=9 * 36)    # the walk would read on into the wire map
    yield "section_end", cm.write_r1cs(SHAPE, CONS, section_order=(1, 2, 3), num_constraints=3)          # a third constraint's counts lie in the next section
    yield "section_end", cm.write_r1cs(SHAPE, CONS, num_constraints=0xffffffff)
    yield "section_end", cm.write_r1cs(SHAPE, [([(1, 1)] * 3, [], [])], constraints_size=4 + 36 * 2 + 8)  # a record crosses the end


def test_every_refusal(check):
    cases = list(_refusals())
    got = check("r1cs", [f for _, f in cases])
    for (why, f), g in zip(cases, got):
        with pytest.raises(cm.CircomError) as e:
            cm.read_r1cs(f)
        assert e.value.args[0] == why, (why, e.value.args)
        assert g == ["refused", why], (why, g)


def test_every_truncation_of_the_golden_files_is_refused(check):
    g = golden("circom_kat.json")
    data = H(g["r1cs"])
    cut = data[:12 + 12 + 64 + 12 + g["payload_len"]]                # the wire map behind the two sections is never read: cutting into it changes nothing
    assert check("r1cs", [cut])[0] == model_line(cut) == model_line(data)
    prefixes = [cut[:n] for n in range(len(cut))]
    got = check("r1cs", prefixes)
    for n, (p, res) in enumerate(zip(prefixes, got)):
        with pytest.raises(cm.CircomError):
            cm.read_r1cs(p)
        assert res[0] == "refused", n
    w = H(g["wtns"])
    prefixes = [w[:n] for n in range(len(w))]
    got = check("wtns", prefixes)
    for n, (p, res) in enumerate(zip(prefixes, got)):
        with pytest.raises(cm.CircomError):
            cm.read_wtns(p)
        assert res[0] == "refused", n


def test_wtns_spans_and_refusals(check):
    vals = [1, 5, 6, 7, R - 1]
    body = b"".join(v.to_bytes(32, "little") for v in vals)
    ok = [cm.write_wtns(vals), cm.write_wtns(vals, sections=[(2, body)]), cm.write_wtns(vals, sections=[(7, b"abc"), (2, body), (1, b"")]),
          cm.write_wtns([], sections=[(2, b"")])]
    got = check("wtns", ok)
    for f, g in zip(ok, got):
        v, off = cm.read_wtns(f)
        assert g == ["ok", str(off), str(len(v))] and v == cm.parse_wtns(f)
    bad = [("magic", cm.write_wtns(vals, magic=b"wtnz")), ("twice", cm.write_wtns(vals, sections=[(2, body), (2, body)])), ("none", cm.write_wtns(vals, sections=[(1, b"x" * 40)])),
           ("size", cm.write_wtns(vals, sections=[(2, body + b"\0")])), ("io", cm.write_wtns(vals)[:-1]), ("io", cm.write_wtns(vals, sections=[(2, body), (5, b"tail")])[:-1]),
           ("io", b"wtns\x02\0\0\0"), ("io", b"wt")]
    got = check("wtns", [f for _, f in bad])
    for (why, f), g in zip(bad, got):
        with pytest.raises(cm.CircomError) as e:
            cm.read_wtns(f)
        assert e.value.args[0] == why and g == ["refused", why], (why, g)
    # what the example does with two of them, without a word
    assert cm.parse_wtns(bad[1][1]) == vals + vals and cm.parse_wtns(bad[4][1]) == vals[:-1]
