"""CPU: tests/circom_model.py on its own footing — the hand-assembled files of tests/golden/circom_kat.json through the reader, the writers against the
reader, and a file made of a raw circuit against the instance built from that circuit directly."""
import pytest

import circom_model as cm
import nizk_model as nm
import snark_model as sm
from conftest import golden

R = cm.R_MOD
H = bytes.fromhex


def _trip(rows):
    return [(r, c, int(v)) for r, c, v in rows]


def test_golden_files_give_the_hand_worked_triplets_and_values():
    g = golden("circom_kat.json")
    r = cm.read_r1cs(H(g["r1cs"]))
    assert {k: r[k] for k in g["header"]} == g["header"]
    assert [r["a"], r["b"], r["c"]] == [_trip(g["raw"][k]) for k in "ABC"]
    assert (r["payload_off"], r["payload_len"], r["dropped"]) == (g["payload_off"], g["payload_len"], [0, 0, 0])
    assert cm.walk_arrays(r) == (g["run_first"], g["mat_first"])
    nc, nv, ni, ncp, nvp = cm.shape(r)
    assert dict(num_vars=nv, num_inputs=ni, num_cons_padded=ncp, num_vars_padded=nvp) == g["shape"] and nc == 3
    assert list(cm.to_sparse_matrices_padded(r, nvp)) == [_trip(g["padded"][k]) for k in "ABC"]
    assert cm.first_bad_wire(r) is None
    vals, off = cm.read_wtns(H(g["wtns"]))
    assert [str(v) for v in vals] == g["witness"] and H(g["wtns"])[off:off + 32] == (1).to_bytes(32, "little")
    inputs, table = cm.split_witness(vals, ni)
    assert [str(v) for v in inputs] == g["input"] and [str(v) for v in table] == g["vars"] + ["0"] and len(table) == g["vars_table_len"]
    # the witness satisfies the circuit it was written for
    inst = sm.Instance(ncp, nvp, ni, cm.triplet_lists(cm.to_sparse_matrices_padded(r, nvp)))
    assert (inst.nc, inst.nv) == (ncp, nvp) and sm.is_sat(inst, table, inputs) == (True, 0, None)
    assert sm.is_sat(inst, [table[0] + 1] + table[1:], inputs)[0] is False


@pytest.mark.parametrize("order", [(1, 2, 3), (2, 1), (1, 3, 2), (9, 2, 77, 1)])
def test_write_then_read_round_trips(order):
    shape = dict(n_wires=9, n_pub_out=2, n_pub_in=1, n_prv_in=3, n_labels=40)
    cons = [([(0, 5), (8, R - 1)], [], [(3, 7)]), ([], [(4, 1), (4, 2)], []), ([(1, R), (2, 9)], [(5, R + 5)], [(6, 2**256 - 1), (7, 0)])]
    data = cm.write_r1cs(shape, cons, section_order=order, extra_sections={9: b"\x00" * 5, 77: b"xyz"})
    r = cm.read_r1cs(data)
    assert (r["num_variables"], r["num_pub_inputs"], r["num_prv_inputs"], r["num_labels"], r["num_constraints"]) == (9, 3, 3, 40, 3)
    assert r["counts"] == [2, 0, 1, 0, 2, 0, 2, 1, 2] and r["dropped"] == [1, 1, 1]
    assert r["a"] == [(0, 0, 5), (0, 8, R - 1), (2, 2, 9)] and r["b"] == [(1, 4, 1), (1, 4, 2)] and r["c"] == [(0, 3, 7), (2, 7, 0)]
    assert len(r["file_order"]) == 10 and [e[3] for e in r["file_order"]].count(None) == 3
    a, b, c = cm.to_sparse_matrices_padded(r, 8)
    assert a == [(0, 8, 5), (0, 4, R - 1), (2, 10, 9)] and b == [(1, 0, 1), (1, 0, 2)] and c == [(0, 11, 7), (2, 3, 0)]      # wires 0, 3 (= n_pub), 4 (= n_pub + 1), 8 (= nWires - 1)
    assert cm.first_bad_wire(dict(r, file_order=r["file_order"] + [(0, 2, 9, 1)])) == 10
    vals = [1, 2, 3, R - 1, 0]
    assert cm.read_wtns(cm.write_wtns(vals))[0] == vals == cm.parse_wtns(cm.write_wtns(vals))
    with pytest.raises(cm.CircomError):
        cm.read_wtns(cm.write_wtns([1, R]))
    assert cm.parse_wtns(cm.write_wtns([1, R + (1 << 70) + 5])) == [1, (R + (1 << 70) + 5) & (2**64 - 1)]      # the example's low 64 bits


@pytest.mark.parametrize("key", nm.KEYS)
def test_a_file_made_of_a_raw_circuit_gives_the_instance_of_that_circuit(key):
    nc, nv, ni, _ = key
    mats, vars_, inputs = nm.instance(key)
    want = sm.Instance(nc, nv, ni, mats)
    r1cs, wtns = cm.raw_to_circom(nc, nv, ni, mats, vars_, inputs)
    r = cm.read_r1cs(r1cs)
    assert cm.shape(r) == (nc, nv, ni, want.nc, want.nv)
    got = cm.triplet_lists(cm.to_sparse_matrices_padded(r, want.nv))
    assert tuple((list(a), list(b), list(c)) for a, b, c in got) == tuple((list(a), list(b), list(c)) for a, b, c in want.mats)
    vals, _ = cm.read_wtns(wtns)
    got_inputs, table = cm.split_witness(vals, ni)
    assert got_inputs == inputs and table == sm.pad_vars(vars_, len(table)) and len(table) <= want.nv
    assert sm.is_sat(sm.Instance(want.nc, want.nv, ni, got), table, got_inputs)[0]
