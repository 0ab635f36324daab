"""circom's .r1cs and .wtns readers in plain Python: a literal restatement of the reference's R1CS::from_reader and to_sparse_matrices_padded
(src/r1cs_reader.rs, cited by line) and of parse_wtns (examples/keyless_benchmark.rs:38-72) — the checker of csrc/circom_host.hpp and of sbn_circom_*.

    read_r1cs                   R1CS::from_reader (r1cs_reader.rs:55-191).  What goes BEYOND the reference is marked "REFUSAL BEYOND THE REFERENCE"
    to_sparse_matrices_padded   :213-242
    num_private_vars, shape     :255-257 and snark_model.pad_shape (snark.rs:74-90)
    parse_wtns                  keyless_benchmark.rs:38-72, literally: it truncates and concatenates without a word
    read_wtns                   parse_wtns with the cases it mishandles refused (what sbn_circom_wtns_load does)
    write_r1cs / write_wtns     the writers of the test files
    raw_to_circom               a raw circuit of snark_model.satisfying_instance as a pair of files

Scalars are Python integers; a file is bytes."""
import snark_model as sm
from snark_model import R_MOD

FIELD_BYTES = 32


class CircomError(ValueError):
    """args[0]: "magic", "version", "io" (a read past the end), "field_size", "no_header", "no_constraints" — the reference's R1CSError — or one of the
    refusals beyond it: "prime", "wires", "section_end", "bad_wire" (args[1]: the entry in file order); for .wtns files: "magic", "io", "twice", "none", "size",
    "short", "value" (args[1]: the index)"""


class _Reader:
    """Read + Seek over bytes: read_exact fails past the end (std::io::ErrorKind::UnexpectedEof), seek never does"""

    def __init__(self, data):
        self.d, self.pos = data, 0

    def read_exact(self, n):
        if self.pos + n > len(self.d):
            raise CircomError("io")
        out = self.d[self.pos:self.pos + n]
        self.pos += n
        return out

    def u32(self):
        return int.from_bytes(self.read_exact(4), "little")

    def u64(self):
        return int.from_bytes(self.read_exact(8), "little")


def bytes_to_scalar(b):
    """r1cs_reader.rs:286-299: Fr::from_bigint is None for a value >= r"""
    if len(b) != 32:
        return None
    v = int.from_bytes(b, "little")
    return v if v < R_MOD else None


def _read_header_section(rd, num_sections):
    """r1cs_reader.rs:95-129"""
    rd.pos = 12                                                                                  # :99
    for _ in range(num_sections):                                                                # :101
        section_type = rd.u32(); section_size = rd.u64()                                         # :102-103
        if section_type == 1:                                                                    # :105
            field_size = rd.u32()                                                                # :107
            prime = rd.d[rd.pos:rd.pos + field_size]
            rd.pos += field_size                                                                 # :110 (a seek: the prime is skipped)
            num_variables = rd.u32(); num_pub_outputs = rd.u32(); num_pub_inputs = rd.u32(); num_prv_inputs = rd.u32()      # :112-115
            num_labels = rd.u64(); num_constraints = rd.u32()                                    # :116-117
            return num_constraints, num_variables, num_pub_outputs + num_pub_inputs, num_prv_inputs, num_labels, field_size, prime      # :120-122
        rd.pos += section_size                                                                   # :124
    raise CircomError("no_header")                                                               # :128


def _read_constraints_section(rd, num_sections, num_constraints, field_size, out):
    """r1cs_reader.rs:131-191; out: what the model records beside the three matrices (the section's place, the per-run counts, every entry in file order)"""
    rd.pos = 12                                                                                  # :137
    for _ in range(num_sections):                                                                # :139
        section_type = rd.u32(); section_size = rd.u64()                                         # :140-141
        if section_type == 2:                                                                    # :143
            out["payload_off"], out["payload_len"] = rd.pos, section_size
            end = rd.pos + section_size
            mats = ([], [], [])
            for constraint_idx in range(num_constraints):                                        # :149
                for m in range(3):                                                               # :150-181, the three copies of one loop
                    if rd.pos + 4 > end:
                        raise CircomError("section_end")                                         # REFUSAL BEYOND THE REFERENCE: it ignores section_size here
                    n = rd.u32()                                                                 # :151
                    if rd.pos + n * (4 + field_size) > end:
                        raise CircomError("section_end")                                         # REFUSAL BEYOND THE REFERENCE, as above
                    out["counts"].append(n)
                    for _ in range(n):                                                           # :152
                        col = rd.u32()                                                           # :153
                        scalar = bytes_to_scalar(rd.read_exact(field_size))                      # :154-156
                        out["file_order"].append((m, constraint_idx, col, scalar))
                        if scalar is not None:
                            mats[m].append((constraint_idx, col, scalar))                        # :157
                        else:
                            out["dropped"][m] += 1
            return mats                                                                          # :184
        rd.pos += section_size                                                                   # :186
    raise CircomError("no_constraints")                                                          # :190


def read_r1cs(data):
    """R1CS::from_reader (r1cs_reader.rs:55-93) -> dict(num_constraints, num_variables, num_pub_inputs, num_prv_inputs, num_labels, a, b, c) and what the
    model records: payload_off, payload_len, counts (entries per run, 3 per constraint), dropped (per matrix), file_order [(m, row, wire, value or None)]"""
    rd = _Reader(bytes(data))
    if rd.read_exact(4) != b"r1cs":                                                              # :57-61
        raise CircomError("magic")
    version = rd.u32()                                                                           # :64
    if version != 1:
        raise CircomError("version")                                                             # :65-67
    num_sections = rd.u32()                                                                      # :70
    num_constraints, num_variables, num_pub, num_prv, num_labels, field_size, prime = _read_header_section(rd, num_sections)      # :73-74
    if field_size != 32:
        raise CircomError("field_size")                                                          # :76-78
    if prime != R_MOD.to_bytes(32, "little"):
        raise CircomError("prime")                                                               # REFUSAL BEYOND THE REFERENCE: it never looks at the prime
    if num_variables < 1 + num_pub:
        raise CircomError("wires")                                                               # REFUSAL BEYOND THE REFERENCE: num_private_vars (:255-257) underflows
    out = dict(counts=[], dropped=[0, 0, 0], file_order=[])
    a, b, c = _read_constraints_section(rd, num_sections, num_constraints, field_size, out)      # :81
    out.update(num_constraints=num_constraints, num_variables=num_variables, num_pub_inputs=num_pub, num_prv_inputs=num_prv, num_labels=num_labels, a=a, b=b, c=c)
    return out


def first_bad_wire(r1cs):
    """REFUSAL BEYOND THE REFERENCE (it aliases such a wire onto another column): the lowest entry, in file order, that is kept and names a wire >= nWires"""
    for g, (_, _, wire, scalar) in enumerate(r1cs["file_order"]):
        if scalar is not None and wire >= r1cs["num_variables"]:
            return g
    return None


def num_private_vars(r1cs):
    return r1cs["num_variables"] - 1 - r1cs["num_pub_inputs"]                                    # :255-257


def to_sparse_matrices_padded(r1cs, num_vars_padded):
    """r1cs_reader.rs:213-242 -> three lists of (row, col, value)"""
    n_pub = r1cs["num_pub_inputs"]                                                               # :218

    def remap_col(col):                                                                          # :224-235
        if col == 0:
            return num_vars_padded
        if col <= n_pub:
            return num_vars_padded + col
        return col - n_pub - 1
    return tuple([(row, remap_col(col), val) for row, col, val in r1cs[k]] for k in "abc")       # :237-241


def shape(r1cs):
    """-> (num_cons, num_vars, num_inputs, num_cons_padded, num_vars_padded): the raw shape the file gives Instance::new and snark.rs:74-90's padding
    (examples/keyless_benchmark.rs:99 pads num_cons with next_power_of_two() alone: it differs for one constraint only, which R1CSProof cannot take)"""
    nc, nv, ni = r1cs["num_constraints"], num_private_vars(r1cs), r1cs["num_pub_inputs"]
    ncp, nvp, _, _ = sm.pad_shape(nc, nv, ni)
    return nc, nv, ni, ncp, nvp


def triplet_lists(mats):
    """[(row, col, val)] x 3 -> ((rows, cols, vals),) x 3, as r1cs_upload and the models take matrices"""
    return tuple(([t[0] for t in m], [t[1] for t in m], [t[2] for t in m]) for m in mats)


def walk_arrays(r1cs):
    """-> (run_first [3 n + 1], mat_first [3 n]) of csrc/circom_host.hpp from the model's per-run counts"""
    run_first, mat_first, tot, per = [], [], 0, [0, 0, 0]
    for k, n in enumerate(r1cs["counts"]):
        run_first.append(tot); mat_first.append(per[k % 3])
        tot += n; per[k % 3] += n
    return run_first + [tot], mat_first


# ---- the witness ---------------------------------------------------------------------------------------------------------------------

def parse_wtns(data):
    """keyless_benchmark.rs:38-72, literally -> [values]"""
    data = bytes(data)
    if len(data) < 4 or data[0:4] != b"wtns":                                                    # :43-45
        raise CircomError("magic")
    if len(data) < 12:
        raise CircomError("io")                                                                  # :47 (the slice panics)
    num_sections = int.from_bytes(data[8:12], "little")                                          # :47
    offset = 12                                                                                  # :48
    witness_values = []
    for _ in range(num_sections):                                                                # :51
        if offset + 12 > len(data):
            break                                                                                # :52
        section_id = int.from_bytes(data[offset:offset + 4], "little")                           # :53
        section_size = int.from_bytes(data[offset + 4:offset + 12], "little")                    # :54
        offset += 12                                                                             # :55
        if section_id == 2:                                                                      # :57
            num_witnesses = section_size // 32                                                   # :58
            for i in range(num_witnesses):                                                       # :59
                start = offset + i * 32
                if start + 32 > len(data):
                    break                                                                        # :61
                b = data[start:start + 32]
                v = int.from_bytes(b, "little")
                witness_values.append(v if v < R_MOD else int.from_bytes(b[0:8], "little"))      # :64-66
        offset += section_size                                                                   # :69
    return witness_values


def read_wtns(data):
    """parse_wtns with what it mishandles refused -> (values, the byte offset of the first).  On every file this accepts the values are parse_wtns's"""
    data = bytes(data)
    if len(data) < 4:
        raise CircomError("io")
    if data[0:4] != b"wtns":
        raise CircomError("magic")
    if len(data) < 12:
        raise CircomError("io")
    num_sections = int.from_bytes(data[8:12], "little")
    offset, found = 12, None
    for _ in range(num_sections):
        if offset + 12 > len(data):
            raise CircomError("io")                                                              # REFUSAL: the example stops reading
        section_id = int.from_bytes(data[offset:offset + 4], "little")
        section_size = int.from_bytes(data[offset + 4:offset + 12], "little")
        offset += 12
        if offset + section_size > len(data):
            raise CircomError("io")                                                              # REFUSAL: the example keeps the values that are there
        if section_id == 2:
            if found is not None:
                raise CircomError("twice")                                                       # REFUSAL: the example appends the second section's values
            if section_size % 32:
                raise CircomError("size")                                                        # REFUSAL: the example drops the tail
            found = (offset, section_size // 32)
        offset += section_size
    if found is None:
        raise CircomError("none")
    values = [int.from_bytes(data[found[0] + 32 * i:found[0] + 32 * i + 32], "little") for i in range(found[1])]
    for i, v in enumerate(values):
        if v >= R_MOD:
            raise CircomError("value", i)                                                        # REFUSAL: the example takes the low 64 bits
    assert values == parse_wtns(data)
    return values, found[0]


def split_witness(values, num_inputs):
    """-> (input, vars padded to the table sbn_circom_wtns_load returns); fewer than 1 + num_inputs values are refused"""
    if len(values) < 1 + num_inputs:
        raise CircomError("short")
    inputs, vars_ = values[1:1 + num_inputs], values[1 + num_inputs:]
    n = sm.npo2(max(len(vars_), num_inputs + 1))
    return inputs, vars_ + [0] * (n - len(vars_))


# ---- writers -------------------------------------------------------------------------------------------------------------------------

def _le(x, n):
    return int(x).to_bytes(n, "little")


def write_r1cs(shape_, constraints, section_order=(1, 2, 3), extra_sections=None, magic=b"r1cs", version=1, field_size=32, prime=R_MOD, num_constraints=None,
               num_sections=None, constraints_size=None):
    """shape_: dict(n_wires, n_pub_out, n_pub_in, n_prv_in, n_labels); constraints: [(A, B, C)], each a list of (wire, value); section_order: the types
    in file order (1: header, 2: constraints, anything else: the bytes extra_sections gives it, default a wire map of n_wires u64).  The keyword arguments
    behind it write files a reader must refuse"""
    extra = dict(extra_sections or {})
    head = _le(field_size, 4) + _le(prime, 32) + _le(shape_["n_wires"], 4) + _le(shape_["n_pub_out"], 4) + _le(shape_["n_pub_in"], 4) + _le(shape_["n_prv_in"], 4) + \
        _le(shape_["n_labels"], 8) + _le(len(constraints) if num_constraints is None else num_constraints, 4)
    cons = b""
    for abc in constraints:
        for run in abc:
            cons += _le(len(run), 4) + b"".join(_le(w, 4) + _le(v, 32) for w, v in run)
    out = magic + _le(version, 4) + _le(len(section_order) if num_sections is None else num_sections, 4)
    for t in section_order:
        body = head if t == 1 else cons if t == 2 else extra.get(t, b"".join(_le(i, 8) for i in range(shape_["n_wires"])))
        size = constraints_size if (t == 2 and constraints_size is not None) else len(body)
        out += _le(t, 4) + _le(size, 8) + body
    return out


def write_wtns(values, sections=None, magic=b"wtns"):
    """values: the witness; sections: [(id, bytes)] in file order (default: circom's header section 1, then the values as section 2)"""
    if sections is None:
        sections = [(1, _le(32, 4) + _le(R_MOD, 32) + _le(len(values), 4)), (2, b"".join(_le(v, 32) for v in values))]
    out = magic + _le(2, 4) + _le(len(sections), 4)
    for sid, body in sections:
        out += _le(sid, 4) + _le(len(body), 8) + body
    return out


def raw_to_circom(num_cons, num_vars, num_inputs, mats, vars_, inputs, **kw):
    """a raw circuit in the numbering vars | 1 | inputs (snark_model.satisfying_instance) -> (.r1cs bytes, .wtns bytes).  The entries of a matrix must be in
    row order, as a file holds them; their order inside a row is kept.  Wire 0 is the constant, 1 .. num_inputs the inputs, the variables follow"""
    def wire(col):
        return col + num_inputs + 1 if col < num_vars else col - num_vars
    cons = [([], [], []) for _ in range(num_cons)]
    for m, (rows, cols, vals) in enumerate(mats):
        assert list(rows) == sorted(rows), "a file holds a matrix in constraint order"
        for r, c, v in zip(rows, cols, vals):
            cons[r][m].append((wire(c), v))
    shape_ = dict(n_wires=1 + num_inputs + num_vars, n_pub_out=num_inputs // 2, n_pub_in=num_inputs - num_inputs // 2, n_prv_in=0, n_labels=1 + num_inputs + num_vars)
    return write_r1cs(shape_, cons, **kw), write_wtns([1] + list(inputs) + list(vars_))
