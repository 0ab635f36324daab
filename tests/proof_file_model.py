"""The proof file of harness/sbn_spartan.cpp (harness/standalone_host.hpp has the layout) in plain Python: the checker of its reader and writer.

    "SBNP" | version u32 = 1 | mode u8 (0 snark, 1 nizk) | kzg u8 | 0 u16 | num_cons, num_vars, num_inputs, num_nz_entries u64 | digest_len u32, digest
    | inputs 32 B each | proof_len u64, proof          all little-endian"""
from transcript_model import R_MOD

SNARK, NIZK = 0, 1


class ProofFileError(ValueError):
    """args[0]: short, magic, version, mode, kzg, reserved, length, input, trailing, mode_mismatch, kzg_mismatch"""


def write(mode, kzg, num_cons, num_vars, num_nz, digest, inputs, proof, version=1, reserved=0, magic=b"SBNP", num_inputs=None, digest_len=None, proof_len=None):
    """inputs: integers.  The keyword arguments behind `proof` write files a reader must refuse"""
    le = lambda x, n: int(x).to_bytes(n, "little")                                    # noqa: E731
    return magic + le(version, 4) + bytes([mode, kzg]) + le(reserved, 2) + le(num_cons, 8) + le(num_vars, 8) + le(len(inputs) if num_inputs is None else num_inputs, 8) + \
        le(num_nz, 8) + le(len(digest) if digest_len is None else digest_len, 4) + digest + b"".join(le(x, 32) for x in inputs) + \
        le(len(proof) if proof_len is None else proof_len, 8) + proof


def read(data, want_mode=-1, want_kzg=-1):
    """-> dict(mode, kzg, num_cons, num_vars, num_inputs, num_nz, digest, inputs (bytes), proof); refusals in the order the reader meets them"""
    data = bytes(data)
    pos = 0

    def take(n, why="short"):
        nonlocal pos
        if n > len(data) - pos:
            raise ProofFileError(why)
        out = data[pos:pos + n]
        pos += n
        return out
    if take(4) != b"SBNP":
        raise ProofFileError("magic")
    head = take(8)
    if int.from_bytes(head[:4], "little") != 1:
        raise ProofFileError("version")
    mode, kzg = head[4], head[5]
    if mode > 1:
        raise ProofFileError("mode")
    if kzg > 1 or (kzg and mode == NIZK):
        raise ProofFileError("kzg")
    if head[6:8] != bytes(2):
        raise ProofFileError("reserved")
    if want_mode >= 0 and want_mode != mode:
        raise ProofFileError("mode_mismatch")
    if want_kzg >= 0 and want_kzg != kzg:
        raise ProofFileError("kzg_mismatch")
    nc, nv, ni, nz = (int.from_bytes(take(8), "little") for _ in range(4))
    digest = take(int.from_bytes(take(4), "little"), "length")
    if ni > (len(data) - pos) // 32:
        raise ProofFileError("length")
    inputs = take(32 * ni)
    if any(int.from_bytes(inputs[i:i + 32], "little") >= R_MOD for i in range(0, len(inputs), 32)):
        raise ProofFileError("input")
    proof = take(int.from_bytes(take(8), "little"), "length")
    if pos != len(data):
        raise ProofFileError("trailing")
    return dict(mode=mode, kzg=kzg, num_cons=nc, num_vars=nv, num_inputs=ni, num_nz=nz, digest=digest, inputs=inputs, proof=proof)
