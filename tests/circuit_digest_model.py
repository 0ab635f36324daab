"""The library's own circuit digest (include/sbn254.h: sbn_circom_r1cs_digest) in plain Python over hashlib.shake_256 — the checker of
k_circom_digest_leaves and of the root in csrc/circom_host.hpp.  It is NOT the reference's R1CSShape::get_digest (zlib over bincode, r1cs.rs:97-101).

    leaf(m, j) = SHAKE256("sbn254/r1cs-digest/leaf/v1" | u8 m | u64le j | u32le k | k x (u32le row | u32le col | val[32]))[0..32]
                 entries 128 j .. 128 j + k - 1 of matrix m, k = min(128, nnz[m] - 128 j); no leaf for nnz[m] = 0
    root       = SHAKE256("sbn254/r1cs-digest/root/v1" | u64le num_constraints | num_variables | num_pub_inputs | num_cons_padded | num_vars_padded
                          | for m = 0, 1, 2: u64le nnz[m] | the leaves of m in order)[0..32]

The entries are what sbn_circom_r1cs_download returns: kept entries in file order, remapped columns, canonical values."""
import hashlib

import circom_model as cm

LEAF_DOMAIN = b"sbn254/r1cs-digest/leaf/v1"
ROOT_DOMAIN = b"sbn254/r1cs-digest/root/v1"
LEAF_ENTRIES = 128
RATE = 136                                     # SHAKE256's rate in bytes


def _le(x, n):
    return int(x).to_bytes(n, "little")


def leaf_message(m, j, entries):
    """entries: the leaf's [(row, col, val)]"""
    return LEAF_DOMAIN + _le(m, 1) + _le(j, 8) + _le(len(entries), 4) + b"".join(_le(r, 4) + _le(c, 4) + _le(v, 32) for r, c, v in entries)


def leaf(m, j, entries):
    return hashlib.shake_256(leaf_message(m, j, entries)).digest(32)


def leaves(m, mat):
    """mat: [(row, col, val)] -> the leaves of matrix m, in order"""
    return [leaf(m, j, mat[LEAF_ENTRIES * j:LEAF_ENTRIES * (j + 1)]) for j in range((len(mat) + LEAF_ENTRIES - 1) // LEAF_ENTRIES)]


def digest(shape5, mats):
    """shape5: (num_constraints, num_variables, num_pub_inputs, num_cons_padded, num_vars_padded); mats: three lists of (row, col, val)"""
    msg = ROOT_DOMAIN + b"".join(_le(x, 8) for x in shape5)
    for m, mat in enumerate(mats):
        msg += _le(len(mat), 8) + b"".join(leaves(m, mat))
    return hashlib.shake_256(msg).digest(32)


def digest_of_file(data):
    """the digest sbn_circom_r1cs_digest gives for the bytes of a .r1cs file"""
    r = cm.read_r1cs(data)
    _, _, _, ncp, nvp = cm.shape(r)
    return digest((r["num_constraints"], r["num_variables"], r["num_pub_inputs"], ncp, nvp), cm.to_sparse_matrices_padded(r, nvp))


def rate_edge_counts():
    """the k in 1 .. 128 at which a leaf's message ends on a block edge of the sponge: its length is 135 mod 136 (the two pad bits share the block's
    last byte) or 0 mod 136 (the pad fills a block of its own)"""
    return {k: (39 + 40 * k) % RATE for k in range(1, LEAF_ENTRIES + 1) if (39 + 40 * k) % RATE in (0, RATE - 1)}
