"""Point sets with chosen groups of equal bases, and the expected row commitments over them (test infrastructure for
tests/test_gpu_merge_seams.py and tests/test_merge_model_cpu.py).

A set is laid out by an explicit list of group sizes: group i repeats pool point i, the columns of all groups are shuffled over the
row so that no group is contiguous, and h is a point of its own, a member of a group, or absent.  The pool is a few thousand points
of known discrete log (oracle_lib.g1_mul_gen_batch).  Expected values come from oracle_lib.commit_rows on the full matrix (which
knows nothing of groups) for R <= 2049 and from the grouped form above that: per-group sums in Python integers mod r, then
oracle_lib.msm_pippenger over the unique bases plus blind * h."""
import random

import pyref

R_MOD = pyref.R
INF = bytes(64)
POOL_N = 4200
_POOL = {}


def sb(v):
    return v.to_bytes(32, "little")


def pack(vals):
    return b"".join(v.to_bytes(32, "little") for v in vals)


def unpack(b):
    return [int.from_bytes(b[i:i + 32], "little") for i in range(0, len(b), 32)]


def pool(ol):
    """POOL_N distinct points k_i G with random known k_i, plus their discrete logs; built once per process"""
    if not _POOL:
        rng = random.Random(0x5eed)
        dl = [rng.randrange(2, R_MOD) for _ in range(POOL_N)]
        xy = ol.g1_mul_gen_batch(pack(dl), 8)
        _POOL["pts"] = [xy[64 * i:64 * i + 64] for i in range(POOL_N)]
        _POOL["dl"] = dl
        assert len(set(_POOL["pts"])) == POOL_N
    return _POOL["pts"]


class PointSet:
    """cols[j]: the key of column j's point (a pool index, "inf", or ("neg", pool index)); hkey likewise or None"""

    def __init__(self, ol, cols, hkey):
        self.ol, self.cols, self.hkey, self.R = ol, cols, hkey, len(cols)
        self.G = b"".join(self.point(k) for k in cols)
        self.h = self.point(hkey) if hkey is not None else None

    def point(self, key):
        if key == "inf":
            return INF
        if isinstance(key, tuple):
            return self.ol.g1_neg(pool(self.ol)[key[1]])
        return pool(self.ol)[key]

    def unique(self):
        """number of distinct points among G and h (the merge's U)"""
        return len(set(self.cols) | ({self.hkey} if self.hkey is not None else set()))


def make_set(ol, sizes, seed, pad_to=None, h="own", keys=None):
    """groups of the given sizes (group i -> keys[i], default pool index i), then singletons up to pad_to columns; the columns are
    shuffled.  h: "own" (a point of no group), ("group", i) (the base of group i) or None"""
    keys = list(keys) if keys else list(range(len(sizes)))
    cols = [k for k, n in zip(keys, sizes) for _ in range(n)]
    nxt = 1 + max([len(sizes) - 1] + [k if isinstance(k, int) else k[1] for k in keys if k != "inf"])      # singletons: pool points no group uses
    while pad_to is not None and len(cols) < pad_to:
        cols.append(nxt)
        nxt += 1
    assert pad_to is None or len(cols) == pad_to
    random.Random(seed).shuffle(cols)
    hkey = nxt if h == "own" else None if h is None else keys[h[1]]
    return PointSet(ol, cols, hkey)


def grouped_rows(ps, Z, blinds, L):
    """the grouped form: sum the scalars of equal bases mod r, one MSM over the unique bases (+ blind * h)"""
    uniq = sorted(set(ps.cols), key=str)
    pts = b"".join(ps.point(k) for k in uniq) + (ps.h or INF)
    at = {k: i for i, k in enumerate(uniq)}
    out = b""
    for i in range(L):
        acc = [0] * len(uniq)
        row = Z[i * ps.R:(i + 1) * ps.R]
        for k, v in zip(ps.cols, row):
            acc[at[k]] += v
        sc = pack([a % R_MOD for a in acc] + [blinds[i] if blinds else 0])
        out += ps.ol.msm_pippenger(sc, pts, 4)
    return out


def expected_rows(ps, Z, blinds, L):
    """Z: L * R ints row-major, blinds: L ints or None -> L x 64 B"""
    assert len(Z) == L * ps.R and (blinds is None or ps.h is not None)
    if ps.R <= 2049:
        return ps.ol.commit_rows(pack(Z), pack(blinds) if blinds else None, L, ps.R, ps.G, ps.h or INF, 8)
    return grouped_rows(ps, Z, blinds, L)


def inf_flags(want):
    return bytes(1 if want[i:i + 64] == INF else 0 for i in range(0, len(want), 64))
