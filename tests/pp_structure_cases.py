"""Fixtures of the public-parameter structure tests (tests/test_pp_structure_refs.py on the CPU,
tests/test_gpu_pp_structure.py and tests/test_gpu_pp_view.py on the GPU), built from the Python oracle:

  * a random nv = 4 parameter (keygen_from_scalars with SplitMix64 draws),
  * the degenerate nv = 6 parameter of tests/degenerate_pp.py (trapdoor entries 0, 1 and 1/2),
  * the identities the structure check, the derived verifier parameter and the views rest on, as
    predicates over the oracle's points,
  * helpers that replace or swap whole points inside serialized parameter bytes.

Serialized layout (spartan.PublicParameter.serialize_uncompressed): u64 nv, u64 nv, then per G1 level
u64 count + count x 96 B, u64 nv, per G2 level u64 count + count x 192 B, g (96 B), h (192 B)."""
from functools import lru_cache

import degenerate_pp
import spartan
from bls12_381 import G1, G2
from gen import SplitMix64

RANDOM_NV = 4
RANDOM_SEED = 0x9A7A5EED


class Fixture:
    def __init__(self, nv, gs, hs, t):
        self.nv, self.gs, self.hs = nv, gs, hs
        self.pp, self.vp, self.t = spartan.keygen_from_scalars(nv, gs, hs, t)
        self.bytes = self.pp.serialize_uncompressed()
        self.vp_bytes = self.vp.serialize_uncompressed()


@lru_cache(maxsize=None)
def random_pp():
    rs = SplitMix64(RANDOM_SEED)
    gs, hs = rs.next_fr(), rs.next_fr()
    return Fixture(RANDOM_NV, gs, hs, [rs.next_fr() for _ in range(RANDOM_NV)])


@lru_cache(maxsize=None)
def degenerate():
    gs, hs, t = degenerate_pp.trapdoor()
    d = degenerate_pp.build()
    f = Fixture.__new__(Fixture)
    f.nv, f.gs, f.hs = degenerate_pp.NV, gs, hs
    f.pp, f.vp, f.t = d.pp, d.vp, list(t)
    f.bytes, f.vp_bytes = d.bytes, d.vp_bytes
    return f


# ------------------------------------------------------------------ identities over oracle points
def _sum(curve, pts):
    acc = curve.inf
    for p in pts:
        if p is not None:
            acc = curve.madd(acc, p)
    return curve.to_affine(acc)


def fold_failures(pp):
    """[(curve 1 | 2, level, pair)] with powers[i][2b] + powers[i][2b+1] != powers[i+1][b] (the last
    level's pair against g / h), in the order the library reports them"""
    bad = []
    for c, curve, levels, last in ((1, G1, pp.powers_of_g, pp.g), (2, G2, pp.powers_of_h, pp.h)):
        for i, lvl in enumerate(levels):
            for b in range(len(lvl) // 2):
                target = levels[i + 1][b] if i + 1 < len(levels) else last
                if _sum(curve, [lvl[2 * b], lvl[2 * b + 1]]) != target:
                    bad.append((c, i, b))
    return bad


def odd_sums(pp):
    """sum_b powers_of_g[i][2b+1] for every level"""
    return [_sum(G1, lvl[1::2]) for lvl in pp.powers_of_g]


def sliced(pp, vp, k):
    """the parameter of nv - k variables inside pp, and its verifier parameter"""
    nv = pp.nv - k
    return (spartan.PublicParameter(nv, pp.powers_of_g[k:], pp.powers_of_h[k:], pp.g, pp.h),
            spartan.VerifierParameter(nv, vp.g, vp.h, vp.g_mask_random[k:]))


# ------------------------------------------------------------------ serialized bytes
def point_offset(nv, curve, level, index):
    """byte offset of powers_of_g[level][index] (curve 1) / powers_of_h[level][index] (curve 2)"""
    assert 0 <= level < nv and 0 <= index < 1 << (nv - level)
    pos = 16
    for i in range(nv):
        pos += 8
        if curve == 1 and i == level:
            return pos + 96 * index
        pos += 96 << (nv - i)
    pos += 8
    for i in range(nv):
        pos += 8
        if curve == 2 and i == level:
            return pos + 192 * index
        pos += 192 << (nv - i)
    raise AssertionError("curve must be 1 or 2")


def g_offset(nv):
    return point_offset(nv, 2, nv - 1, 1) + 192


def point_size(curve):
    return 96 if curve == 1 else 192


def get_point(b, nv, curve, level, index):
    o = point_offset(nv, curve, level, index)
    return b[o:o + point_size(curve)]


def replace_point(b, nv, curve, level, index, point_bytes):
    o = point_offset(nv, curve, level, index)
    assert len(point_bytes) == point_size(curve) and b[o:o + len(point_bytes)] != point_bytes
    return b[:o] + point_bytes + b[o + len(point_bytes):]


def replace_g(b, nv, point_bytes):
    o = g_offset(nv)
    assert len(point_bytes) == 96 and b[o:o + 96] != point_bytes
    return b[:o] + point_bytes + b[o + 96:]


def swap_points(b, nv, curve, level, i, j):
    pi, pj = get_point(b, nv, curve, level, i), get_point(b, nv, curve, level, j)
    return replace_point(replace_point(b, nv, curve, level, i, pj), nv, curve, level, j, pi)


def expected_failures(nv, curve, level, index):
    """the pairs a replaced point breaks: (level, index >> 1), and (level - 1, index) above level 0"""
    out = [(curve, level, index >> 1)]
    if level > 0:
        out.append((curve, level - 1, index))
    return sorted(out)
