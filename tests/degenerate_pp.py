"""A legal public parameter full of infinite and repeated points, shared by tests/test_pp_degenerate.py
(CPU: pins the oracles on it) and tests/test_gpu_pp_degenerate.py (the HIP library from load to proof).

Multilinear KZG: powers_of_g[i][x] = g^{eq(t[i..], x)} with variable i the lowest bit of x. A trapdoor
entry t_i = 0 puts every odd point of level i at infinity (and half of every lower level), t_i = 1 every
even point, and t_i = 1/2 makes the two points of every pair of level i equal. With
t = [1/2, 0, random, 1, random, 1/2] the G2 levels, whose pairs raw[2j] + raw[2j+1] the preprocessing
adds (k_precompute, pair_sum), hold every class of pair: equal, infinite + finite, finite + infinite,
both infinite, and two different finite points; level 0 mixes finite and infinite points inside the
chunks of 32 that the batch inversion walks (k_normalize): chunks that start with infinities, end with
them and have them between finite points; the verifier parameter's g^{t_1} is infinity. build()
asserts all of that on the Python oracle's points before anything is compared."""
from functools import lru_cache

import spartan
from bls12_381 import R
from gen import SplitMix64

NV = 6
SEED = 0xDE6E9A7A
PAIR_CLASSES = ("equal", "infinite + finite", "finite + infinite", "both infinite", "different")
NORM_CHUNK = 32  # kNormChunk (msm_impl.hpp)


def pair_class(a, b):
    if a is None or b is None:
        return "both infinite" if a is b else "infinite + finite" if a is None else "finite + infinite"
    return "equal" if a == b else "different"


def trapdoor():
    rs = SplitMix64(SEED)
    half = pow(2, -1, R)
    return rs.next_fr(), rs.next_fr(), [half, 0, rs.next_fr(), 1, rs.next_fr(), half]


def chunk_shapes(infinite):
    """of a list of is-infinity flags, per chunk of 32 that holds both kinds: does it start with
    infinity, end with it, hold one between two finite points"""
    out = []
    for k in range(0, len(infinite), NORM_CHUNK):
        c = infinite[k:k + NORM_CHUNK]
        if any(c) and not all(c):
            fin = [i for i, f in enumerate(c) if not f]
            out.append({"starts": c[0], "ends": c[-1], "between": any(c[fin[0]:fin[-1]])})
    return out


class DegeneratePP:
    def __init__(self):
        gs, hs, t = trapdoor()
        self.pp, self.vp, self.t = spartan.keygen_from_scalars(NV, gs, hs, t)
        self.bytes = self.pp.serialize_uncompressed()
        self.vp_bytes = self.vp.serialize_uncompressed()
        # the pair classes of the G2 levels, per level
        self.classes = [[pair_class(lvl[2 * j], lvl[2 * j + 1]) for j in range(len(lvl) // 2)] for lvl in self.pp.powers_of_h]
        seen = {c for lvl in self.classes for c in lvl}
        assert seen == set(PAIR_CLASSES), "pair classes missing: %s" % (set(PAIR_CLASSES) - seen)
        # level 0 of G1 as the batch inversion walks it, and the 32 pair sums of level 0 of G2 (infinite
        # where both points are: equal points double, and no pair is P, -P)
        assert len(self.pp.powers_of_g[0]) == 1 << NV
        self.g1_chunks = chunk_shapes([p is None for p in self.pp.powers_of_g[0]])
        self.g2_chunks = chunk_shapes([c == "both infinite" for c in self.classes[0]])
        for chunks in (self.g1_chunks, self.g2_chunks):
            assert chunks, "no chunk of 32 mixes finite and infinite points"
            assert any(c["starts"] for c in chunks) and any(c["ends"] for c in chunks) and any(c["between"] for c in chunks)
        self.inf_g1 = sum(p is None for lvl in self.pp.powers_of_g for p in lvl)
        self.inf_g2 = [sum(p is None for p in lvl) for lvl in self.pp.powers_of_h]
        self.equal_pairs = [lvl.count("equal") for lvl in self.classes]
        inf_mask = [p is None for p in self.vp.g_mask_random]
        assert any(inf_mask) and not all(inf_mask)
        assert self.pp.g is not None and self.pp.h is not None


@lru_cache(maxsize=None)
def build():
    return DegeneratePP()
