"""Inputs of the subgroup membership tests, shared by the host and the GPU suites.

The ground truth of every case is the oracle's definition, [r] P = O (Curve.mul of oracle/py/bls12_381.py),
computed once per curve. Classes:
  a  random multiples of the generator                       members
  b  random curve points (random x, solve for y)             non-members
  c  [r] (b): pure cofactor torsion                          non-members
  d  generator multiple + (c)                                non-members
  e  points of small prime order l < 2^16, l | cofactor      non-members
  f  infinity                                                member
  g  a non-canonical coordinate, a point off the curve       rejected
cases() asserts that the oracle calls every (a) a member and every (b) - (e) a non-member, so a degenerate
draw cannot hide a failure."""
import functools
import random

from bls12_381 import (FLAG_POS_Y, G1, G2, Q, R, g1_decompress, g1_uncompressed, g2_decompress, g2_uncompressed,
                       ser_fq, ser_fq2)

Z = -0xD201000000010000
H1 = (Z - 1) ** 2 // 3
H2 = (Z**8 - 4 * Z**7 + 5 * Z**6 - 4 * Z**4 + 6 * Z**3 - 4 * Z**2 - 4 * Z + 13) // 9
assert (Z - 1) ** 2 % 3 == 0 and (Z**8 - 4 * Z**7 + 5 * Z**6 - 4 * Z**4 + 6 * Z**3 - 4 * Z**2 - 4 * Z + 13) % 9 == 0

CURVES = {1: (G1, H1, g1_uncompressed, 96), 2: (G2, H2, g2_uncompressed, 192)}


def random_point(cid, rng):
    """a uniformly drawn x with a point on the curve above it (affine)"""
    while True:
        try:
            if cid == 1:
                return g1_decompress(ser_fq(rng.randrange(Q), FLAG_POS_Y * rng.randrange(2)))
            return g2_decompress(ser_fq2((rng.randrange(Q), rng.randrange(Q)), FLAG_POS_Y * rng.randrange(2)))
        except ValueError:
            continue


def small_primes(h):
    return [l for l in range(2, 1 << 16) if h % l == 0 and all(l % d for d in range(2, int(l**0.5) + 1))]


def in_subgroup_oracle(curve, A):
    return A is None or curve.is_inf(curve.mul(curve.from_affine(A), R))


def _affine_mul(curve, A, k):
    return curve.to_affine(curve.mul(curve.from_affine(A), k))


def _affine_add(curve, A, B):
    return curve.to_affine(curve.add(curve.from_affine(A), curve.from_affine(B)))


@functools.lru_cache(maxsize=None)
def cases(cid, seed=0x5B6):
    """[(class name, uncompressed bytes, expected flag)] for curve cid (1: G1, 2: G2)"""
    curve, h, ser, _ = CURVES[cid]
    rng = random.Random(seed + cid)
    out = []

    def add(name, A, want):
        assert curve.on_curve(A)
        assert in_subgroup_oracle(curve, A) == want, (name, "the oracle disagrees with the class")
        out.append((name, ser(A), want))

    randoms = [random_point(cid, rng) for _ in range(3)]
    for P in randoms:  # the group order is h r
        assert curve.is_inf(curve.mul(curve.from_affine(P), h * R))
    add("a generator", curve.gen, True)
    multiples = [_affine_mul(curve, curve.gen, rng.randrange(1, R)) for _ in range(3)]
    for A in multiples:
        add("a multiple", A, True)
    torsion = [_affine_mul(curve, P, R) for P in randoms]
    for P, T, A in zip(randoms, torsion, multiples):
        add("b random", P, False)
        add("c torsion", T, False)
        add("d multiple + torsion", _affine_add(curve, A, T), False)
    primes = small_primes(h)
    assert primes, "the cofactor has small prime factors"
    for l in primes:
        T = None
        for _ in range(4):  # [#E / l] P: finite for all but 1 / l of the points when the l-part is cyclic
            T = _affine_mul(curve, random_point(cid, rng), h * R // l)
            if T is not None:
                break
        while T is None:
            # l^2 | #E with an l-part that is not cyclic (Z_l x Z_l): [#E / l] kills every point. Clear
            # everything but the l-part instead and climb down to order l.
            m = h * R
            while m % l == 0:
                m //= l
            T = _affine_mul(curve, random_point(cid, rng), m)
            while T is not None and _affine_mul(curve, T, l) is not None:
                T = _affine_mul(curve, T, l)
        assert curve.is_inf(curve.mul(curve.from_affine(T), l))
        add("e order %d" % l, T, False)
    add("f infinity", None, True)
    # g: x + q in the first coordinate (still below 2^382: no flag bit), and (x, y + 1)
    good = ser(multiples[0])
    out.append(("g non-canonical", (int.from_bytes(good[:48], "little") + Q).to_bytes(48, "little") + good[48:], False))
    y0 = int.from_bytes(good[-48:], "little")
    out.append(("g off the curve", good[:-48] + ((y0 + 1) % Q).to_bytes(48, "little"), False))
    return tuple(out)


def interleaved(cid, n):
    """n cases cycling through the classes so that neighbouring lanes differ in outcome: (bytes, flags)"""
    cs = cases(cid)
    members = [c for c in cs if c[2]]
    others = [c for c in cs if not c[2]]
    order = []
    for i in range(max(len(members), len(others))):
        order.append(others[i % len(others)])
        order.append(members[i % len(members)])
    pick = [order[i % len(order)] for i in range(n)]
    return b"".join(c[1] for c in pick), [c[2] for c in pick]
