"""Compressed wire images of public and verifier parameters, shared by tests/test_pp_compressed_cases.py
(CPU: pins this helper to the oracle) and tests/test_gpu_pp_compressed.py (the HIP loader and serializer).

oracle/py/spartan.py has only the uncompressed serializers; the compressed form is what ark-serialize's
default serialize() writes: the same framing in the derive order of commitment/data_structures.rs:9-17
(u64 nv, u64 nv, per G1 level u64 2^(nv-i) and the points, u64 nv, per G2 level likewise, g, h) with
48 / 96-byte compressed points. Every byte comes from the oracle's g1_compress / g2_compress over the points of
spartan.keygen_from_scalars."""
from functools import lru_cache

import degenerate_pp
import spartan
from bls12_381 import (F2_ONE, FLAG_INF, FLAG_POS_Y, G1, G2, G2_B, Q, f2_mul, f2_neg, f2_sqr, f2_sub, g1_compress,
                       g1_decompress, g1_uncompressed, g2_compress, g2_decompress, g2_uncompressed, ser_fq, ser_fq2,
                       ser_u64)
from gen import SplitMix64

NVS = (1, 2, 5)
SEED = 0xC0A9


def pp_image(pp, first_level=0):
    """compressed PublicParameter bytes of levels first_level .. nv - 1 (the parameter of nv - first_level
    variables inside pp)"""
    nv = pp.nv - first_level
    out = [ser_u64(nv), ser_u64(nv)]
    for lvl in pp.powers_of_g[first_level:]:
        out.append(ser_u64(len(lvl)))
        out.extend(g1_compress(p) for p in lvl)
    out.append(ser_u64(nv))
    for lvl in pp.powers_of_h[first_level:]:
        out.append(ser_u64(len(lvl)))
        out.extend(g2_compress(p) for p in lvl)
    out.append(g1_compress(pp.g))
    out.append(g2_compress(pp.h))
    return b"".join(out)


def vp_image(vp):
    return (ser_u64(vp.nv) + g1_compress(vp.g) + g2_compress(vp.h) + ser_u64(len(vp.g_mask_random))
            + b"".join(g1_compress(x) for x in vp.g_mask_random))


def image_length(nv):
    return 24 + 16 * nv + 144 * (2 ** (nv + 1) - 2) + 144


def uncompressed_length(nv):
    return 24 + 16 * nv + 288 * (2 ** (nv + 1) - 2) + 288


def point_offset(nv, curve, level, index):
    """byte offset of powers_of_g[level][index] (curve 1) / powers_of_h[level][index] (curve 2) in an image"""
    assert 0 <= level < nv and 0 <= index < 1 << (nv - level)
    pos = 16
    for cid, ps in ((1, 48), (2, 96)):
        for i in range(nv):
            pos += 8
            if (cid, i) == (curve, level):
                return pos + ps * index
            pos += ps << (nv - i)
        pos += 8
    raise AssertionError


def g_offset(nv):
    return image_length(nv) - 144


def h_offset(nv):
    return image_length(nv) - 96


def parse_image(img):
    """(nv, G1 levels, G2 levels, g, h) of an image as lists of compressed points"""
    pos = 0

    def u64():
        nonlocal pos
        v = int.from_bytes(img[pos:pos + 8], "little")
        pos += 8
        return v

    def level(ps):
        nonlocal pos
        k = u64()
        pts = [img[pos + ps * i:pos + ps * (i + 1)] for i in range(k)]
        pos += ps * k
        return pts

    nv = u64()
    g1 = [level(48) for _ in range(u64())]
    g2 = [level(96) for _ in range(u64())]
    g, h = img[pos:pos + 48], img[pos + 48:pos + 144]
    assert pos + 144 == len(img)
    return nv, g1, g2, g, h


class Fixture:
    def __init__(self, pp, vp):
        self.nv, self.pp, self.vp = pp.nv, pp, vp
        self.bytes = pp.serialize_uncompressed()
        self.image = pp_image(pp)
        self.vp_bytes = vp.serialize_uncompressed()
        self.vp_image = vp_image(vp)


@lru_cache(maxsize=None)
def random_pp(nv):
    rs = SplitMix64(SEED + nv)
    pp, vp, _ = spartan.keygen_from_scalars(nv, rs.next_fr_nonzero(), rs.next_fr_nonzero(), [rs.next_fr() for _ in range(nv)])
    return Fixture(pp, vp)


@lru_cache(maxsize=None)
def degenerate():
    d = degenerate_pp.build()
    return Fixture(d.pp, d.vp)


# ------------------------------------------------------------------ points for the kernels
def raw_fq(x, flags=0):
    """48 bytes of any x < 2^382, canonical or not"""
    b = bytearray(x.to_bytes(48, "little"))
    b[47] |= flags
    return bytes(b)


@lru_cache(maxsize=None)
def pool(cid):
    """The 44 cases of tests/test_gpu_decompress.py for curve cid (1 | 2): [(compressed, expected
    uncompressed, ok)], 40 random points of both y signs, infinity, an x with no point, two non-canonical x"""
    g2 = cid == 2
    curve = G2 if g2 else G1
    compress, decompress = (g2_compress, g2_decompress) if g2 else (g1_compress, g1_decompress)
    uncompressed = g2_uncompressed if g2 else g1_uncompressed
    size = 192 if g2 else 96
    rng = SplitMix64(0xDEC0 + g2)
    out, signs = [], set()
    for _ in range(40):
        P = curve.mul_affine(curve.gen, rng.next_fr_nonzero())
        c = compress(P)
        signs.add(c[-1] & FLAG_POS_Y)
        assert decompress(c) == P
        out.append((c, uncompressed(P), True))
    assert signs == {0, FLAG_POS_Y}
    out.append((compress(None), uncompressed(None), True))
    k = 1
    while True:  # the first x = k (G1) / k + u (G2) whose x^3 + b is not a square
        c = ser_fq2((k, 1), FLAG_POS_Y) if g2 else ser_fq(k, FLAG_POS_Y)
        try:
            decompress(c)
        except ValueError:
            break
        k += 1
    out.append((c, bytes(size), False))
    good = out[0][0]
    if g2:  # x >= q in either half
        out.append((raw_fq(Q + 5) + good[48:], bytes(size), False))
        out.append((good[:48] + raw_fq(Q, good[95] & 0xC0), bytes(size), False))
    else:
        out.append((raw_fq(Q + 5, good[47] & 0xC0), bytes(size), False))
        out.append((raw_fq(Q), bytes(size), False))
    assert len(out) == 44
    return tuple(out)


SPECIALS = (40, 41, 42, 43)  # infinity, no point, non-canonical twice


def batch(cid, n):
    """n cases of pool(cid). Valid points fill the batch; every special case is then placed at an even
    index, at an odd index and at the last index (as far as n has room), so that a rejected or infinite
    point shares a lane or a lockstep pair with a valid one on either side and ends a batch."""
    p = pool(cid)
    picks = [p[i % 40] for i in range(n)]
    placed = {s: set() for s in SPECIALS}
    if n >= 2:
        slots = list(range(n - 1))
        at = 0
        for s in SPECIALS:
            for parity in (0, 1):
                while at < len(slots) and slots[at] % 2 != parity:
                    at += 1
                if at < len(slots):
                    picks[slots[at]] = p[s]
                    placed[s].add("even" if parity == 0 else "odd")
                    at += 1
    return picks, placed


def last_batches(cid, n):
    """for each special case, the batch(cid, n) with that case as its last point"""
    p = pool(cid)
    out = []
    for s in SPECIALS:
        picks, _ = batch(cid, n)
        picks = list(picks)
        picks[n - 1] = p[s]
        out.append(picks)
    return out


# ------------------------------------------------------------------ Algorithm 9's other branch
def _f2_pow(a, e):
    acc = F2_ONE
    for bit in bin(e)[2:]:
        acc = f2_sqr(acc)
        if bit == "1":
            acc = f2_mul(acc, a)
    return acc


@lru_cache(maxsize=None)
def fq_rhs_points(count=3):
    """G2 curve points (x, c u), c in Fq: y^2 = -c^2 lies in Fq and is no square there, so x^3 + b takes the
    alpha = -1 branch of the Fq2 square root (the root is u x0), which no random point reaches. x is a cube
    root of -c^2 - b: q^2 - 1 = 9 m with 3 not dividing m, so t^(1/3 mod m) is a cube root of a cube t up to
    one of the nine 9th roots of unity. [(compressed, uncompressed, True)]"""
    n = Q * Q - 1
    assert n % 9 == 0 and n % 27 != 0
    m = n // 9
    e = pow(3, -1, m)
    k = 2
    while _f2_pow((k, 1), n // 3) == F2_ONE:  # a non-cube: its m-th power has order 9
        k += 1
    g9 = _f2_pow((k, 1), m)
    out, c = [], 1
    while len(out) < 2 * count:
        c += 1
        y = (0, c)
        t = f2_sub(f2_sqr(y), G2_B)
        if _f2_pow(t, n // 3) != F2_ONE:
            continue
        x = _f2_pow(t, e)
        for _ in range(9):
            if f2_mul(f2_sqr(x), x) == t:
                break
            x = f2_mul(x, g9)
        assert f2_mul(f2_sqr(x), x) == t and G2.on_curve((x, y))
        for P in ((x, y), (x, f2_neg(y))):  # both signs
            comp = g2_compress(P)
            assert g2_decompress(comp) == P
            out.append((comp, g2_uncompressed(P), True))
    return tuple(out)
