"""spx_g1_decompress / spx_g2_decompress (the batch verifier's decompression kernel) against the oracle's
decompression, byte for byte on the uncompressed output: random points of both y signs, infinity, an x
with no point on the curve, a non-canonical x, at batch sizes around one wave."""
import pytest

from bls12_381 import (FLAG_INF, FLAG_POS_Y, G1, G2, Q, g1_compress, g1_decompress, g1_uncompressed, g2_compress,
                       g2_decompress, g2_uncompressed, ser_fq, ser_fq2)
from gen import SplitMix64

pytestmark = pytest.mark.gpu


def _raw_fq(x, flags=0):  # 48 bytes of any x < 2^382, canonical or not
    b = bytearray(x.to_bytes(48, "little"))
    b[47] |= flags
    return bytes(b)


def _cases(curve):
    """[(compressed, expected uncompressed, ok)] : 40 points, infinity, a non-residue, non-canonical x"""
    g2 = curve is G2
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
    assert signs == {0, FLAG_POS_Y}  # both y signs
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
        out.append((_raw_fq(Q + 5) + good[48:], bytes(size), False))
        out.append((good[:48] + _raw_fq(Q, good[95] & 0xC0), bytes(size), False))
    else:
        out.append((_raw_fq(Q + 5, good[47] & 0xC0), bytes(size), False))
        out.append((_raw_fq(Q), bytes(size), False))
    return out


@pytest.fixture(scope="module")
def cases():
    return {"g1": _cases(G1), "g2": _cases(G2)}


@pytest.mark.parametrize("curve", ["g1", "g2"])
@pytest.mark.parametrize("n", [1, 63, 64, 65])
def test_decompress_matches_oracle(spx, ctx, cases, curve, n):
    pool = cases[curve]
    fn = spx.g1_decompress if curve == "g1" else spx.g2_decompress
    size = 96 if curve == "g1" else 192
    # n = 1: every kind of case alone; otherwise the pool cycled from the specials on, so that rejected
    # and infinite points sit among valid ones in the first and in the second wave
    batches = [[c] for c in (pool[0], pool[40], pool[41], pool[42], pool[43])] if n == 1 else \
        [[pool[(38 + i) % len(pool)] for i in range(n)]]
    for batch in batches:
        out, ok = fn(ctx, b"".join(c[0] for c in batch))
        assert ok == [c[2] for c in batch]
        for i, c in enumerate(batch):
            assert out[size * i : size * (i + 1)] == c[1], (curve, n, i)
