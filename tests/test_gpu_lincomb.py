"""spx_lincomb_g1 / spx_lincomb_g2 (the batch verifier's segmented linear combination) against the
oracle's msm_naive: segment lengths around one wave and past one block's stride, the edge scalars, an
infinite base, a segment that cancels to infinity and one whose reduction tree meets equal points."""
import pytest

from bls12_381 import G1, G2, R, g1_uncompressed, g2_uncompressed, msm_naive
from gen import SplitMix64

pytestmark = pytest.mark.gpu

# (length, kind): "cancel" = one point twice with s and r - s; "double" = one point twice with equal scalars
SEGMENTS = [(1, "plain"), (2, "cancel"), (2, "double"), (63, "plain"), (64, "plain"), (65, "plain"), (257, "plain")]
EDGE = [0, 1, R - 1, (1 << 128) - 1]


def _points(curve, count):
    """count distinct affine points (k + 1) P0, by additions (cheap for the Python oracle)"""
    P0 = curve.from_affine(curve.mul_affine(curve.gen, 0xC0FFEE))
    acc, out = P0, []
    for _ in range(count):
        out.append(acc)
        acc = curve.add(acc, P0)
    return curve.batch_to_affine(out)


def _build(curve, g2):
    rng = SplitMix64(0x11C0 + g2)
    total = sum(n for n, _ in SEGMENTS)
    pts = _points(curve, total)
    bases, scalars, seg, want = [], [], [0], []
    pos = 0
    for n, kind in SEGMENTS:
        b = pts[pos : pos + n]
        pos += n
        if kind == "cancel":
            s = rng.next_fr_nonzero()
            b, k = [b[0], b[0]], [s, R - s]
        elif kind == "double":
            s = rng.next_fr_nonzero() >> 127
            b, k = [b[0], b[0]], [s, s]
        else:
            # mostly 128-bit scalars; one 255-bit one in sixteen; the edge values, an infinite base and a
            # doubled point (equal scalars, adjacent lanes) where the segment has room
            k = [rng.next_fr() if i % 16 == 5 else rng.next_fr() >> 127 for i in range(n)]
            if n >= 63:
                k[:4] = EDGE
                b[7] = None
                b[11], k[11] = b[10], k[10]
        # G2's longest segment: the oracle's share is capped by repeating 32 bases (the sum over equal
        # bases collapses to one multiplication each); every other segment goes to msm_naive as it is
        if g2 and n > 65:
            b = [b[i % 32] for i in range(n)]
            acc = {}
            for i in range(n):
                acc[i % 32] = (acc.get(i % 32, 0) + k[i]) % R
            ref = msm_naive(curve, b[:32], [acc[i] for i in range(32)])
        else:
            ref = msm_naive(curve, b, k)
        bases += b
        scalars += k
        seg.append(len(bases))
        want.append(curve.to_affine(ref))
    return bases, scalars, seg, want


@pytest.fixture(scope="module")
def data():
    return {"g1": _build(G1, False), "g2": _build(G2, True)}


@pytest.mark.parametrize("curve", ["g1", "g2"])
def test_lincomb_matches_msm_naive(spx, ctx, data, curve):
    bases, scalars, seg, want = data[curve]
    unc = g1_uncompressed if curve == "g1" else g2_uncompressed
    fn = spx.lincomb_g1 if curve == "g1" else spx.lincomb_g2
    got = fn(ctx, b"".join(unc(b) for b in bases), scalars, seg)  # several segments in one call
    assert len(got) == len(SEGMENTS)
    assert want[1] is None  # the cancelling segment sums to infinity
    for s, (g, w) in enumerate(zip(got, want)):
        assert g == unc(w), (curve, SEGMENTS[s])
    # one segment alone, and the whole input as a single segment (the sum of the segments' sums)
    lo, hi = seg[4], seg[5]
    assert fn(ctx, b"".join(unc(b) for b in bases[lo:hi]), scalars[lo:hi], [0, hi - lo]) == [unc(want[4])]
    C = G1 if curve == "g1" else G2
    tot = C.inf
    for w in want:
        tot = C.add(tot, C.from_affine(w))
    assert fn(ctx, b"".join(unc(b) for b in bases), scalars, [0, len(bases)]) == [unc(C.to_affine(tot))]


def test_lincomb_argument_checks(spx, ctx):
    P = g1_uncompressed(G1.gen)
    with pytest.raises(spx.InvalidArgument):
        spx.lincomb_g1(ctx, P * 2, [1, 2], [0, 1])  # offsets must end at n
    with pytest.raises(spx.InvalidArgument):
        spx.lincomb_g1(ctx, P * 2, [1, 2], [0, 2, 1, 2])  # and ascend
    with pytest.raises(spx.SerializationError):
        spx.lincomb_g1(ctx, P, (R).to_bytes(32, "little"), [0, 1])  # canonical scalars only
    assert spx.lincomb_g1(ctx, P * 2, [1, 2], [0, 0, 2, 2]) == [
        g1_uncompressed(None), g1_uncompressed(G1.mul_affine(G1.gen, 3)), g1_uncompressed(None)]  # empty segments
