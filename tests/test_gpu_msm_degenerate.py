"""spx_msm_g1 / spx_msm_g2 with bases at infinity, byte-equal to the oracle's MSM. An infinite base is a
legal input (ark-serialize's infinity encoding); on the device it is the (0, 0) sentinel that the
accumulation loop skips (k_accum_aff: for G2 a predicate combined over the lane pair, in a loop whose
arithmetic exchanges through DPP between the pair's lanes). The cases put finite and infinite
references side by side in one wave (every third base infinite), leave whole runs of references
infinite so that all-infinite partial sums reach k_accum_xyzz, the hot-bucket reduction and the
weighting tree, and cover the results that are themselves infinity. The finite bases are level 0 of a
GPU-generated public parameter, so no point is computed in Python. The same mixed input under the
wide window plan (c = 17, folded signs) is the "every third base infinite" case of
tests/msm_wide_check.py."""
import random

import pytest

from bls12_381 import g1_uncompressed, g2_uncompressed

import msm_wide_check as wc

pytestmark = pytest.mark.gpu

R = wc.R
NV = 10
INF = {"g1": g1_uncompressed(None), "g2": g2_uncompressed(None)}
SIZE = {"g1": 96, "g2": 192}


@pytest.fixture(scope="module")
def bases(spx, ctx):
    """{curve: 2^10 finite uncompressed points}"""
    g1, g2 = wc.pp_bases(spx.MLProofForR1CS.setup(ctx, NV, 0xDE6E).serialize_uncompressed(), NV)
    out = {"g1": [g1[96 * i:96 * (i + 1)] for i in range(1 << NV)], "g2": [g2[192 * i:192 * (i + 1)] for i in range(1 << NV)]}
    assert all(INF[c] not in out[c] for c in out)
    return out


def _msm(spx, ctx, oc, curve, pts, scalars):
    b, sc, n = b"".join(pts), wc.fr(scalars), len(pts)
    assert len(b) == SIZE[curve] * n and len(scalars) == n
    if curve == "g1":
        return spx.msm_g1(ctx, b, sc), oc.msm_g1(b, sc, n)
    return spx.msm_g2(ctx, b, sc), oc.msm_g2(b, sc, n)


def _with_inf(fin, curve, n, infinite):
    return [INF[curve] if i in infinite else fin[i] for i in range(n)]


# name -> (indices of the infinite bases, scalars) for n bases; rs: the case's own generator
def _one(at):
    return lambda n, rs: ({at(n)}, [rs.randrange(1, R) for _ in range(n)])


PATTERNS = {
    "first infinite": _one(lambda n: 0),
    "last infinite": _one(lambda n: n - 1),
    "middle infinite": _one(lambda n: n // 2),
    "all but one infinite": lambda n, rs: (set(range(n)) - {n // 3}, [rs.randrange(1, R) for _ in range(n)]),
    # finite and infinite references meet in the same wave at the same loop step; for G2 some lane pairs
    # of a wave skip while others add
    "every third infinite": lambda n, rs: (set(range(0, n, 3)), [rs.randrange(R) for _ in range(n)]),
    "all infinite": lambda n, rs: (set(range(n)), [rs.randrange(1, R) for _ in range(n)]),
    "finite x 0, infinite x nonzero": lambda n, rs: (set(range(1, n, 3)),
                                                     [rs.randrange(1, R) if i % 3 == 1 else 0 for i in range(n)]),
}
RESULT_IS_INFINITY = ("all infinite", "finite x 0, infinite x nonzero")


@pytest.mark.parametrize("curve", ["g1", "g2"])
def test_single_infinite_base(spx, ctx, oc, curve):
    """n = 1: an infinite base with a nonzero scalar"""
    for s in (1, R - 1, wc.FIXED):
        got, want = _msm(spx, ctx, oc, curve, [INF[curve]], [s])
        assert want == INF[curve] and got == want


@pytest.mark.parametrize("pattern", list(PATTERNS))
@pytest.mark.parametrize("n", [2, 64, 65, 256])
@pytest.mark.parametrize("curve", ["g1", "g2"])
def test_infinite_bases(spx, ctx, oc, bases, curve, n, pattern):
    infinite, scalars = PATTERNS[pattern](n, random.Random(1000 * n + len(pattern)))
    assert infinite and all(0 <= i < n for i in infinite)
    assert all(scalars[i] for i in infinite)  # no infinite base is dropped for a zero scalar
    got, want = _msm(spx, ctx, oc, curve, _with_inf(bases[curve], curve, n, infinite), scalars)
    if pattern in RESULT_IS_INFINITY:
        assert want == INF[curve]
    else:
        assert want != INF[curve]
    assert got == want


@pytest.mark.parametrize("finite", ["all but 200..391", "3 of 1024"])
@pytest.mark.parametrize("curve", ["g1", "g2"])
def test_infinite_partials_reach_the_hot_bucket_reduction(spx, ctx, oc, bases, curve, finite):
    """n = 1024, one scalar n times: every window's references pile into one bucket, which the planned
    partial levels leave hot. A run of 192 infinite bases (where a bucket keeps its references in base
    order, whole first-level segments of at most 64 references are infinite), and 3 finite bases among
    1021 infinite ones (whatever the order, at most 3 of a bucket's partials of any level are finite):
    all-infinite partials enter k_accum_xyzz, k_accum_hot and the weighting leaf"""
    n = 1 << NV
    infinite = set(range(200, 392)) if finite == "all but 200..391" else set(range(n)) - {5, 500, 1001}
    before = ctx.msm_skew_stats()
    got, want = _msm(spx, ctx, oc, curve, _with_inf(bases[curve], curve, n, infinite), [wc.FIXED] * n)
    st = ctx.msm_skew_stats()
    assert want != INF[curve] and got == want
    assert st[1] > before[1] and st[2] > before[2], "no hot bucket was reduced: %r -> %r" % (before, st)
