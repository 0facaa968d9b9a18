"""spx_pp_check_structure and spx_pp_derive_vp on the GPU ("Public-parameter structure and
views"), against the oracle fixtures of tests/pp_structure_cases.py (whose identities
tests/test_pp_structure_refs.py asserts on the CPU).

Stage 1 (k_fold_check, one pair of points per lane) must accept well-formed parameters, among them the
degenerate one whose pairs are equal points, infinite + finite, finite + infinite, both infinite and two
different finite points, and must name exactly the pairs a replaced point breaks. Stage 2 (an opening
self-test under the derived verifier parameter) must catch what keeps every pair sum: two swapped points
of a pair. The derived verifier parameter (k_odd_sum) must equal the trapdoor's g^{t_i} byte for byte."""
import random

import pytest

import pp_structure_cases as cases
import spartan

pytestmark = pytest.mark.gpu

R = spartan.R
# k_fold_check runs blocks of 64 lanes (kPPFoldLanes), k_odd_sum blocks of 256 (kPPSumThreads): nv = 10 has
# 1023 pairs (16 blocks) and 512 odd points in level 0 (2 blocks), nv = 11 twice that
FOLD_LANES, SUM_THREADS = 64, 256
GEN_SEED = 0x57C7
ENTROPIES = (None, bytes(range(32)), bytes(range(100, 132)))


@pytest.fixture(scope="module")
def gen10(spx, ctx):
    pp = spx.MLProofForR1CS.setup(ctx, 10, GEN_SEED)
    return pp, pp.serialize_uncompressed()


# ------------------------------------------------------------------ accepts
@pytest.mark.parametrize("which", ["random", "degenerate"])
def test_accepts_loaded(spx, ctx, which):
    fx = cases.random_pp() if which == "random" else cases.degenerate()
    pp = spx.PublicParameter.load(ctx, fx.bytes)
    for e in ENTROPIES:
        assert pp.check_structure(entropy=e) == (0, None, 1)
    assert pp.check_structure(strict=False) == (0, None, 1)
    assert spx.PublicParameter.load(ctx, fx.bytes, check_structure=True).nv == fx.nv


@pytest.mark.parametrize("nv", [1, 10, 11])
def test_accepts_generated(spx, ctx, nv):
    if nv >= 10:  # more pairs, and more odd points in level 0, than one workgroup
        assert (1 << nv) - 1 > FOLD_LANES and 1 << (nv - 1) > SUM_THREADS
    pp =spx.MLProofForR1CS.setup(ctx, nv, GEN_SEED + nv)
    assert pp.check_structure() == (0, None, 1)


# ------------------------------------------------------------------ locates
def _other(b, nv, curve, level, index):
    """another valid point of the same parameter: the one at the mirrored index of the level (index 0 and
    1 of the last level map to each other)"""
    n = 1 << (nv - level)
    return cases.get_point(b, nv, curve, level, n - 1 - index)


LOCATE = {
    "G1 level 0 index 0": [(1, 0, 0)],
    "G1 level 0 last index": [(1, 0, (1 << 10) - 1)],
    "G1 last level index 1": [(1, 9, 1)],
    "G2 level 3 middle index": [(2, 3, 37)],
    "one point on each curve": [(2, 1, 200), (1, 4, 9)],
}


@pytest.mark.parametrize("name", list(LOCATE))
def test_locates_replaced_points(spx, ctx, gen10, name):
    _, b = gen10
    nv = 10
    want = []
    bad_bytes = b
    for curve, level, index in LOCATE[name]:
        bad_bytes = cases.replace_point(bad_bytes, nv, curve, level, index, _other(b, nv, curve, level, index))
        want += cases.expected_failures(nv, curve, level, index)
    want.sort()
    pp = spx.PublicParameter.load(ctx, bad_bytes)
    bad, first, opening_ok = pp.check_structure(strict=False)
    assert (bad, first, opening_ok) == (len(want), want[0], -1)
    with pytest.raises(spx.SerializationError) as ei:
        pp.check_structure()
    c, lvl, pair = want[0]
    msg = str(ei.value)
    assert msg.startswith("%s level %d pair %d: points %d + %d != " % ("powers_of_g" if c == 1 else "powers_of_h", lvl, pair,
                                                                      2 * pair, 2 * pair + 1)), msg
    assert ("level %d point %d" % (lvl + 1, pair) if lvl + 1 < nv else " != g ") in msg
    assert msg.endswith("(%d such pair%s)" % (len(want), "" if len(want) == 1 else "s")), msg
    with pytest.raises(spx.SerializationError):
        spx.PublicParameter.load(ctx, bad_bytes, check_structure=True)


def test_locates_replaced_g(spx, ctx, gen10):
    _, b = gen10
    pp = spx.PublicParameter.load(ctx, cases.replace_g(b, 10, cases.get_point(b, 10, 1, 5, 3)))
    assert pp.check_structure(strict=False) == (1, (1, 9, 0), -1)
    with pytest.raises(spx.SerializationError, match=r"powers_of_g level 9 pair 0: points 0 \+ 1 != g \(1 such pair\)"):
        pp.check_structure()


# ------------------------------------------------------------------ stage 2
def test_swapped_pair_fails_the_opening_only(spx, ctx):
    fx = cases.random_pp()
    swapped = cases.swap_points(fx.bytes, fx.nv, 1, 0, 0, 1)
    assert cases.fold_failures(spartan.PublicParameter.deserialize_uncompressed(swapped)) == []
    pp = spx.PublicParameter.load(ctx, swapped)
    good = spx.PublicParameter.load(ctx, fx.bytes)
    for e in ENTROPIES:
        assert pp.check_structure(entropy=e, strict=False) == (0, None, 0)
        with pytest.raises(spx.SerializationError, match="opening self-test failed"):
            pp.check_structure(entropy=e)
        assert good.check_structure(entropy=e, strict=False) == (0, None, 1)


# ------------------------------------------------------------------ derived verifier parameter
@pytest.mark.parametrize("nv", [1, 6, 10, 11])
def test_derive_vp_generated(spx, ctx, nv):
    pp = spx.MLProofForR1CS.setup(ctx, nv, GEN_SEED + nv)
    assert pp.derive_vp() == spx.verifier_parameter(pp)


@pytest.mark.parametrize("which", ["random", "degenerate"])
def test_derive_vp_loaded(spx, ctx, which):
    fx = cases.random_pp() if which == "random" else cases.degenerate()
    if which == "degenerate":
        assert fx.vp.g_mask_random[1] is None  # t_1 = 0: every odd point of level 1 is infinite
        assert fx.pp.powers_of_g[4][1] == fx.pp.powers_of_g[4][3]  # t_5 = 1/2: equal summands (doubling)
    pp = spx.PublicParameter.load(ctx, fx.bytes)
    with pytest.raises(spx.InvalidArgument, match="trapdoor unknown"):
        spx.verifier_parameter(pp)
    assert pp.derive_vp() == fx.vp_bytes


# ------------------------------------------------------------------ end to end
def test_proof_and_opening_verify_under_the_derived_vp(spx, ctx, oc):
    fx = cases.random_pp()
    pp = spx.PublicParameter.load(ctx, fx.bytes)
    vp = pp.derive_vp()
    inst = oc.Instance(0, fx.nv, 2, 0x5EED0004)
    pk = spx.MLArgumentForR1CS.index(ctx, *[spx.Csr(M.n, M.row_ptr, M.col, M.val) for M in inst.mats])
    proof = spx.MLArgumentForR1CS.prove(pk, inst.v_bytes, inst.w_bytes, pp)
    assert spx.MLArgumentForR1CS.verify(pk, inst.v_bytes, proof, vp) is True
    rs = random.Random(44)
    table = spx.fr_bytes([rs.randrange(R) for _ in range(1 << fx.nv)])
    point = spx.fr_bytes([rs.randrange(R) for _ in range(fx.nv)])
    com = spx.MLPolyCommit.commit(pp, table)
    value, opening = spx.MLPolyCommit.open(pp, table, point)
    assert spx.MLPolyCommit.verify(vp, com, point, value, opening) is True
    other = spx.fr_bytes([rs.randrange(R)])
    assert spx.MLPolyCommit.verify(vp, com, point, other, opening) is False
