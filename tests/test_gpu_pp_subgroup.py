"""spx_pp_check_subgroup ("Subgroup membership"): a generated public parameter passes; a
serialized one with a point swapped for a curve point outside the subgroup still loads through spx_pp_load,
as before, and the check names exactly that point."""
import ctypes

import pytest

import subgroup_cases as sc

pytestmark = pytest.mark.gpu

NV = 3
U64_MAX = 2**64 - 1


def _offsets(nv):
    """byte offsets of the points of a serialized PublicParameter: ({(curve, level): offset}, g, h)"""
    pos, lv = 16, {}
    for cid, ps in ((1, 96), (2, 192)):
        for i in range(nv):
            pos += 8
            lv[(cid, i)] = pos
            pos += ps << (nv - i)
        pos += 8 if cid == 1 else 0
    return lv, pos, pos + 96


def _outsider(cid, name):
    return next(c[1] for c in sc.cases(cid) if c[0] == name and not c[2])


def _swap(data, nv, where, cid_class):
    """data with the point at `where` = (curve, level, index), "g" or "h" replaced"""
    lv, g_at, h_at = _offsets(nv)
    cid = {"g": 1, "h": 2}.get(where) or where[0]
    ps = 96 * cid
    at = g_at if where == "g" else h_at if where == "h" else lv[(cid, where[1])] + ps * where[2]
    assert at + ps <= len(data)
    return data[:at] + _outsider(cid, cid_class) + data[at + ps :]


def _check(spx, ctx, pp):
    bad = ctypes.c_uint64(99)
    first = (ctypes.c_uint64 * 3)(7, 7, 7)
    rc = spx.lib().spx_pp_check_subgroup(ctx.h, pp.h, ctypes.byref(bad), first)
    return rc, bad.value, tuple(first), spx.lib().spx_last_error().decode()


@pytest.fixture(scope="module")
def pp_bytes(spx, ctx):
    pp = spx.MLProofForR1CS.setup(ctx, NV, 4242)
    data = pp.serialize_uncompressed()
    lv, g_at, h_at = _offsets(NV)
    assert h_at + 192 == len(data)
    return data


@pytest.mark.parametrize("nv", [3, 6])
def test_generated_pp_passes(spx, ctx, nv):
    pp = spx.MLProofForR1CS.setup(ctx, nv, 4242 + nv)
    before = ctx.subgroup_stats()
    rc, bad, first, _ = _check(spx, ctx, pp)
    after = ctx.subgroup_stats()
    assert (rc, bad) == (0, 0)
    assert pp.check_subgroup() == (0, None)
    npts = 2 * (2 ** (nv + 1) - 2)  # levels of 2^nv .. 2 points, both curves
    assert (after[0] - before[0], after[1] - before[1], after[2] - before[2]) == (npts, 2, 0)
    # NULL outputs are allowed
    assert spx.lib().spx_pp_check_subgroup(ctx.h, pp.h, None, None) == 0


SWAPS = [
    ((1, 0, 5), "d multiple + torsion", (1, 0, 5), "powers_of_g level 0 index 5"),
    ((1, NV - 1, 1), "b random", (1, NV - 1, 1), "powers_of_g level %d index 1" % (NV - 1)),
    ((2, 1, 2), "d multiple + torsion", (2, 1, 2), "powers_of_h level 1 index 2"),
    ("g", "b random", (1, U64_MAX, 0), ": g "),
    ("h", "d multiple + torsion", (2, U64_MAX, 0), ": h "),
]


@pytest.mark.parametrize("where,cls,first,named", SWAPS, ids=[str(s[0]) for s in SWAPS])
def test_one_swapped_point(spx, ctx, pp_bytes, where, cls, first, named):
    data = _swap(pp_bytes, NV, where, cls)
    pp = spx.PublicParameter.load(ctx, data)  # existing behaviour: on the curve is all spx_pp_load asks
    assert pp.serialize_uncompressed() == data
    rc, bad, got_first, msg = _check(spx, ctx, pp)
    assert (rc, bad, got_first) == (4, 1, first)  # SPX_SERIALIZATION
    assert "outside the prime-order subgroup" in msg and named in msg
    assert pp.check_subgroup(strict=False) == (1, (first[0], None if first[1] == U64_MAX else first[1], first[2]))
    with pytest.raises(spx.SerializationError, match="outside the prime-order subgroup"):
        spx.PublicParameter.load(ctx, data, check_subgroup=True)


def test_two_swapped_points(spx, ctx, pp_bytes):
    data = _swap(_swap(pp_bytes, NV, (2, 0, 7), "b random"), NV, (1, 1, 3), "b random")
    rc, bad, first, msg = _check(spx, ctx, spx.PublicParameter.load(ctx, data))
    assert (rc, bad, first) == (4, 2, (1, 1, 3)) and "2 such points" in msg
    # within one curve the lower level wins, then the lower index
    data = _swap(_swap(pp_bytes, NV, (2, 2, 0), "b random"), NV, (2, 0, 6), "d multiple + torsion")
    rc, bad, first, _ = _check(spx, ctx, spx.PublicParameter.load(ctx, data))
    assert (rc, bad, first) == (4, 2, (2, 0, 6))
    # g and h come after every level
    data = _swap(_swap(pp_bytes, NV, "h", "b random"), NV, "g", "b random")
    rc, bad, first, _ = _check(spx, ctx, spx.PublicParameter.load(ctx, data))
    assert (rc, bad, first) == (4, 2, (1, U64_MAX, 0))


def test_clean_bytes_pass_after_a_round_trip(spx, ctx, pp_bytes):
    assert spx.PublicParameter.load(ctx, pp_bytes, check_subgroup=True).check_subgroup() == (0, None)
