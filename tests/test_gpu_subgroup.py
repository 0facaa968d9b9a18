"""The subgroup membership kernels ("Subgroup membership") through spx_g1_in_subgroup /
spx_g2_in_subgroup against the oracle's [r] P = O: the lane, wave and block edges with the classes of
subgroup_cases.py interleaved so that neighbouring lanes differ in outcome, one array longer than a
launch's grid, and the counters."""
import pytest

import subgroup_cases as sc

pytestmark = pytest.mark.gpu


def _fn(spx, cid):
    return spx.g1_in_subgroup if cid == 1 else spx.g2_in_subgroup


@pytest.mark.parametrize("cid", [1, 2])
def test_every_class_alone(spx, ctx, cid):
    cs = sc.cases(cid)
    got = _fn(spx, cid)(ctx, b"".join(c[1] for c in cs))
    assert [(c[0], g) for c, g in zip(cs, got)] == [(c[0], c[2]) for c in cs]


@pytest.mark.parametrize("cid", [1, 2])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_edges_with_interleaved_classes(spx, ctx, cid, n):
    pts, want = sc.interleaved(cid, n)
    assert n < 2 or want[0] != want[1]  # neighbours diverge
    before = ctx.subgroup_stats()
    got = _fn(spx, cid)(ctx, pts)
    after = ctx.subgroup_stats()
    assert got == want
    assert (after[0] - before[0], after[1] - before[1], after[2] - before[2]) == (n, 0, want.count(False))


@pytest.mark.parametrize("cid", [1, 2])
def test_second_pass_of_the_grid_stride_loop(spx, ctx, cid):
    """one point more than a launch's lanes: the first lane takes a second point. The array repeats a
    257-point pattern, which does not divide the grid, so a lane's two points differ."""
    n = spx.SUBGROUP_GRID_POINTS + 1
    pts, want = sc.interleaved(cid, 257)
    reps = n // 257 + 1
    got = _fn(spx, cid)(ctx, (pts * reps)[: n * sc.CURVES[cid][3]])
    assert got == (want * reps)[:n]


def test_argument_errors(spx, ctx):
    with pytest.raises(spx.InvalidArgument):
        spx.g1_in_subgroup(ctx, bytes(95))
    with pytest.raises(spx.InvalidArgument):
        spx.g2_in_subgroup(ctx, b"")
    import ctypes

    ok = ctypes.create_string_buffer(1)
    assert spx.lib().spx_g1_in_subgroup(ctx.h, None, 1, ok) == 1
    assert spx.lib().spx_g1_in_subgroup(ctx.h, bytes(96), 0, ok) == 1
