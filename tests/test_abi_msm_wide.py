"""The MSM window plan through the C ABI (no GPU): window bits and windows on each side of the wide
threshold, SPX_MSM_WIDE_MIN_LOG, and the fallback to c = 16 where another wide level would take an
opening batch past the sort's bucket limit."""
import pytest

MAX_BUCKETS = 1 << 19  # kMsmMaxBuckets (kernels.hpp)


@pytest.fixture
def plan(spx, monkeypatch):
    spx.lib()
    monkeypatch.delenv("SPX_MSM_WIDE_MIN_LOG", raising=False)
    return spx


def test_default_threshold(plan):
    assert plan.msm_window_plan(1 << 18) == (17, 15)
    assert plan.msm_window_plan(1 << 20) == (17, 15)
    assert plan.msm_window_plan((1 << 18) - 1) == (16, 16)
    assert plan.msm_window_plan(1 << 14) == (16, 16)
    assert plan.msm_window_plan(1 << 13) == (11, 24)
    assert plan.msm_window_plan(1 << 5) == (3, 86)


@pytest.mark.parametrize("setting,first_wide", [("17", 17), ("19", 19), ("10", 10), ("3", 8), ("0", None)])
def test_setting(plan, monkeypatch, setting, first_wide):
    monkeypatch.setenv("SPX_MSM_WIDE_MIN_LOG", setting)
    for k in range(5, 27):
        c, w = plan.msm_window_plan(1 << k)
        if first_wide is not None and k >= first_wide:
            assert (c, w) == (17, 15)
        else:
            assert c == (16 if k >= 14 else max(3, k - 2)) and w == -(-256 // c)


@pytest.mark.parametrize("setting", [None, "8", "14", "0"])
@pytest.mark.parametrize("nv", [12, 20, 24, 25, 26])
def test_level_plan_fits_the_bucket_limit(plan, monkeypatch, nv, setting):
    """the largest levels go wide first; the rest of the candidates keep 16 bits once the batch of all
    levels would pass the limit (at 2^24 with the default threshold: level 0 .. 4 wide, the 2^18-point
    level 5 at 16 bits, since level 0 may run inside the first opening's batch)"""
    if setting is not None:
        monkeypatch.setenv("SPX_MSM_WIDE_MIN_LOG", setting)
    wide_min = 18 if setting is None else int(setting)
    c = plan.msm_level_plan(nv)
    assert len(c) == nv
    assert sum(1 << (x - 1) for x in c) <= MAX_BUCKETS
    cand = [i for i in range(nv) if wide_min and nv - i - 1 >= wide_min]
    wide = [i for i in range(nv) if c[i] == 17]
    assert wide == cand[: len(wide)]  # a prefix of the candidates: the largest levels
    for i in range(nv):
        if c[i] != 17:
            k = nv - i - 1
            assert c[i] == (16 if k >= 14 else max(3, k - 2))
    if len(wide) < len(cand):  # one more wide level would not have fitted
        nxt = cand[len(wide)]
        assert sum(1 << (x - 1) for x in c) - (1 << (c[nxt] - 1)) + (1 << 16) > MAX_BUCKETS
    if setting is None and nv <= 20:
        assert wide == cand
