"""The bucket weighting's schedule (tests/weighting_cases.py: the kernels' slot arithmetic over a toy
additive group) against sum_u (u + 1) X_u and against the (F, S, D) recurrence it replaces: every lb
from 1 to 10, batches whose instances have fewer chunks than the widest, every rank of G = 1, 2, 4, 8,
empty buckets, and hand-over levels other than the shipped one (a small top buffer, so the launched
levels run many rounds)."""
import random

import pytest

import weighting_cases as wc

P = wc.P61


def _buckets(lb, seed, empty=0.0):
    rs = random.Random(seed)
    return [0 if rs.random() < empty else rs.randrange(1, P) for _ in range(1 << lb)]


def _share(X, lg, sel):
    """sum_k (sel + G k + 1) X_k over a rank's local buckets"""
    G = 1 << lg
    return sum((sel + G * k + 1) * x for k, x in enumerate(X)) % P


# (top nodes, top elements): the shipped sizes; a top kernel of 2 nodes (launched levels nearly to the
# root); one that takes every level itself
TOPS = [(wc.K_TOP_NODES, wc.K_TOP_ELEMS), (2, 16), (1024, 8192)]


@pytest.mark.parametrize("tops", TOPS)
@pytest.mark.parametrize("lb", range(1, 11))
def test_single_instance(lb, tops):
    for empty in (0.0, 0.7, 1.0):
        X = _buckets(lb, 100 * lb + int(10 * empty), empty)
        (got,), (adds,) = wc.run_batch([(X, 0, 0)], *tops)
        assert got == wc.direct(X)
        f, s = wc.parent_tree(X, wc.chunk_log(lb))
        assert got == f and s == sum(X) % P
        # 2 additions per bucket in the leaf; above it 3 per chunk: the S-tree, the U_l and F0
        assert adds <= 2 * len(X) + 3 * (len(X) >> wc.chunk_log(lb))


@pytest.mark.parametrize("tops", TOPS)
@pytest.mark.parametrize("lbs", [(10, 1), (10, 3, 9, 2), (1, 10, 5), (7, 7, 4), (2, 1), (10, 8, 6, 4, 2, 1, 3, 5, 7, 9)])
def test_batch_with_narrower_instances(lbs, tops):
    """instances with fewer chunks than the batch's widest run its levels with sums that have no partner"""
    insts = [(_buckets(lb, 7 * i + lb, 0.3), 0, 0) for i, lb in enumerate(lbs)]
    got, _ = wc.run_batch(insts, *tops)
    assert got == [wc.direct(X) for X, _, _ in insts]


@pytest.mark.parametrize("tops", TOPS)
@pytest.mark.parametrize("lg", [0, 1, 2, 3])
@pytest.mark.parametrize("lb", range(1, 11))
def test_rank_shares(lb, lg, tops):
    """every rank's share G F - (G - 1 - sel) S of an instance of 2^(lb + lg) buckets dealt round-robin,
    and their sum: the whole instance's value"""
    G = 1 << lg
    full = _buckets(lb + lg, 31 * lb + lg, 0.2)
    insts = [(full[sel::G], lg, sel) for sel in range(G)]
    got, _ = wc.run_batch(insts, *tops)
    for sel in range(G):
        assert got[sel] == _share(full[sel::G], lg, sel)
        f, s = wc.parent_tree(full[sel::G], wc.chunk_log(lb))
        assert got[sel] == (G * f - (G - 1 - sel) * s) % P
    assert sum(got) % P == wc.direct(full)


def test_split_and_whole_instances_in_one_batch():
    full = _buckets(9, 5)
    insts = [(full[1::4], 2, 1), (_buckets(10, 6), 0, 0), (_buckets(1, 7), 0, 0), (full[3::4], 2, 3)]
    got, _ = wc.run_batch(insts)
    assert got == [_share(full[1::4], 2, 1), wc.direct(insts[1][0]), wc.direct(insts[2][0]), _share(full[3::4], 2, 3)]


def test_hand_over_of_the_wide_plan():
    """2^16 buckets (c = 17): handed over at 32 nodes after 9 launched levels, 192 slots exactly"""
    assert wc.top_from(1 << 14, 14) == 10
    assert 32 + 10 * 16 == wc.K_TOP_ELEMS
    # c = 24, the widest the library takes: 2^23 buckets, 21 levels
    lv = wc.top_from(1 << 21, 21)
    n = (1 << 21) >> (lv - 1)
    assert n + lv * max(1, n // 2) <= wc.K_TOP_ELEMS and n >= 8
