"""The MSM bucket weighting (k_tree_chunk, k_tree_level, k_tree_top: per-level sums of right children,
combined at the root) through spx_msm_g1 / spx_msm_g2 and whole proofs, byte for byte against the
oracle: scalars that fill one bucket, the first, the last, none, or meet P + P and P + (-P) above the
buckets, at 2^2 .. 2^9 buckets; the full-depth tree of the wide plan (2^16 buckets) in a child process;
the mixed batches of an opening; and the ranks' shares of split instances.
tests/test_weighting_cases.py checks the same schedule's slot arithmetic without a GPU."""
import os
import random
import subprocess
import sys
import threading

import pytest

from test_gpu_parity import R, _pp_bases

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
LOG_V = 3


def _fr(values):
    return b"".join(int(x).to_bytes(32, "little") for x in values)


def _every_digit(c, d):
    """the scalar whose c-bit windows below bit 252 all hold d (d <= 2^(c-1): the signed digits are d too)"""
    return sum(d << (c * w) for w in range(252 // c))


@pytest.fixture(scope="module")
def bases(oc):
    return _pp_bases(oc, 12, 0x3E0)


def _cases(n, c, seed):
    """(name, base pattern, scalars): pattern None = the n distinct bases, "same" = the first one n times"""
    rs = random.Random(seed)
    lb = c - 1
    m = 1 << min(lb - 1, 2)  # buckets per chunk of the weighting leaf
    s = rs.randrange(R)
    return [
        ("random", None, [rs.randrange(R) for _ in range(n)]),
        ("all equal", None, [s] * n),
        ("every digit 1: the first bucket", None, [_every_digit(c, 1)] * n),
        ("every digit 2^(c-1): the last bucket", None, [_every_digit(c, 1 << (c - 1))] * n),
        ("digits 1 and 2^(c-1): weights 1 and 2^lb", None, [_every_digit(c, 1 if i % 2 else 1 << (c - 1)) for i in range(n)]),
        ("all zero", None, [0] * n),
        ("one base, equal scalars", "same", [s] * n),
        ("one base, negated scalars", "same", [s if i % 2 else R - s for i in range(n)]),
        # buckets 0 and m (the first of chunks 0 and 1) hold the same point: P + P in the first level above the leaf
        ("one base in two chunks", "same", [1 if i % 2 else m + 1 for i in range(n)]),
    ]


@pytest.mark.parametrize("lg", [4, 6, 9, 12])
def test_msm_scalars(spx, ctx, oc, bases, lg):
    n = 1 << lg
    c, _ = spx.msm_window_plan(n)
    assert 3 <= c <= 10
    fails = []
    for name, pattern, sc in _cases(n, c, 40 + lg):
        scb = _fr(sc)
        for curve, b, w, mine, theirs in (("g1", bases[0], 96, spx.msm_g1, oc.msm_g1), ("g2", bases[1], 192, spx.msm_g2, oc.msm_g2)):
            bb = b[:w] * n if pattern == "same" else b[: w * n]
            got, want = mine(ctx, bb, scb), theirs(bb, scb, n)
            if got != want:
                fails.append((name, curve))
            if name in ("all zero", "one base, negated scalars") and want != theirs(bb, _fr([0] * n), n):
                fails.append((name, curve, "the case does not sum to infinity"))
    assert not fails, fails


def test_wide_plan_full_depth_tree():
    """2^10 points under the wide plan: c = 17, 2^16 buckets (14 levels above the leaf), mostly empty"""
    e = dict(os.environ)
    for k in ("SPX_SORT_FORM", "SPX_MSM_CAP_SCALE"):
        e.pop(k, None)
    e["SPX_MSM_WIDE_MIN_LOG"] = "8"
    r = subprocess.run([sys.executable, "-u", os.path.join(HERE, "weighting_wide_check.py")], env=e, timeout=120,
                       capture_output=True, text=True)
    print(r.stdout)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "all equal" in r.stdout


@pytest.fixture(scope="module")
def proof10(oc):
    inst = oc.Instance(0, 10, LOG_V, 0x3E2)
    ppb = oc.PP.keygen(10, 0x3E3).serialize()
    return inst, ppb, oc.prove(inst.mats, inst.v_bytes, inst.w_bytes, oc.PP.load(ppb), 0, 0)


def _prove(spx, c, inst, ppb):
    pp = spx.PublicParameter.load(c, ppb)
    pk = spx.MLArgumentForR1CS.index(c, *[spx.Csr(M.n, M.row_ptr, M.col, M.val) for M in inst.mats])
    return spx.MLArgumentForR1CS.prove(pk, inst.v_bytes, inst.w_bytes, pp)


def test_proofs_mixed_batches(spx, ctx, oc, proof10):
    """an opening's MSMs run as one batch of instances with different bucket counts (levels of 2^(nv-1)
    down to 1 points): narrower instances run the widest one's levels with sums that have no partner"""
    inst, ppb, want = proof10
    assert _prove(spx, ctx, inst, ppb) == want
    inst = oc.Instance(0, 12, LOG_V, 0x3E4)
    ppb = oc.PP.keygen(12, 0x3E5).serialize()
    assert _prove(spx, ctx, inst, ppb) == oc.prove(inst.mats, inst.v_bytes, inst.w_bytes, oc.PP.load(ppb), 0, 0)


@pytest.mark.parametrize("G", [2, 4])
def test_sharded_shares(spx, proof10, G):
    """G in-process ranks: every split instance's rank computes G F - (G - 1 - sel) S, sel != 0 among them"""
    inst, ppb, want = proof10
    group = spx.CommGroup(G)
    out, errs = [None] * G, []

    def run(r):
        try:
            c = spx.Context(0)
            c.set_comm_group(group, r)
            out[r] = _prove(spx, c, inst, ppb)
        except Exception as e:  # surfaced below
            errs.append(repr(e))

    ths = [threading.Thread(target=run, args=(r,)) for r in range(G)]
    for t in ths:
        t.start()
    for t in ths:
        t.join(timeout=120)
    assert not errs, errs
    for r in range(G):
        assert out[r] == want, "rank %d proof differs" % r
