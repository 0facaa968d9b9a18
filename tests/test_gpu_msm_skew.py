"""Skewed scalars (0 / 1 witnesses): the MSM's hot-bucket reduction (k_accum_hot, msm_impl.hpp) and the
wave-aggregated counting of the bucket sort, at n = 2^14, the smallest size that uses c = 16, 16 windows
and the Keys16 path. There the affine level takes 8 references per thread and two XYZZ levels of
kSeg = 4 are planned, so a bucket of more than 512 references is hot; all ones leaves 128 partials to
the weighting leaf with the reduction off. Every result is byte-equal to the C oracle's; the public
parameter comes from the GPU keygen (the oracle's takes ~10 s at this size)."""
import ctypes
import os
import random
import subprocess
import sys
import threading

import numpy as np
import pytest

import msm_skew_check as sk
from msm_skew_check import K_SEG, LOG_N, N, R

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
LOG_V = 3


class Env:
    pass


@pytest.fixture(scope="module")
def env(spx, ctx, oc):
    """public parameter (GPU keygen, loaded into the oracle), its level-0 bases, the booleanity circuit
    at 2^14 with a seeded 0 / 1 witness, and the oracle's proof of it (computed once: ~9 s)"""
    e = Env()
    pp = spx.MLProofForR1CS.setup(ctx, LOG_N, sk.PP_SEED)
    e.ppb = pp.serialize_uncompressed()
    e.vp = spx.verifier_parameter(pp)
    del pp  # only bytes stay in the fixture: no library handle lives as long as the module
    e.ppc = oc.PP.load(e.ppb)
    e.g1, e.g2 = sk.pp_bases(e.ppb, LOG_N)
    # A = B = C = identity: row i is z_i * z_i = z_i, satisfied by every 0 / 1 assignment
    rp = (ctypes.c_uint64 * (N + 1)).from_buffer_copy(np.arange(N + 1, dtype=np.uint64).tobytes())
    col = (ctypes.c_uint32 * N).from_buffer_copy(np.arange(N, dtype=np.uint32).tobytes())
    val = sk.fr([1]) * N
    e.omats = [oc.CsrMatrix(N, rp, col, val) for _ in range(3)]
    e.mats = [spx.Csr(N, rp, col, val) for _ in range(3)]
    rs = random.Random(77)
    z = [1] + [rs.getrandbits(1) for _ in range(N - 1)]
    e.v, e.w = sk.fr(z[: 1 << LOG_V]), sk.fr(z[1 << LOG_V :])
    e.want = oc.prove(e.omats, e.v, e.w, e.ppc, 0, 0)
    return e


@pytest.fixture
def fresh(spx):
    """contexts of this test's own (the skew statistics are cumulative per context)"""
    made = []

    def make(hot=None):
        c = spx.Context(0)
        made.append(c)  # before anything can raise: a failing test leaves no context open at exit
        if hot is not None:
            c.set_msm_hot(hot)
        return c

    yield make
    for c in made:
        c.close()


def _msm(spx, oc, env, group, c, scalars, bases=None):
    if group == "g1":
        b = env.g1 if bases is None else bases
        return spx.msm_g1(c, b, scalars), oc.msm_g1(b, scalars, N)
    b = env.g2 if bases is None else bases
    return spx.msm_g2(c, b, scalars), oc.msm_g2(b, scalars, N)


GROUPS = ["g1", "g2"]


@pytest.mark.parametrize("group", GROUPS)
def test_all_ones(spx, oc, env, fresh, group):
    """case 1: every reference in bucket 0. On: reduced, at most kSeg partials at the leaf. Off: the same
    bytes, and the leaf adds more than kSeg (128 by the plan): the input does reach the leaf skewed."""
    sc = sk.all_ones()
    on, off = fresh(1), fresh(0)
    got, want = _msm(spx, oc, env, group, on, sc)
    st = on.msm_skew_stats()
    print("hot on ", st)
    assert got == want
    assert st[0] == 1 and st[1] == 1 and st[2] >= 1 and st[3] <= K_SEG
    got_off, _ = _msm(spx, oc, env, group, off, sc)
    st = off.msm_skew_stats()
    print("hot off", st)
    assert got_off == want
    assert st[1] == 1 and st[2] == 0 and st[3] > K_SEG


@pytest.mark.parametrize("group", GROUPS)
@pytest.mark.parametrize("shape", ["bits", "level0"])
def test_bits_and_level0_shape(spx, oc, env, fresh, group, shape):
    """case 2: seeded random bits, and seeded {0, 1, r - 1} (the shared level-0 opening's scalars)"""
    sc = sk.random_bits() if shape == "bits" else sk.level0_shape()
    c = fresh()
    got, want = _msm(spx, oc, env, group, c, sc)
    st = c.msm_skew_stats()
    print(st)
    assert got == want
    assert st[2] >= 1 and st[3] <= K_SEG


@pytest.mark.parametrize("group", GROUPS)
def test_half_repeated(spx, oc, env, fresh, group):
    """case 3: 16 hot buckets (one per window of the fixed scalar) inside ordinary bins"""
    sc = sk.half_repeated()
    c = fresh()
    got, want = _msm(spx, oc, env, group, c, sc)
    st = c.msm_skew_stats()
    print(st)
    assert got == want
    assert st[2] >= 16 and st[3] <= K_SEG


@pytest.mark.parametrize("group", GROUPS)
def test_four_hot_buckets_in_one_chunk(spx, oc, env, fresh, group):
    """case 4: scalars cycling 1, 2, 3, 4: the four buckets of one leaf chunk all hot"""
    c = fresh()
    got, want = _msm(spx, oc, env, group, c, sk.cycle_1234())
    st = c.msm_skew_stats()
    print(st)
    assert got == want
    assert st[2] == 4 and st[3] <= K_SEG


@pytest.mark.parametrize("group", GROUPS)
@pytest.mark.parametrize("scalars", ["ones", "one_and_minus_one"])
def test_one_base_repeated(spx, oc, env, fresh, group, scalars):
    """case 5: one base n times. All ones: equal partials meet in the hot tree (its doubling branch).
    1 and r - 1 alternating: the sum is (n / 2) r P, the identity."""
    w = 96 if group == "g1" else 192
    bases = (env.g1 if group == "g1" else env.g2)[5 * w : 6 * w] * N
    sc = sk.all_ones() if scalars == "ones" else sk.fr([1, R - 1]) * (N // 2)
    c = fresh()
    got, want = _msm(spx, oc, env, group, c, sc, bases)
    st = c.msm_skew_stats()
    print(st)
    assert got == want
    assert st[2] >= 1 and st[3] <= K_SEG


@pytest.mark.parametrize("group", GROUPS)
def test_uniform_scalars_take_no_hot_path(spx, oc, env, fresh, group):
    """case 6: uniform random scalars: no bucket near the threshold (mean 8), no hot bucket"""
    sc = sk.uniform()
    most = max(sk.bucket_counts(sc).values())
    print("largest bucket", most)
    assert most < 128
    c = fresh()
    got, want = _msm(spx, oc, env, group, c, sc)
    st = c.msm_skew_stats()
    print(st)
    assert got == want
    assert st[0] == 1 and st[1] == 0 and st[2] == 0


def test_full_proof_bits_witness(spx, ctx, oc, env, fresh):
    """case 7: the booleanity circuit with a 0 / 1 witness: prove is byte-equal to the oracle's, hot
    buckets were reduced, the proof verifies; prove_many over three contexts, one with the reduction off"""
    c = fresh(1)
    pp = pk = wit = None
    try:
        pp = spx.PublicParameter.load(c, env.ppb)
        pk = spx.MLArgumentForR1CS.index(c, *env.mats)
        got = spx.MLArgumentForR1CS.prove(pk, env.v, env.w, pp)
        st = c.msm_skew_stats()
        print(st)
        assert got == env.want
        assert st[1] >= 1 and st[2] >= 1 and st[3] <= K_SEG
        assert spx.MLArgumentForR1CS.verify(pk, env.v, got, env.vp)
        ctxs = [c, fresh(1), fresh(0)]
        wit = spx.Witness(c, env.v, env.w)
        many = spx.MLArgumentForR1CS.prove_many(ctxs, pk, [wit] * 6, pp)
        assert len(many) == 6
        for p in many:
            assert p == env.want
        print("hot off", ctxs[2].msm_skew_stats())
        assert ctxs[2].msm_skew_stats()[2] == 0
    finally:  # handles of a context go before the context does, also when an assertion fails
        del wit, pk, pp


@pytest.mark.parametrize("G", [2, 4])
def test_virtual_ranks(spx, oc, env, G):
    """case 8: the same instance proof-sharded over G virtual ranks (split instances, I.lg != 0): every
    rank's proof is the oracle's, and the rank that owns bucket 0 reduced it"""
    group = spx.CommGroup(G)
    out, stats, errs = [None] * G, [None] * G, []

    def run(r):
        try:
            c = spx.Context(0)
            c.set_comm_group(group, r)
            pp = spx.PublicParameter.load(c, env.ppb)
            pk = spx.MLArgumentForR1CS.index(c, *env.mats)
            out[r] = spx.MLArgumentForR1CS.prove(pk, env.v, env.w, pp)
            stats[r] = c.msm_skew_stats() + (c.msm_reruns(),)
        except Exception as e:
            errs.append(repr(e))

    ths = [threading.Thread(target=run, args=(r,)) for r in range(G)]
    for t in ths:
        t.start()
    for t in ths:
        t.join(timeout=120)
    print(stats)
    assert not errs, errs
    for r in range(G):
        assert out[r] == env.want, "rank %d" % r
        assert stats[r][3] <= K_SEG
    assert sum(s[2] for s in stats) >= 1


@pytest.mark.parametrize("form", ["staged", "direct"])
def test_forced_sort_forms(form):
    """case 9: cases 1-3 under each forced form of the bucket sort, at c = 16 (tests/msm_skew_check.py)"""
    env_ = dict(os.environ, SPX_SORT_FORM=form)
    r = subprocess.run([sys.executable, "-u", os.path.join(HERE, "msm_skew_check.py")], env=env_, timeout=120,
                       capture_output=True, text=True)
    print(r.stdout)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
