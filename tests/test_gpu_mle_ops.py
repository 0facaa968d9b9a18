"""The kernels and launchers of mle_kernels.hip, one family at a time, against the big-integer references of
tests/mle_cases.py, at the smallest shapes that reach each launch branch (the wave-transposed rounds,
fused and unfused reductions, stride loops, the wave opening fold, the tail, the lockstep groups).
tests/native/mle_ops.hip #includes the kernel file, so the kernels, launch constants and launchers are
the product's; the product library is not involved.

Every output is compared as exact Montgomery words with the reference. Output buffers arrive filled
with a pattern that must be intact wherever the kernel must not write (quotient levels switched off,
null outputs, partial slots beyond the grid, rows no entry names). A round is launched twice on the
same ticket and partials: both results must be the reference and the ticket must read 0 after each."""
import ctypes
import os
import random
import subprocess

import numpy as np
import pytest

import mle_cases as mc
import spartan
from mle_cases import R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SO = os.path.join(ROOT, "tests", "native", "libmle_ops.so")

c_int, c_u64, vp = ctypes.c_int, ctypes.c_uint64, ctypes.c_void_p


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(SO):  # a failing build fails the test; it never skips
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "r1cs-spartan_amd", "csrc"), "mlelib"])
    L = ctypes.CDLL(SO)
    sig = {
        "mle_round": [c_int] * 6 + [vp, c_u64, vp, c_u64, vp, c_u64, vp, c_u64, vp, c_u64, vp, c_u64, vp, vp],
        "mle_round_group": [c_int] * 4 + [vp, c_u64, vp, c_u64, vp, c_u64, vp, c_u64, vp, c_u64, vp, c_u64, vp, vp],
        "mle_reduce_partials": [vp, c_int, vp],
        "mle_eq_table": [c_int, vp, c_int, c_u64, c_u64, vp],
        "mle_eq_factors": [c_int, vp, vp, vp],
        "mle_eq_expand": [vp, vp, c_u64, c_int, c_u64, c_u64, c_int, vp],
        "mle_open_level": [c_int, c_int, vp, c_u64, vp, vp, vp],
        "mle_open_fold": [c_int, c_int, c_int, vp, c_u64, vp, vp, c_u64, vp, vp],
        "mle_open_tail": [vp, c_u64, c_int, vp, vp, c_u64, vp],
        "mle_open_tail_levels": [c_u64, c_int],
        "mle_open_eval_group": [c_int, vp, vp, c_int, vp],
        "mle_spmv": [c_int, vp, vp, vp, c_u64, vp, c_u64, vp, c_u64],
        "mle_spmv_group_direct": [c_int, c_int, vp, vp, vp, c_u64, vp, c_u64, vp, c_u64],
        "mle_round_plan": [c_int, c_int, c_int, c_int, c_u64, vp],
        "mle_open_eval_plan": [c_int, vp, c_int, vp],
        "mle_mont": [c_int, c_int, vp, c_u64, vp],
        "mle_copy_runs": [c_int, vp, c_int, c_int, vp],
    }
    for name, args in sig.items():
        f = getattr(L, name)
        f.restype, f.argtypes = c_int, args
    return L


def ptr(a):
    if a is None:
        return None
    assert a.flags["C_CONTIGUOUS"] and a.flags["WRITEABLE"]
    return a.ctypes.data


def call(L, name, *args):
    err = getattr(L, name)(*args)
    if err > 0:  # nothing more is launched on a device that reported an error
        pytest.exit("HIP error %d in %s" % (err, name), returncode=3)
    assert err == 0, "%s refused its arguments" % name


def same(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    if not np.array_equal(got, want):
        bad = np.nonzero((got != want).any(axis=-1))[0]
        raise AssertionError("%s: %d of %d entries differ, first at %d: got %s want %s" % (
            what, len(bad), len(got), bad[0], [hex(int(x)) for x in got[bad[0]]], [hex(int(x)) for x in want[bad[0]]]))


def intact(buf, what):
    assert (buf == mc.PATTERN).all(), "%s: written where nothing may be written" % what


# ------------------------------------------------------------------ rounds
def run_round(L, c, mode, need1, fused, grid, eout):
    """one round case through mle_round; `grid` / `fused` are what the launch uses (restated for mode 0)"""
    nout = 2 * c.half if c.fold else 0
    out = mc.pattern(c.ntab * nout) if c.fold else None
    want_eout = bool(eout and c.fold and c.which == 1)
    Eout = mc.pattern(c.half) if want_eout else None
    partial = mc.pattern(mc.ROUND_PARTIALS)
    ticket2 = np.full(2, 0xFFFFFFFF, dtype=np.uint32)
    res = mc.pattern(6)
    call(L, "mle_round", c.which, mode, c.fold, need1, fused, grid, ptr(c.tabs_w), c.nin, ptr(c.E_w), c.nE, ptr(c.r_w),
         c.half, ptr(out), nout, ptr(Eout), c.half if want_eout else 0, ptr(partial), mc.ROUND_PARTIALS, ptr(ticket2),
         ptr(res))
    want = c.sums_w.copy()
    if not need1:
        want[1] = 0  # G(1) / P(1) left to the host: the word is written, as zero
    same(res[:3], want, "result3 of the first launch")
    same(res[3:], want, "result3 of the second launch on the same ticket and partials")
    assert ticket2.tolist() == [0, 0], "ticket after the launches: %s" % ticket2.tolist()
    if c.fold:
        same(out, c.out_w, "folded tables")
    if want_eout:
        same(Eout, c.Eout_w, "Eout")
    intact(partial[3 * grid:], "partials beyond the grid of %d blocks" % grid)
    if fused and grid == 1:
        intact(partial, "partials of a one-block fused launch")


def _round_id(p):
    which, half, fold, need1, eout = p
    form, grid, fused = mc.round_dispatch(which, fold, need1, half)
    return "sc%d-half%d-fold%d-need%d-eout%d-%s-g%d-%s" % (which, half, fold, need1, eout, form, grid,
                                                          "fused" if fused else "reduce")


@pytest.mark.parametrize("p", mc.launcher_round_params(), ids=_round_id)
def test_round_launcher(lib, p):
    """launch_sc1_round / launch_sc2_round with their production dispatch"""
    which, half, fold, need1, eout = p
    _, grid, fused = mc.round_dispatch(which, fold, need1, half)
    run_round(lib, mc.round_case(which, half, fold), 0, need1, fused, grid, eout)


def _edge_id(p):
    which, half, fold, need1, kind = p
    return "sc%d-half%d-fold%d-need%d-%s-%s" % (which, half, fold, need1, kind, mc.round_dispatch(which, fold, need1, half)[0])


@pytest.mark.parametrize("p", mc.edge_round_params(), ids=_edge_id)
def test_round_value_edges(lib, p):
    """all-zero tables, every entry r - 1, E all zero, A B = C in every pair, challenges 0, 1, r - 1"""
    which, half, fold, need1, kind = p
    c = mc.round_case(which, half, fold, kind)
    if kind in ("zero", "abc", "ezero"):
        assert c.sums == [0, 0, 0]
    _, grid, fused = mc.round_dispatch(which, fold, need1, half)
    run_round(lib, c, 0, need1, fused, grid, 1)


@pytest.mark.parametrize("fused", [1, 0], ids=["fused", "reduce"])
@pytest.mark.parametrize("need1", [0, 1])
@pytest.mark.parametrize("fold", [0, 1])
@pytest.mark.parametrize("wg", mc.WAVE_DIRECT, ids=lambda wg: "w%d-g%d" % wg)
@pytest.mark.parametrize("which", [1, 2])
def test_round_wave_direct(lib, which, wg, fold, need1, fused):
    """k_sc1_wave / k_sc2_wave<FOLD, NEED1, FUSED> over 64 w pairs with a grid the test gives: idle waves
    in the reduction, the stride loop with a ragged last pass; unfused: summed by k_reduce_partials<3>"""
    w, grid = wg
    run_round(lib, mc.round_case(which, 64 * w, fold), 3, need1, fused, grid, 1)


@pytest.mark.parametrize("fused", [1, 0], ids=["fused", "reduce"])
@pytest.mark.parametrize("which", [1, 2])
def test_round_quad_pair_direct(lib, which, fused):
    """k_sc1_fold_quad / k_sc2_fold_pair with one block over 200 pairs: 4 / 2 passes, the last one partly filled"""
    run_round(lib, mc.round_case(which, 200, 1), 2, 0, fused, 1, 1)


@pytest.mark.parametrize("fused", [1, 0], ids=["fused", "reduce"])
@pytest.mark.parametrize("fold", [0, 1])
@pytest.mark.parametrize("which", [1, 2])
def test_round_lane_direct(lib, which, fold, fused):
    """k_sc1_round / k_sc2_round, both reductions (the launcher reaches the unfused one only from 2^14
    pairs on, where the wave form takes over), two blocks striding over 700 pairs"""
    run_round(lib, mc.round_case(which, 700, fold), 1, 1, fused, 2, 1)


@pytest.mark.parametrize("kind", ["rand", "rm1"])
@pytest.mark.parametrize("nblk", mc.REDUCE_NBLK)
def test_reduce_partials(lib, nblk, kind):
    """k_reduce_partials<3>: one block, its loop past 256 blocks, every partial r - 1"""
    rng = random.Random(nblk)
    vals = [R - 1] * (3 * nblk) if kind == "rm1" else [rng.randrange(R) for _ in range(3 * nblk)]
    want = [sum(vals[k::3]) % R for k in range(3)]
    part, out = mc.mont_words(vals), mc.pattern(3)
    call(lib, "mle_reduce_partials", ptr(part), nblk, ptr(out))
    same(out, mc.mont_words(want), "sums")


def _group_id(p):
    k, half, fold, need1 = p
    return "k%d-half%d-fold%d-need%d" % p


@pytest.mark.parametrize("p", mc.GROUP_ROUNDS, ids=_group_id)
@pytest.mark.parametrize("which", [1, 2])
def test_round_group(lib, which, p):
    """launch_sc1_round / launch_sc2_round with k jobs: distinct tables and challenges per job, every
    job's outputs equal the reference of its own tables"""
    k, half, fold, need1 = p
    form = mc.group_dispatch(which, fold, need1, half, k)
    _, grid, fused = mc.round_dispatch(which, fold, need1, half)
    jobs = [mc.build_round(which, half, fold, "rand", seed=100 + j) for j in range(k)]
    c0 = jobs[0]
    nout = 2 * half if fold else 0
    want_eout = bool(fold and which == 1)
    tabs = np.concatenate([c.tabs_w for c in jobs])
    E = np.concatenate([c.E_w for c in jobs]) if which == 1 else None
    r = np.concatenate([c.r_w for c in jobs])
    out = mc.pattern(k * c0.ntab * nout) if fold else None
    Eout = mc.pattern(k * half) if want_eout else None
    partial = mc.pattern(k * mc.ROUND_PARTIALS)
    ticket2 = np.full(2 * k, 0xFFFFFFFF, dtype=np.uint32)
    res = mc.pattern(2 * 3 * k)
    call(lib, "mle_round_group", which, k, fold, need1, ptr(tabs), c0.nin, ptr(E), c0.nE, ptr(r), half, ptr(out), nout,
         ptr(Eout), half if want_eout else 0, ptr(partial), mc.ROUND_PARTIALS, ptr(ticket2), ptr(res))
    assert (ticket2 == 0).all(), "tickets after the launches: %s" % ticket2.tolist()
    for j, c in enumerate(jobs):
        want = c.sums_w.copy()
        if not need1:
            want[1] = 0
        for rep in range(2):
            same(res[3 * (rep * k + j):][:3], want, "job %d (%s), launch %d: result3" % (j, form, rep))
        if fold:
            same(out[j * c.ntab * nout:][:c.ntab * nout], c.out_w, "job %d: folded tables" % j)
        if want_eout:
            same(Eout[j * half:][:half], c.Eout_w, "job %d: Eout" % j)
        intact(partial[j * mc.ROUND_PARTIALS + 3 * grid:][:mc.ROUND_PARTIALS - 3 * grid], "job %d: partials beyond the grid" % j)


# ------------------------------------------------------------------ eq tables
def run_eq_table(L, k, rs, nvar, base, count):
    kk = max(k, 1)
    r_w = mc.mont_words([v for r in rs for v in r]) if nvar else None
    out = mc.pattern(kk * count)
    call(L, "mle_eq_table", k, ptr(r_w), nvar, base, count, ptr(out))
    return out.reshape(kk, count, 8)


@pytest.mark.parametrize("kind", ["rand", "edges"])
@pytest.mark.parametrize("nvar", mc.EQ_FULL_NVAR)
def test_eq_table_full(lib, nvar, kind):
    """launch_eq_table, the whole table, against the oracle's eq_table; r with entries 0, 1, r - 1"""
    r = mc.eq_point(nvar, kind)
    got = run_eq_table(lib, 0, [r], nvar, 0, 1 << nvar)
    same(got[0], mc.mont_words(spartan.eq_table(r)), "eq table")


@pytest.mark.parametrize("kind", ["rand", "edges"])
@pytest.mark.parametrize("win", mc.EQ_WINDOWS, ids=lambda w: "nvar%d-base%d-count%d" % w)
def test_eq_table_window(lib, win, kind):
    """windows of 25- / 26-variable tables across multiples of 2^klo: eq evaluated at the window's indices"""
    nvar, base, count = win
    r = mc.eq_point(nvar, kind)
    got = run_eq_table(lib, 0, [r], nvar, base, count)
    same(got[0], mc.mont_words([mc.eq_at(r, base + i) for i in range(count)]), "eq window")


@pytest.mark.parametrize("shape", [(3, 0, 8), (14, 0, 1 << 14), (25, (1 << 25) - 300, 300)], ids=lambda s: "nvar%d-count%d" % (s[0], s[2]))
def test_eq_table_group(lib, shape):
    """launch_eq_table with the jobs of k = 3 distinct points"""
    nvar, base, count = shape
    rs = [mc.eq_point(nvar, "rand", seed=j) for j in range(3)]
    got = run_eq_table(lib, 3, rs, nvar, base, count)
    for j, r in enumerate(rs):
        same(got[j], mc.mont_words([mc.eq_at(r, base + i) for i in range(count)]), "proof %d" % j)


@pytest.mark.parametrize("scaled", [1, 0], ids=["scaled", "plain"])
@pytest.mark.parametrize("L", mc.EQ_FACTOR_L)
def test_eq_factors(lib, L, scaled):
    """k_eq_factors on eq_factors_for(L), as launch_col_stream launches it: lo, then the three copies
    scale[m] hi[x] at m 2^k + x; the rest of the scratch untouched"""
    r = mc.eq_point(L, "edges" if L > 2 else "rand")
    scale = [random.Random(L).randrange(R), 0, R - 1] if scaled else None
    want = mc.mont_words(mc.eq_factors_ref(L, r, scale))
    r_w = mc.mont_words(r)
    s_w = mc.mont_words(scale) if scaled else None
    scratch = mc.pattern(mc.EQ_SCRATCH)
    call(lib, "mle_eq_factors", L, ptr(r_w), ptr(s_w), ptr(scratch))
    same(scratch[:len(want)], want, "factor tables")
    intact(scratch[len(want):], "scratch behind the tables")


def test_eq_expand_stride(lib):
    """k_eq_expand with two blocks over 1 300 entries from an odd base: three passes, the last partly filled"""
    rng = random.Random(7)
    klo, nhi, base, count = 5, 64, 37, 1300
    lo, hi = [rng.randrange(R) for _ in range(1 << klo)], [rng.randrange(R) for _ in range(nhi)]
    lo_w, hi_w, out = mc.mont_words(lo), mc.mont_words(hi), mc.pattern(count)
    call(lib, "mle_eq_expand", ptr(lo_w), ptr(hi_w), nhi, klo, base, count, 2, ptr(out))
    same(out, mc.mont_words([lo[(i + base) & 31] * hi[(i + base) >> 5] % R for i in range(count)]), "expanded table")


# ------------------------------------------------------------------ openings
@pytest.mark.parametrize("outs", ["q", "rout", "both"])
@pytest.mark.parametrize("half", mc.OPEN_LEVEL_HALVES)
def test_open_level(lib, half, outs):
    """launch_open_level: quotient only, fold only, both"""
    t, p = mc.open_table(2 * half, "rand"), mc.open_points(1, "rand")
    qs, rs = mc.open_chain_ref(t, p)
    rin, p_w = mc.mont_words(t), mc.mont_words(p)
    rout = mc.pattern(half) if outs != "q" else None
    q = mc.pattern(half) if outs != "rout" else None
    call(lib, "mle_open_level", 0, 0, ptr(rin), half, ptr(rout), ptr(q), ptr(p_w))
    if q is not None:
        same(q, mc.mont_words(qs[0]), "quotients")
    if rout is not None:
        same(rout, mc.mont_words(rs[0]), "folded table")


def test_open_level_stride(lib):
    """k_open_level with one block over 700 pairs; point r - 1 on a table of r - 1"""
    half = 700
    t, p = mc.open_table(2 * half, "rm1"), [R - 1]
    t[5], t[1398] = 0, 1
    qs, rs = mc.open_chain_ref(t, p)
    rin, p_w, rout, q = mc.mont_words(t), mc.mont_words(p), mc.pattern(half), mc.pattern(half)
    call(lib, "mle_open_level", 1, 1, ptr(rin), half, ptr(rout), ptr(q), ptr(p_w))
    same(q, mc.mont_words(qs[0]), "quotients")
    same(rout, mc.mont_words(rs[0]), "folded table")


def run_open_fold(L, mode, grid, nf, nout, mask, kind="rand"):
    t = mc.open_table(nout << nf, kind, seed=nf)
    pts = mc.open_points(nf, "rand" if kind == "rand" else "edges", seed=nout)
    qs, rs = mc.open_chain_ref(t, pts)
    qoffs, nq = mc.fold_offsets(nf, nout, mask)
    rin, p_w = mc.mont_words(t), mc.mont_words(pts)
    rout, q = mc.pattern(nout), (mc.pattern(nq) if nq else None)
    qo = np.array(qoffs, dtype=np.uint64)
    call(L, "mle_open_fold", mode, grid, nf, ptr(rin), nout, ptr(rout), ptr(q), nq, ptr(p_w), ptr(qo))
    same(rout, mc.mont_words(rs[nf - 1]), "rout")
    if nq:  # the levels back to back: together they are the whole buffer
        want = [v for j in range(nf) if qoffs[j] != mc.NOQ for v in qs[j]]
        same(q, mc.mont_words(want), "quotient levels %s" % [j for j in range(nf) if qoffs[j] != mc.NOQ])


def _fold_ids(nf):
    return [(nf, m) for m in range(1 << nf)]


@pytest.mark.parametrize("nfmask", _fold_ids(2) + _fold_ids(3), ids=lambda x: "nf%d-off%d" % x)
@pytest.mark.parametrize("nout", mc.OPEN_FOLD_NOUT)
def test_open_fold_launcher(lib, nout, nfmask):
    """launch_open_fold, 2 and 3 levels, every subset of the levels' quotients switched off (qoff = ~0),
    the others back to back; nout = 2^14 takes k_open_fold_wave<2> / <3>"""
    nf, mask = nfmask
    run_open_fold(lib, 0, 0, nf, nout, mask)


@pytest.mark.parametrize("mask", [0, 5, 7])
@pytest.mark.parametrize("wg", mc.WAVE_DIRECT, ids=lambda wg: "w%d-g%d" % wg)
@pytest.mark.parametrize("nf", [2, 3])
def test_open_fold_wave_direct(lib, nf, wg, mask):
    """k_open_fold_wave<2> / <3> over 64 w outputs with the grid given: idle waves, ragged stride"""
    w, grid = wg
    run_open_fold(lib, 2, grid, nf, 64 * w, mask & ((1 << nf) - 1))


@pytest.mark.parametrize("nf", [2, 3])
def test_open_fold_lane_stride(lib, nf):
    """k_open_fold<2> / <3> with one block over 300 outputs; points 0, 1, r - 1"""
    run_open_fold(lib, 1, 1, nf, 300, 0, kind="edges")


@pytest.mark.parametrize("kind", ["zero", "rm1", "edges"])
@pytest.mark.parametrize("nout", [65, 1 << 14])
@pytest.mark.parametrize("nf", [2, 3])
def test_open_fold_value_edges(lib, nf, nout, kind):
    """an all-zero table, every entry r - 1, and points 0, 1, r - 1, on the per-lane and the wave form"""
    run_open_fold(lib, 0, 0, nf, nout, 0, kind=kind)


@pytest.mark.parametrize("with_q", [1, 0], ids=["q", "noq"])
@pytest.mark.parametrize("hl", mc.OPEN_TAIL, ids=lambda hl: "half%d-nlev%d" % hl)
def test_open_tail(lib, hl, with_q):
    """launch_open_tail from `half` pairs through nlev levels (up to the whole chain)"""
    half, nlev = hl
    t, pts = mc.open_table(2 * half, "rand", seed=nlev), mc.open_points(nlev, "edges" if nlev >= 3 else "rand")
    qs, rs = mc.open_chain_ref(t, pts)
    want_q = [v for q in qs for v in q]
    rin, p_w, last = mc.mont_words(t), mc.mont_words(pts), mc.pattern(1)
    q = mc.pattern(len(want_q)) if with_q else None
    call(lib, "mle_open_tail", ptr(rin), half, nlev, ptr(p_w), ptr(q), len(want_q) if with_q else 0, ptr(last))
    same(last, mc.mont_words(rs[-1][:1]), "last")
    if with_q:
        same(q, mc.mont_words(want_q), "quotients of the levels, contiguous")


@pytest.mark.parametrize("hrl", mc.OPEN_TAIL_LEVELS, ids=lambda x: "half%d-rem%d" % x[:2])
def test_open_tail_levels(lib, hrl):
    """open_tail_levels on its boundary (kTailMax pairs, the TailPoints capacity, fewer than 2 levels)"""
    half, remaining, want = hrl
    assert lib.mle_open_tail_levels(half, remaining) == want == mc.open_tail_levels(half, remaining)


def _plan_rounds():
    """every (which, fold, need1, half) of the round case tables, and the halves around the wave threshold"""
    out = {(w, f, n1, h) for w, h, f, n1, _ in mc.launcher_round_params()}
    out |= {(w, f, n1, h) for w, h, f, n1, _ in mc.edge_round_params()}
    out |= {(w, f, n1, h) for _, h, f, n1 in mc.GROUP_ROUNDS for w in (1, 2)}
    out |= {(w, f, n1, h) for w in (1, 2) for f in (0, 1) for n1 in (0, 1)
            for h in (1 << 13, (1 << 14) - 1, 1 << 14, 1 << 16, 1 << 20)}
    return sorted(out)


def test_round_plan(lib):
    """sc_round_plan, the one place of mle_kernels.hip that decides a round's form, grid, fused-or-reduce and
    per-proof launching, against round_dispatch / group_dispatch (host arithmetic, no launch)"""
    forms = {0: ("lane", "lane"), 1: ("quad", "pair"), 2: ("wave", "wave")}  # kRoundLane, kRoundSplit, kRoundWave
    for which, fold, need1, half in _plan_rounds():
        for k in (1, 2, 3, mc.GROUP_MAX):
            got = np.full(4, -1, dtype=np.int32)
            assert lib.mle_round_plan(which, k, fold, need1, half, ptr(got)) == 0
            form, grid, fused = mc.round_dispatch(which, fold, need1, half)
            what = (which, k, fold, need1, half)
            assert (forms[int(got[0])][which - 1], int(got[1]), bool(got[2])) == (form, grid, fused), what
            assert bool(got[3]) == (mc.group_dispatch(which, fold, need1, half, k) == "per-proof"), what


@pytest.mark.parametrize("Lv", sorted(set(mc.OPEN_EVAL_L) | {1, 2, 10, 11, 20}))
def test_open_eval_plan(lib, Lv):
    """open_eval_plan, the stubbed opening chain's steps for one proof and for a group, against
    mc.open_eval_plan (host arithmetic, no launch)"""
    steps = np.zeros((32, 5), dtype=np.uint64)
    copy = np.full(1, -1, dtype=np.int32)
    n = lib.mle_open_eval_plan(Lv, ptr(steps), 32, ptr(copy))
    want, want_copy = mc.open_eval_plan(Lv)
    assert n == len(want) and bool(copy[0]) == want_copy
    first = 0
    for (kind, at, levels, size, wave), w in zip(steps[:n].tolist(), want):
        assert at == first
        if w[0] == "tail":    # kOpenTail
            assert (kind, size, levels, wave) == (0, w[1], w[2], 0)
        elif w[0] == "fold":  # kOpenFold
            assert (kind, levels, size, bool(wave)) == (1, w[1], w[2], w[3])
        else:                 # kOpenLevel
            assert (kind, levels, size, wave) == (2, 1, w[1], 0)
        first += levels
    assert first == Lv


@pytest.mark.parametrize("k", mc.OPEN_EVAL_K)
@pytest.mark.parametrize("Lv", mc.OPEN_EVAL_L)
def test_open_eval_group(lib, Lv, k):
    """launch_open_eval with k jobs: last[j] = z_j(point_j) by the oracle's mle_eval. k = 1 walks the chain
    with the per-proof launchers (L = 1 ends on a level, whose output the copy kernel moves to `last`); k = 8
    and 9 take the group kernels (L = 17 the wave group fold, k = 9 two tail launches)"""
    n = 1 << Lv
    zs = [mc.open_table(n, "rand", seed=1000 + j) for j in range(k)]
    ps = [mc.open_points(Lv, "edges" if j == 1 and Lv >= 3 else "rand", seed=j) for j in range(k)]
    z_w = mc.mont_words([v for z in zs for v in z])
    p_w = mc.mont_words([v for p in ps for v in p])
    last = mc.pattern(k)
    call(lib, "mle_open_eval_group", k, ptr(z_w), ptr(p_w), Lv, ptr(last))
    same(last, mc.mont_words([spartan.mle_eval(z, p) for z, p in zip(zs, ps)]), "z_j(point_j)")


# ------------------------------------------------------------------ SpMV, conversions, copies
def check_spmv(case, zs, out):
    out = out.reshape(len(zs), 3, case.nrows, 8)
    named = np.zeros((3, case.nrows), dtype=bool)
    for d in case.dst:
        named[d >> 30, d & 0x3FFFFFFF] = True
    for j, z in enumerate(zs):
        ref = mc.spmv_ref(case.val, case.col, case.dst, z)
        keys = sorted(ref)
        got = np.stack([out[j, m, x] for m, x in keys])
        same(got, mc.mont_words([ref[key] for key in keys]), "proof %d: products" % j)
        intact(out[j][~named], "proof %d: slots no entry names" % j)


@pytest.mark.parametrize("entries", mc.SPMV_ENTRIES)
def test_spmv_sliced(lib, entries):
    """launch_spmv_sliced: fewer entries than eighths, a chunk boundary, two chunks per range"""
    c = mc.spmv_case(entries)
    z = mc.spmv_z(c.nz, 0)
    val_w, z_w = mc.mont_words(c.val), mc.mont_words(z)
    col, dst = np.array(c.col, dtype=np.uint32), np.array(c.dst, dtype=np.uint32)
    out = mc.pattern(3 * c.nrows)
    call(lib, "mle_spmv", 0, ptr(val_w), ptr(col), ptr(dst), entries, ptr(z_w), c.nz, ptr(out), c.nrows)
    check_spmv(c, [z], out)


@pytest.mark.parametrize("entries", [9, 8 * 1024 + 1])
@pytest.mark.parametrize("k", mc.SPMV_GROUP_K)
def test_spmv_sliced_group(lib, k, entries):
    """k_spmv_sliced_group: k = 1 and 3 end its two-at-a-time loop on an odd proof. k = 2, 3 through
    launch_spmv_sliced; a group of one is the per-proof kernel there, so k = 1 launches the group kernel
    itself, at the launcher's group grid"""
    c = mc.spmv_case(entries)
    zs = [mc.spmv_z(c.nz, j) for j in range(k)]
    val_w, z_w = mc.mont_words(c.val), mc.mont_words([v for z in zs for v in z])
    col, dst = np.array(c.col, dtype=np.uint32), np.array(c.dst, dtype=np.uint32)
    out = mc.pattern(k * 3 * c.nrows)
    args = (ptr(val_w), ptr(col), ptr(dst), entries, ptr(z_w), c.nz, ptr(out), c.nrows)
    if k == 1:
        call(lib, "mle_spmv_group_direct", k, mc.spmv_grid(entries, True), *args)
    else:
        call(lib, "mle_spmv", k, *args)
    check_spmv(c, zs, out)


def run_mont(L, mode, grid, w):
    data = w.copy()
    err = np.full(1, -1, dtype=np.int32)
    call(L, "mle_mont", mode, grid, ptr(data), len(data), ptr(err))
    return data, int(err[0])


def test_to_mont_values(lib):
    """k_to_mont: 0, 1, r - 1 convert and leave err clear; r, r + 1, 2^256 - 1 each set it"""
    got, err = run_mont(lib, 0, 0, mc.words(mc.TO_MONT_OK))
    same(got, mc.mont_words(mc.TO_MONT_OK), "Montgomery forms")
    assert err == 0
    for bad in mc.TO_MONT_BAD:
        _, err = run_mont(lib, 0, 0, mc.words([5, bad, 7]))
        assert err == 1, "non-canonical %x not flagged" % bad


def test_to_mont_stride(lib):
    """k_to_mont with two blocks over 1 000 elements"""
    vals = [random.Random(3).randrange(R) for _ in range(1000)]
    got, err = run_mont(lib, 1, 2, mc.words(vals))
    same(got, mc.mont_words(vals), "Montgomery forms")
    assert err == 0


def test_from_mont_round_trip(lib):
    """k_from_mont of Python's Montgomery forms gives the canonical words back"""
    vals = mc.TO_MONT_OK + [random.Random(4).randrange(R) for _ in range(600)]
    got, _ = run_mont(lib, 2, 0, mc.mont_words(vals))
    same(got, mc.words(vals), "canonical forms")


@pytest.mark.parametrize("shape", [(1, 1, 1), (3, 3, 5), (16, 2, 700), (2, 1, 4096)], ids=lambda s: "k%d-runs%d-per%d" % s)
def test_copy_runs_group(lib, shape):
    """launch_copy_runs: the runs of each proof back to back, words unchanged"""
    k, nruns, per = shape
    src = np.arange(k * nruns * per * 8, dtype=np.uint32).reshape(-1, 8)
    dst = mc.pattern(k * nruns * per)
    call(lib, "mle_copy_runs", k, ptr(src), nruns, per, ptr(dst))
    same(dst, src, "copied runs")
