"""tests/mle_cases.py on the CPU: its references pinned to the oracle (oracle/py/spartan.py), and the
claims of its shape tables asserted with the launch arithmetic of mle_kernels.hip restated in Python.
A later change of kWaveMinHalf, kFuseMaxBlocks, kTailMax or kTailGroup has to be restated in
mle_cases.py, and then a table that no longer reaches its branch fails here instead of silently testing
nothing on the GPU."""
import random
from types import SimpleNamespace

import numpy as np
import pytest

import mle_cases as mc
import spartan
from mle_cases import R


def _rand(seed, n):
    rng = random.Random(seed)
    return [rng.randrange(R) for _ in range(n)]


# ------------------------------------------------------------------ references against the oracle
@pytest.mark.parametrize("half", [1, 3, 37])
def test_sc2_reference_is_the_oracles_round(half):
    M, Z, r = _rand(1, 4 * half), _rand(2, 4 * half), _rand(3, 1)[0]
    o = spartan.MLSumcheckProver([[M, Z]], 8)
    sums, out = mc.sc2_ref(M, Z, None, 0)
    assert sums == o.prove_round(None) and out is None
    sums, (Mo, Zo) = mc.sc2_ref(M, Z, r, 1)
    assert sums == o.prove_round(r)
    assert Mo == spartan.fix_first(M, r) and Zo == spartan.fix_first(Z, r)


@pytest.mark.parametrize("half", [1, 3, 37])
def test_sc1_reference_is_g_of_t(half):
    """G(t) = sum_b (A_t B_t - C_t) e evaluated naively from X_t = X_0 + t (X_1 - X_0), and the same
    sums from the oracle's prover on the products A B E - C E (its t = 0, 1, 2)"""
    A, B, C = (_rand(s, 4 * half) for s in (1, 2, 3))
    E, r = _rand(4, 2 * half), _rand(5, 1)[0]

    def naive(A, B, C, E):
        out = []
        for t in range(3):
            s = 0
            for b in range(len(E)):
                at, bt, ct = (X[2 * b] + t * (X[2 * b + 1] - X[2 * b]) for X in (A, B, C))
                s += (at * bt - ct) * E[b]
            out.append(s % R)
        return out

    def oracle(A, B, C, E, challenge=None):
        # E depends on no round variable of the kernel's tables: as a table of the oracle's prover it is
        # constant over each pair, E2[2b] = E2[2b+1] = E[b]
        E2 = [e for e in E for _ in range(2)]
        negC = [(-c) % R for c in C]
        return spartan.MLSumcheckProver([[A, B, E2], [negC, E2]], 8).prove_round(challenge)[:3]

    # round 1: the 4 half entries of a table are 2 half pairs, one entry of E each
    sums, out, Eo = mc.sc1_ref(A, B, C, E, None, 0)
    assert sums == naive(A, B, C, E) == oracle(A, B, C, E) and out is None and Eo is None
    sums, (Ao, Bo, Co), Eo = mc.sc1_ref(A, B, C, E, r, 1)
    assert [Ao, Bo, Co] == [spartan.fix_first(X, r) for X in (A, B, C)]
    assert Eo == [(E[2 * b] + E[2 * b + 1]) % R for b in range(half)]
    assert sums == naive(Ao, Bo, Co, Eo) == oracle(Ao, Bo, Co, Eo)


def test_abc_tables_sum_to_zero():
    for which, kinds in ((1, ["zero", "ezero", "abc"]), (2, ["zero"])):
        for fold in (0, 1):
            for kind in kinds:
                assert mc.build_round(which, 5, fold, kind).sums == [0, 0, 0], (which, fold, kind)
    assert mc.build_round(1, 5, 1, "rm1").sums != [0, 0, 0]


@pytest.mark.parametrize("nvar", [0, 1, 2, 7])
def test_eq_references(nvar):
    r = mc.eq_point(nvar, "edges")
    tab = spartan.eq_table(r)
    assert tab == [mc.eq_at(r, x) for x in range(1 << nvar)]
    if nvar:
        ext = spartan.eq_extension(r)
        for x in (0, (1 << nvar) - 1, 5 % (1 << nvar)):
            prod = 1
            for poly in ext:
                prod = prod * poly[x] % R
            assert prod == tab[x]
        scale = _rand(nvar, 3)
        k0, k1 = mc.eq_split(nvar)
        f = mc.eq_factors_ref(nvar, r, scale)
        assert len(f) == (1 << k0) + 3 * (1 << k1)
        for m in range(3):
            for x in range(1 << nvar):
                assert f[x & ((1 << k0) - 1)] * f[(1 << k0) + (m << k1) + (x >> k0)] % R == scale[m] * tab[x] % R


def test_opening_reference_is_the_oracles_open(monkeypatch):
    """open_'s quotients q[k] and evaluation with its commitments stubbed out (the scalar side only)"""
    nv = 6
    table, point = _rand(1, 1 << nv), _rand(2, nv)
    monkeypatch.setattr(spartan, "msm", lambda curve, bases, scalars: None)
    monkeypatch.setattr(spartan, "G2", SimpleNamespace(to_affine=lambda p: p))
    value, _, q = spartan.open_(SimpleNamespace(powers_of_h=[None] * nv, h=None), table, point)
    qs, rs = mc.open_chain_ref(table, point)
    assert [q[nv - i] for i in range(nv)] == qs
    assert rs[-1] == [value] == [spartan.mle_eval(table, point)]
    for j in range(nv):  # the table after j + 1 levels evaluates to the same value at the remaining point
        assert spartan.mle_eval(rs[j], point[j + 1:]) == value


def test_montgomery_helpers_round_trip():
    vals = mc.TO_MONT_OK + _rand(9, 50)
    assert [mc.from_mont(mc.to_mont(v)) for v in vals] == vals
    assert mc.to_mont(1) == (1 << 256) % R and mc.from_mont((1 << 256) % R) == 1
    assert mc.ints(mc.words(vals)) == vals
    assert mc.ints(mc.mont_words(vals)) == [mc.to_mont(v) for v in vals]
    w = mc.words([1 + (2 << 32) + (3 << 224)])
    assert w.dtype == np.uint32 and w.tolist() == [[1, 2, 0, 0, 0, 0, 0, 3]]
    assert all(v >= R for v in mc.ints(mc.pattern(2)))  # the fill pattern is no canonical Fr
    assert all(b >= R for b in mc.TO_MONT_BAD) and all(v < R for v in mc.TO_MONT_OK)


def test_spmv_case_shape():
    for entries in mc.SPMV_ENTRIES:
        c = mc.spmv_case(entries)
        assert len(c.val) == len(c.col) == len(c.dst) == entries
        assert c.col == sorted(c.col) and max(c.col) < c.nz
        assert len(set(c.dst)) == entries, "one entry per (row, matrix)"
        assert all((d >> 30) < 3 and (d & 0x3FFFFFFF) < c.nrows - 3 for d in c.dst), "three rows stay unnamed"
        if entries >= 3:
            assert {d >> 30 for d in c.dst} == {0, 1, 2}
        ref = mc.spmv_ref(c.val, c.col, c.dst, mc.spmv_z(c.nz, 0))
        assert len(ref) == entries


# ------------------------------------------------------------------ what the shape tables claim to reach
def test_round_shapes_reach_their_branches():
    d = mc.round_dispatch
    assert mc.ROUND_HALVES == sorted(set(mc.ROUND_HALVES))
    # one block against two, per small form
    assert (d(1, 1, 0, 64), d(1, 1, 0, 65)) == (("quad", 1, True), ("quad", 2, True))
    assert (d(2, 1, 0, 128), d(2, 1, 0, 129)) == (("pair", 1, True), ("pair", 2, True))
    for which in (1, 2):
        for fold, need1 in ((0, 0), (0, 1), (1, 1)):
            assert (d(which, fold, need1, 256), d(which, fold, need1, 257)) == (("lane", 1, True), ("lane", 2, True))
    # the quad form's full grid without a second pass, then its stride; the pair form's stride at no power of two
    assert d(1, 1, 0, 4096) == ("quad", mc.FUSE_MAX_BLOCKS, True) and mc.passes("quad", 64, 4096) == 1
    assert d(1, 1, 0, 8192) == ("quad", 64, True) and mc.passes("quad", 64, 8192) == 2
    assert d(2, 1, 0, 8192) == ("pair", 64, True) and mc.passes("pair", 64, 8192) == 1
    assert d(2, 1, 0, 12288) == ("pair", 64, True) and mc.passes("pair", 64, 12288) == 2 and 12288 & 12287
    assert d(1, 1, 0, 12288) == ("quad", 64, True) and mc.passes("quad", 64, 12288) == 3
    # every small half stays below the wave threshold, fused; the two wave shapes: fused g = 64, unfused g = 128
    for half in mc.ROUND_HALVES:
        for which in (1, 2):
            for fold in (0, 1):
                for need1 in (0, 1):
                    form, g, fused = d(which, fold, need1, half)
                    assert (form == "wave") == (half >= mc.WAVE_MIN_HALF)
                    assert 3 * g <= mc.ROUND_PARTIALS
                    if form == "wave":
                        assert half % 64 == 0, "whole waves"
                        assert (g, fused) == ((64, True) if half == 1 << 14 else (128, False))
                    else:
                        assert fused, "the launcher reaches the unfused small kernels at no half below 2^14"
    assert mc.ROUND_HALVES[-2:] == [1 << 14, 1 << 15] == [mc.WAVE_MIN_HALF, 2 * mc.WAVE_MIN_HALF]
    assert mc.FUSE_MAX_BLOCKS * mc.K_THREADS == mc.WAVE_MIN_HALF


def test_edge_and_group_shapes_reach_their_branches():
    small, wave = mc.EDGE_HALVES
    assert mc.round_dispatch(1, 1, 0, small) == ("quad", 3, True) and mc.round_dispatch(2, 1, 0, small) == ("pair", 2, True)
    assert mc.round_dispatch(1, 0, 1, small)[0] == mc.round_dispatch(1, 1, 1, small)[0] == "lane"
    assert mc.round_dispatch(1, 1, 0, wave)[0] == mc.round_dispatch(2, 0, 1, wave)[0] == "wave"
    kinds = {(p[0], p[4]) for p in mc.edge_round_params()}
    assert {(1, k) for k in mc.EDGE_KINDS_TABLES + mc.EDGE_KINDS_CHALLENGE} <= kinds
    assert {(2, k) for k in ["zero", "rm1"] + mc.EDGE_KINDS_CHALLENGE} <= kinds
    assert all(p[2] for p in mc.edge_round_params() if p[4] in mc.EDGE_KINDS_CHALLENGE), "a challenge needs a fold"
    forms = {}
    for k, half, fold, need1 in mc.GROUP_ROUNDS:
        assert 1 <= k <= mc.GROUP_MAX and (k < 16 or half <= 1 << 14)
        for which in (1, 2):
            forms.setdefault(mc.group_dispatch(which, fold, need1, half, k), set()).add(k)
            _, g, fused = mc.round_dispatch(which, fold, need1, half)
            if half == 1 << 15:
                assert not fused, "k_reduce_partials_group"
    # a group of one is the per-proof launch whatever its shape; the lane form is per-proof at every k
    assert forms["wave"] == {3, 16} and forms["quad"] == {3, 16} and forms["pair"] == {3, 16}
    assert forms["per-proof"] == {1, 3, 16}
    for which in (1, 2):
        one = {mc.round_dispatch(which, f, n1, h)[0] for k, h, f, n1 in mc.GROUP_ROUNDS if k == 1}
        assert one == {"wave", "quad" if which == 1 else "pair", "lane"}, "k = 1 rows of every form, all per-proof"
        for kk in (3, 16):
            assert any(mc.group_dispatch(which, f, n1, h, k) == "per-proof" for k, h, f, n1 in mc.GROUP_ROUNDS if k == kk)
    assert {k for k, *_ in mc.GROUP_ROUNDS} == {1, 3, 16}


def test_direct_shapes_reach_their_branches():
    # wave kernels, 4 waves per block: idle waves, a ragged second pass, several blocks
    assert mc.WAVE_DIRECT[0] == (1, 1)  # three waves of the block have no work and enter the reduction
    w, g = mc.WAVE_DIRECT[1]
    assert g == 1 and 4 < w < 8 and mc.passes("wave", g, 64 * w) == 2
    for w, g in mc.WAVE_DIRECT[2:]:
        assert g > 1 and w % (4 * g) and mc.passes("wave", g, 64 * w) >= 2
    assert mc.passes("wave", 3, 64 * 130) == 11
    # the reduction kernel around its 256 threads, and the largest grid a round has
    assert {255, 256, 257} <= set(mc.REDUCE_NBLK) and max(mc.REDUCE_NBLK) == mc.WAVE_MAX_BLOCKS == mc.ROUND_PARTIALS // 3
    assert mc.passes("quad", 1, 200) == 4 and mc.passes("pair", 1, 200) == 2 and mc.passes("lane", 2, 700) == 2


def test_opening_shapes_reach_their_branches():
    assert [n >= mc.WAVE_MIN_HALF for n in mc.OPEN_FOLD_NOUT] == [False] * 5 + [True]
    assert mc.OPEN_FOLD_NOUT[-1] % 64 == 0 and mc.OPEN_FOLD_NOUT[-2] == mc.WAVE_MIN_HALF - 64
    assert {255, 256, 257} <= set(mc.OPEN_LEVEL_HALVES)
    for half, nlev in mc.OPEN_TAIL:
        assert half <= mc.TAIL_MAX and 1 <= nlev <= mc.TAIL_POINTS and (half >> (nlev - 1)) >= 1
    assert (mc.TAIL_MAX, mc.TAIL_POINTS) in mc.OPEN_TAIL and (256, 9) in mc.OPEN_TAIL  # the full chains
    for half, remaining, want in mc.OPEN_TAIL_LEVELS:
        assert mc.open_tail_levels(half, remaining) == want
    assert {h for h, _, _ in mc.OPEN_TAIL_LEVELS} >= {mc.TAIL_MAX, mc.TAIL_MAX + 1}
    # the fold offsets tile the quotient buffer exactly
    for nf in (2, 3):
        for mask in range(1 << nf):
            qoffs, nq = mc.fold_offsets(nf, 64, mask)
            live = [(qoffs[j], 64 << (nf - 1 - j)) for j in range(nf) if not (mask >> j) & 1]
            assert sum(n for _, n in live) == nq and [o for o, _ in live] == [sum(n for _, n in live[:i]) for i in range(len(live))]
    # the group chain: L = 17 starts with the wave group fold (3 levels), L = 10 is one tail, L = 11 / 12 fold once
    # into a tail, L = 1 is one level and the copy
    plan = {L: mc.open_eval_plan(L) for L in mc.OPEN_EVAL_L}
    assert plan[17][0][0] == ("fold", 3, 1 << 14, True) and plan[17][0][-1][0] == "tail"
    assert plan[10] == ([("tail", 512, 10)], False) and plan[9] == ([("tail", 256, 9)], False)
    assert plan[11] == ([("fold", 3, 256, False), ("tail", 128, 8)], False)
    assert plan[12] == ([("fold", 3, 512, False), ("tail", 256, 9)], False)
    assert plan[1] == ([("level", 1)], True) and plan[2] == ([("tail", 2, 2)], False) and plan[3] == ([("tail", 4, 3)], False)
    # no group chain reaches the 2-level fold: two remaining levels always fit the tail
    for L in range(1, 27):
        assert all(s[:2] != ("fold", 2) for s in mc.open_eval_plan(L)[0])
    # one proof takes k_open_tail itself; 8 proofs fill one group tail launch, 9 need a second
    assert [mc.tail_launches(k) for k in mc.OPEN_EVAL_K] == [[], [8], [8, 1]]


def test_eq_and_spmv_shapes_reach_their_branches():
    for nvar, base, count in mc.EQ_WINDOWS:
        assert nvar in (25, 26) and base + count <= 1 << nvar and count <= 300
    k0 = mc.eq_split(26)[0]
    assert k0 == 13 and mc.eq_split(25) == (13, 12) and mc.eq_split(1) == (1, 0)
    crossing = [(n, b, c) for n, b, c in mc.EQ_WINDOWS if (b >> 13) != ((b + c - 1) >> 13)]
    assert {n for n, _, _ in crossing} == {25, 26}, "a window across a multiple of 2^klo at both sizes"
    assert {(n, b + c) for n, b, c in mc.EQ_WINDOWS} >= {(25, 1 << 25), (26, 1 << 26)}, "the last entry"
    assert max(mc.EQ_FULL_NVAR) == 15 and {0, 1, 13, 14} <= set(mc.EQ_FULL_NVAR)
    for L in mc.EQ_FACTOR_L:
        k0, k1 = mc.eq_split(L)
        assert (1 << k0) + 3 * (1 << k1) <= mc.EQ_SCRATCH
    # SpMV: fewer entries than eighths; 8 x 1024 fills one chunk per range exactly, one more entry spills;
    # 3 x 2^13 gives three chunks per range over a launcher grid of two blocks per range (a stride)
    g = mc.spmv_grid
    assert min(mc.SPMV_ENTRIES) < 8 and {7, 8, 9, 8 * mc.SPMV_CHUNK, 8 * mc.SPMV_CHUNK + 1} <= set(mc.SPMV_ENTRIES)
    assert g(8 * 1024, False) == 8 and g(8 * 1024 + 1, False) == 8 and g(3 << 13, False) == 16 and g(3 << 13, True) == 24
    assert -(-(3 << 13) // 8 // mc.SPMV_CHUNK) == 3
    assert set(mc.SPMV_GROUP_K) == {1, 2, 3}
