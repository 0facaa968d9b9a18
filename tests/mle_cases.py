"""References and case tables for the kernels of mle_kernels.hip (tests/test_gpu_mle_ops.py runs them
through tests/native/mle_ops.hip; tests/test_mle_cases.py pins the references to the oracle on the CPU).

References are plain Python integers mod r, built on oracle/py/spartan.py where it has the function
(fix_first, eq_table, mle_eval) and otherwise written from the comments in mle_kernels.hip:
  sumcheck 1   G(t) = sum_b (A_t B_t - C_t) e,  X_0 = X[2b], X_1 = X[2b+1], X_2 = 2 X_1 - X_0;
               a fold round first binds the previous challenge (fix_first) and takes e' = E[2b] + E[2b+1]
  sumcheck 2   P(t) = sum_b M_t Z_t, the same fold
  opening      q[b] = r[2b+1] - r[2b],  r'[b] = r[2b] + p q[b]; level j's quotients at q + qoff[j]
  sliced SpMV  out_m[row] = val[e] z[col[e]], one entry per (row, matrix)
Python also does the Montgomery conversion (x 2^256 mod r and back): the kernels under test never
prepare or decode their own operands. A kernel's output is compared as its 8 x 32-bit Montgomery words
with the words of the reference value, so a non-canonical representative fails too.

The launch arithmetic of mle_kernels.hip is restated here (grid_for, round_dispatch, group_dispatch,
open_tail_levels, open_eval_plan) so that the shape tables can say, and test_mle_cases.py can assert,
which branch each shape reaches. The C++ side decides each of these in one function (sc_round_plan,
open_eval_plan), which every launch goes through, one proof or a group; test_gpu_mle_ops.py compares the
restatement with those two functions (test_round_plan, test_open_eval_plan). A launcher takes the jobs of k
proofs: k = 1 is the per-proof launch, k > 1 the group kernels. All case data comes from seeds; there are
no fixture files."""
import random
from functools import lru_cache
from types import SimpleNamespace

import numpy as np

import spartan
from spartan import R

MONT = pow(2, 256, R)
MONT_INV = pow(MONT, -1, R)
PATTERN = 0xA5A5A5A5  # fill of every output buffer: as an Fr it is above r, so no kernel result equals it
NOQ = (1 << 64) - 1   # qoff[j] == ~0: level j's quotients are not written


def to_mont(x):
    return x * MONT % R


def from_mont(m):
    return m * MONT_INV % R


def words(vals):
    """integers below 2^256 -> (n, 8) uint32, little-endian limbs"""
    buf = b"".join(v.to_bytes(32, "little") for v in vals)
    return np.frombuffer(buf, dtype="<u4").reshape(-1, 8).astype(np.uint32)


def mont_words(vals):
    return words([v * MONT % R for v in vals])


def ints(arr):
    b = np.ascontiguousarray(arr, dtype="<u4").tobytes()
    return [int.from_bytes(b[i:i + 32], "little") for i in range(0, len(b), 32)]


def pattern(n):
    return np.full((n, 8), PATTERN, dtype=np.uint32)


# ------------------------------------------------------------------ the launch arithmetic, restated
K_THREADS = 256
FUSE_MAX_BLOCKS = 64          # kFuseMaxBlocks
WAVE_MIN_HALF = 1 << 14       # kWaveMinHalf
WAVE_MAX_BLOCKS = 8192        # kWaveMaxBlocks = kRoundPartials / 3
ROUND_PARTIALS = 3 * 8192     # kRoundPartials
TAIL_MAX = 512                # kTailMax
TAIL_POINTS = 10              # sizeof(TailPoints) / sizeof(Fr)
TAIL_GROUP = 8                # kTailGroup
GROUP_MAX = 16                # kGroupMax
EQ_SCRATCH = 4 * 8192         # kEqScratch
SPMV_CHUNK = 256 * 4          # kThreads * kSpmvPer
# pairs (or outputs) one block takes per pass of its stride loop
PER_BLOCK = {"lane": 256, "pair": 128, "quad": 64, "wave": 256}


def grid_for(n, cap=2048):
    return max(1, min(cap, (n + K_THREADS - 1) // K_THREADS))


def round_dispatch(which, fold, need1, half):
    """sc_round_plan (launch_sc1_round / launch_sc2_round): (form, grid, fused)"""
    if half >= WAVE_MIN_HALF:
        g = grid_for(half, WAVE_MAX_BLOCKS)
        return "wave", g, g <= FUSE_MAX_BLOCKS
    if fold and not need1:
        g = grid_for((4 if which == 1 else 2) * half, FUSE_MAX_BLOCKS)
        return ("quad" if which == 1 else "pair"), g, True
    g = grid_for(half, 1024)
    return "lane", g, g <= FUSE_MAX_BLOCKS


def passes(form, grid, n):
    """iterations of the busiest lane's stride loop over n pairs (wave: over n / 64 waves, 4 per block)"""
    if form == "wave":
        return -(-(n // 64) // (4 * grid))
    return -(-n // (PER_BLOCK[form] * grid))


def group_dispatch(which, fold, need1, half, k):
    """launch_sc?_round with k jobs: 'per-proof' (the per-proof kernels, one proof after the other: a group
    of one, and the lane form, which has no group kernel) or the group kernel's form"""
    form = round_dispatch(which, fold, need1, half)[0]
    return "per-proof" if k == 1 or form == "lane" else form


def open_tail_levels(half, remaining):
    if half > TAIL_MAX or remaining < 2:
        return 0
    k = 0
    while (half >> k) >= 1 and k < remaining:
        k += 1
    return min(k, TAIL_POINTS)


def open_eval_plan(L):
    """open_eval_plan (launch_open_eval's steps) for n = 2^L: ('tail', half, levels) / ('fold', nf, nout, wave) /
    ('level', half), and whether the chain ends on a fold (then a copy writes `last`)"""
    n, i, steps = 1 << L, 0, []
    while i < L:
        half = n >> (i + 1)
        if open_tail_levels(half, L - i) == L - i:
            steps.append(("tail", half, L - i))
            return steps, False
        nf = 3 if L - i >= 3 and (half >> 2) >= 1 else (2 if L - i >= 2 and (half >> 1) >= 1 else 1)
        if nf > 1:
            nout = n >> (i + nf)
            steps.append(("fold", nf, nout, nout >= WAVE_MIN_HALF))
        else:
            steps.append(("level", half))
        i += nf
    return steps, True


def tail_launches(k):
    """proofs per k_open_tail_group launch of a group of k > 1 (one proof: k_open_tail itself, no group launch)"""
    return [min(TAIL_GROUP, k - j0) for j0 in range(0, k, TAIL_GROUP)] if k > 1 else []


def spmv_grid(entries, group):
    per_xcd = (entries // 8 + SPMV_CHUNK - 1) // SPMV_CHUNK
    return 8 * min(256, max(1, per_xcd if group else (per_xcd + 1) // 2))


def eq_split(L):
    k0 = (L + 1) // 2
    return k0, L - k0


# ------------------------------------------------------------------ references
def sc1_ref(A, B, C, E, r, fold):
    """(sums[3], folded (A, B, C) or None, E' or None)"""
    if fold:
        A, B, C = (spartan.fix_first(T, r) for T in (A, B, C))
        E = [(E[2 * b] + E[2 * b + 1]) % R for b in range(len(E) // 2)]
    s0 = s1 = s2 = 0
    for b, e in enumerate(E):
        a0, a1, b0, b1, c0, c1 = A[2 * b], A[2 * b + 1], B[2 * b], B[2 * b + 1], C[2 * b], C[2 * b + 1]
        s0 += (a0 * b0 - c0) * e
        s1 += (a1 * b1 - c1) * e
        s2 += ((2 * a1 - a0) * (2 * b1 - b0) - (2 * c1 - c0)) * e
    return [s0 % R, s1 % R, s2 % R], ((A, B, C) if fold else None), (E if fold else None)


def sc2_ref(M, Z, r, fold):
    """(sums[3], folded (M, Z) or None)"""
    if fold:
        M, Z = spartan.fix_first(M, r), spartan.fix_first(Z, r)
    s0 = s1 = s2 = 0
    for b in range(len(M) // 2):
        m0, m1, z0, z1 = M[2 * b], M[2 * b + 1], Z[2 * b], Z[2 * b + 1]
        s0 += m0 * z0
        s1 += m1 * z1
        s2 += (2 * m1 - m0) * (2 * z1 - z0)
    return [s0 % R, s1 % R, s2 % R], ((M, Z) if fold else None)


def eq_at(r, x):
    """eq(r, x) = prod_j (x_j ? r_j : 1 - r_j), variable 0 = LSB"""
    v = 1
    for j, rj in enumerate(r):
        v = v * (rj if (x >> j) & 1 else 1 - rj) % R
    return v


def eq_factors_ref(L, r, scale):
    """eq_factors_for(L) filled by k_eq_factors: lo (2^k0), then the last table: scale[m] hi[x] at
    m 2^k1 + x (three copies), or hi itself without a scale"""
    k0, k1 = eq_split(L)
    lo, hi = spartan.eq_table(r[:k0]), spartan.eq_table(r[k0:])
    if scale is None:
        return lo + hi
    return lo + [s * h % R for s in scale for h in hi]


def open_chain_ref(table, points):
    """the levels of open.rs:42-45: ([q_0, q_1, ...], [r_1, r_2, ...]) for the given points"""
    qs, rs, cur = [], [], list(table)
    for p in points:
        q = [(cur[2 * b + 1] - cur[2 * b]) % R for b in range(len(cur) // 2)]
        cur = [(cur[2 * b] + p * q[b]) % R for b in range(len(q))]
        qs.append(q)
        rs.append(cur)
    return qs, rs


def spmv_ref(val, col, dst, z):
    """{(matrix, row): val z[col]}"""
    return {(d >> 30, d & 0x3FFFFFFF): v * z[c] % R for v, c, d in zip(val, col, dst)}


# ------------------------------------------------------------------ round cases
# launcher level: both sumchecks, fold off / on, need1 off / on, Eout null / non-null at every half
ROUND_HALVES = [1, 2, 3, 64, 65, 128, 129, 256, 257, 4096, 8192, 12288, 1 << 14, 1 << 15]
# direct wave launches: half = 64 w over `grid` blocks (4 waves each)
WAVE_DIRECT = [(1, 1), (7, 1), (9, 2), (130, 3)]
REDUCE_NBLK = [1, 2, 255, 256, 257, 8192]
# value edges: one small shape (two blocks in every small form) and one wave shape
EDGE_HALVES = [129, 1 << 14]
EDGE_KINDS_TABLES = ["zero", "rm1", "ezero", "abc"]  # ezero, abc: sumcheck 1 only
EDGE_KINDS_CHALLENGE = ["r0", "r1", "rm1c"]          # fold rounds only


def _rand(rng, n):
    return [rng.randrange(R) for _ in range(n)]


def round_inputs(which, half, fold, kind, seed):
    """integer tables of one round: (tabs, E or None, r)"""
    rng = random.Random("round %d %d %d %s %d" % (which, half, fold, kind, seed))
    ntab = 3 if which == 1 else 2
    nin, nE = (4 if fold else 2) * half, (2 if fold else 1) * half
    r = {"r0": 0, "r1": 1, "rm1c": R - 1}.get(kind, rng.randrange(R))
    if kind == "zero":
        tabs = [[0] * nin for _ in range(ntab)]
    elif kind == "rm1":
        tabs = [[R - 1] * nin for _ in range(ntab)]
    else:
        tabs = [_rand(rng, nin) for _ in range(ntab)]
    if kind == "abc":  # A constant over each pair (each four of a fold round) and C = A B entry by entry:
        # A_t B_t = C_t at t = 0, 1, 2, before and after the fold, so every term of every sum is 0
        g = 4 if fold else 2
        a = _rand(rng, nin // g)
        tabs[0] = [a[i // g] for i in range(nin)]
        tabs[2] = [x * y % R for x, y in zip(tabs[0], tabs[1])]
    E = None
    if which == 1:
        E = [0] * nE if kind == "ezero" else ([R - 1] * nE if kind == "rm1" else _rand(rng, nE))
    return tabs, E, r


def build_round(which, half, fold, kind="rand", seed=0):
    tabs, E, r = round_inputs(which, half, fold, kind, seed)
    if which == 1:
        sums, out, Eout = sc1_ref(tabs[0], tabs[1], tabs[2], E, r, fold)
    else:
        sums, out = sc2_ref(tabs[0], tabs[1], r, fold)
        Eout = None
    c = SimpleNamespace(which=which, half=half, fold=fold, kind=kind, ntab=len(tabs), nin=len(tabs[0]),
                        nE=len(E) if E else 0, sums=sums)
    c.tabs_w = mont_words([v for T in tabs for v in T])
    c.E_w = mont_words(E) if E else None
    c.r_w = mont_words([r])
    c.sums_w = mont_words(sums)
    c.out_w = mont_words([v for T in out for v in T]) if fold else None
    c.Eout_w = mont_words(Eout) if Eout is not None else None
    return c


@lru_cache(maxsize=4)
def round_case(which, half, fold, kind="rand"):
    """one reference per (sumcheck, half, fold, kind), shared by the need1 / Eout / form variants"""
    return build_round(which, half, fold, kind)


def launcher_round_params():
    """(which, half, fold, need1, eout)"""
    out = []
    for which in (1, 2):
        for half in ROUND_HALVES:
            for fold in (0, 1):
                for need1 in (0, 1):
                    for eout in ((0, 1) if which == 1 and fold else (0,)):
                        out.append((which, half, fold, need1, eout))
    return out


def edge_round_params():
    """(which, half, fold, need1, kind): the fold round without G(1) and round 1 with it at both shapes
    (small: quad / pair and per-lane; 2^14: wave<1,0> and wave<0,1>), the small per-lane fold as well"""
    out = []
    for which in (1, 2):
        kinds = EDGE_KINDS_TABLES if which == 1 else EDGE_KINDS_TABLES[:2]
        for half in EDGE_HALVES:
            combos = [(1, 0), (0, 1)] + ([(1, 1)] if half < WAVE_MIN_HALF else [])
            for fold, need1 in combos:
                for kind in kinds + (EDGE_KINDS_CHALLENGE if fold else []):
                    out.append((which, half, fold, need1, kind))
    return out


# group level: (k, half, fold, need1); k = 16 keeps half <= 2^14 and round 1 (its reference stays short)
GROUP_ROUNDS = [
    (1, 1 << 14, 1, 0), (3, 1 << 14, 1, 0), (3, 1 << 14, 0, 1), (16, 1 << 14, 0, 0),
    (1, 1 << 15, 0, 1), (3, 1 << 15, 1, 0),
    (1, 200, 1, 0), (3, 200, 1, 0), (16, 200, 1, 0),   # small fold round: the quad / pair group kernels
    (1, 300, 0, 1), (3, 300, 1, 1), (16, 300, 0, 1),   # small need1 rounds: the per-proof fallback
]


# ------------------------------------------------------------------ eq cases
EQ_FULL_NVAR = [0, 1, 2, 3, 13, 14, 15]
EQ_WINDOWS = [  # (nvar, base, count): crossing multiples of 2^klo, the first and the last entry
    (25, (1 << 25) - 300, 300), (25, 0, 1), (25, (1 << 25) - 1, 1), (25, (1 << 13) - 100, 300),
    (26, (1 << 25) - 100, 300), (26, 0, 1), (26, (1 << 26) - 1, 1), (26, 5 * (1 << 13) - 1, 2),
]
EQ_FACTOR_L = [1, 2, 13, 26]


def eq_point(nvar, kind, seed=0):
    rng = random.Random("eq %d %s %d" % (nvar, kind, seed))
    r = _rand(rng, nvar)
    if kind == "edges":  # entries 0, 1, r - 1 among random ones
        for j, v in zip(range(0, nvar, 2), [0, 1, R - 1] * nvar):
            r[j] = v
    return r


# ------------------------------------------------------------------ opening cases
OPEN_LEVEL_HALVES = [1, 255, 256, 257]
OPEN_FOLD_NOUT = [1, 63, 64, 65, (1 << 14) - 64, 1 << 14]
OPEN_TAIL = [(1, 1), (2, 1), (2, 2), (256, 1), (256, 5), (256, 9), (512, 1), (512, 10)]  # (half, nlev)
OPEN_TAIL_LEVELS = [  # (half, remaining, levels taken)
    (512, 1, 0), (512, 2, 2), (512, 10, 10), (512, 11, 10), (513, 2, 0), (513, 10, 0), (513, 11, 0), (513, 1, 0),
    (1, 2, 1), (1, 1, 0),
]
OPEN_EVAL_L = [1, 2, 3, 9, 10, 11, 12, 17]
OPEN_EVAL_K = [1, 8, 9]


def open_table(n, kind, seed=0):
    rng = random.Random("open %d %s %d" % (n, kind, seed))
    if kind == "zero":
        return [0] * n
    if kind == "rm1":
        return [R - 1] * n
    return _rand(rng, n)


def open_points(n, kind, seed=0):
    rng = random.Random("points %d %s %d" % (n, kind, seed))
    p = _rand(rng, n)
    if kind == "edges":
        for j, v in zip(range(n), [0, 1, R - 1]):
            p[j] = v
    return p


def fold_offsets(nf, nout, mask):
    """levels' quotient ranges back to back in level order (a write one slot off lands in a neighbour's
    range), the levels in `mask` (bit j) left out: (qoffs, nq)"""
    qoffs, nq = [], 0
    for j in range(nf):
        if (mask >> j) & 1:
            qoffs.append(NOQ)
        else:
            qoffs.append(nq)
            nq += nout << (nf - 1 - j)
    return qoffs, nq


# ------------------------------------------------------------------ SpMV and conversion cases
SPMV_ENTRIES = [1, 7, 8, 9, 1023, 8 * 1024, 8 * 1024 + 1, 3 << 13]
SPMV_GROUP_K = [1, 2, 3]


def spmv_case(entries, seed=0):
    """entries spread over the three matrices, one per (row, matrix), columns ascending; nrows leaves
    three rows that no entry names"""
    rng = random.Random("spmv %d %d" % (entries, seed))
    nrows = (entries + 2) // 3 + 3
    nz = max(4, entries // 3)
    slots = [(m, x) for x in range(nrows - 3) for m in range(3)][:entries]
    rng.shuffle(slots)
    col = sorted(rng.randrange(nz) for _ in range(entries))
    val = _rand(rng, entries)
    for i in range(0, entries, 5):
        val[i] = [0, 1, R - 1][(i // 5) % 3]
    dst = [(m << 30) | x for m, x in slots]
    return SimpleNamespace(entries=entries, nrows=nrows, nz=nz, val=val, col=col, dst=dst)


def spmv_z(nz, seed):
    return _rand(random.Random("spmv z %d %d" % (nz, seed)), nz)


TO_MONT_OK = [0, 1, R - 1, 2, R - 2, MONT, (R - 1) // 2]
TO_MONT_BAD = [R, R + 1, (1 << 256) - 1]
