"""Integer models, word for word, of the field functions on the bucket accumulation's mixed-addition
path (ff29.hpp, fq2pair.hpp), and their directed operands. tests/test_accum_refs.py checks the models
against plain big-integer arithmetic on the CPU; tests/test_gpu_accum_ops.py compares the device
functions (tests/native/accum_ops.hip) with the models' words.

A model follows the header's definition limb by limb in Python `int`s, where nothing can overflow, and
asserts every bound the header states on the way (a column below 2^64, limbs below 2^29 or 2^30), so a
case that passes the CPU test is inside the documented preconditions. The Montgomery scan has one
result whatever the order its columns are summed in: `redc` takes the 27 column sums as integers, and
restates the ways a column can take the previous column's carry: joined (f29_redc_sum: the chain from
0, the carry added after it), seeded (the lockstep pairs of f29_redc_scan_x2: the carry first) and
split (measured and not kept), to show that they produce the same words inside 2^64.

The operands are those of tests/field_cases.py: limbs all 2^29 - 1, limbs 2^30 - 2 after doubling,
K p - 1 and K p + 1 for the K in use, the loose accumulator bounds X < 8p, Y < 4p.
"""
import itertools
import random

import field_cases as fc

P, M29 = fc.P, fc.M29
PL = fc.limbs29(P)
PINV = (-pow(P, -1, 1 << 29)) % (1 << 29)
R29I = fc.R29I
assert PINV == 0x1FFCFFFD
P16 = fc.limbs29(16 * P)
K16 = [P16[0] + (1 << 29)] + [P16[i] + (1 << 29) - 1 for i in range(1, 13)] + [P16[13] - 1]
assert fc.val29(K16) == 16 * P
SEED = 0xACC08

OPS = {"f29_sqr_x2": 0, "f29_mul": 1, "f29_mul2": 2, "f29_redc_sum4": 3, "pair_mul": 4, "pair_mul_sum": 5,
       "pair_sqr_b<8>": 6, "pair_sqr_b<16>": 7, "pair_prep": 8, "f29_mul_x2": 9, "f29_mul2_x2": 10,
       "pair_mul_x2": 11, "pair_sqr_x2<16,8>": 12}


# ------------------------------------------------------------------ the scan
def columns(prods):
    """27 column sums of the limb products of the (a, b) limb pairs in prods"""
    cols = [0] * 27
    for a, b in prods:
        for i in range(14):
            for j in range(14):
                cols[i + j] += a[i] * b[j]
    return cols


def redc(cols, limit=1 << 64, form="joined"):
    """the 14 result words of the scan over the given column sums; asserts that every column, with its
    m p terms and the carry, stays below `limit`.
    form: how the carry enters: the sums are the same integers, only the points at which a partial
    sum is formed, and so the bounds that are asserted, differ."""
    m, t, carry = [], [], 0
    for k in range(27):
        lo = 0 if k < 14 else k - 13
        mp = sum(m[i] * PL[k - i] for i in range(lo, k if k < 14 else 14))
        if form == "seeded":    # carry first, then the products, then m p: one chain
            acc = carry + cols[k]
            assert acc < limit
            acc += mp
        elif form == "split":   # products alone; the carry with the m p chain; one join
            assert cols[k] < limit and carry + mp < limit
            acc = cols[k] + (carry + mp)
        else:                   # joined: products and m p from 0, then the carry
            assert cols[k] + mp < limit
            acc = cols[k] + mp + carry
        assert acc < limit
        if k < 14:
            m.append(((acc & 0xFFFFFFFF) * PINV) & M29)
            acc += m[k] * PL[0]
            assert acc < limit and acc & M29 == 0
        else:
            t.append(acc & M29)
        carry = acc >> 29
    assert carry < 1 << 32
    return tuple(t) + (carry,)


def redc4(prods, form="joined"):
    """f29_redc_sum4: chain A = products 0, 1 (with the carry when seeded), chain B = products 2, 3 and
    m p, each below 2^64, joined by low and high parts"""
    ca_cols, cb_cols = columns(prods[:2]), columns(prods[2:])
    m, t, carry = [], [], 0
    for k in range(27):
        lo = 0 if k < 14 else k - 13
        ca = ca_cols[k] + (carry if form == "seeded" else 0)
        cb = cb_cols[k] + sum(m[i] * PL[k - i] for i in range(lo, k if k < 14 else 14))
        assert ca < 1 << 64 and cb < 1 << 64
        low = (ca & M29) + (cb & M29)
        high = (ca >> 29) + (cb >> 29)
        if form != "seeded":
            low += carry & M29
            high += carry >> 29
        if k < 14:
            m.append(((low & 0xFFFFFFFF) * PINV) & M29)
            low += m[k] * PL[0]
            assert low & M29 == 0
        else:
            t.append(low & M29)
        carry = high + (low >> 29)
        assert carry < 1 << 37
    assert carry < 1 << 32
    return tuple(t) + (carry,)


def sqr_columns(a):
    """f29_sqr_x2's columns: a_i (2 a_j) for i < j and a_i^2, with the doubled limb below 2^30"""
    a2 = [2 * v for v in a]
    assert all(v < 1 << 30 for v in a2)
    cols = [0] * 27
    for k in range(27):
        for i in range(0 if k < 14 else k - 13, 14):
            if 2 * i < k:
                cols[k] += a[i] * a2[k - i]
        if k % 2 == 0:
            cols[k] += a[k // 2] ** 2
        assert cols[k] <= 15 << 58
    return cols


def f29_sub(a, b, k):
    """f29_sub<K>: a - b + K p by the borrow chain, limbs normalized, the top limb whatever is left"""
    kp = fc.limbs29(k * P)
    out, c = [], 0
    for i in range(13):
        t = a[i] - b[i] + kp[i] + c
        out.append(t & M29)
        c = t >> 29  # arithmetic
    top = a[13] - b[13] + kp[13] + c
    assert 0 <= top < 1 << 32
    return tuple(out) + (top,)


# ------------------------------------------------------------------ the lane pair (PairOps<FP29A, true>)
def prep(b0, b1):
    """(y1, y2) of the even lane, (y1, y2) of the odd lane for the second operand b = (b0, b1)"""
    y2e = tuple(K16[i] - b1[i] for i in range(14))
    assert all(0 <= v < 1 << 30 for v in y2e)
    return (tuple(b0), y2e), (tuple(b0), tuple(b1))


def pair_mul(a, b, form="joined"):
    """words of the even and of the odd lane"""
    (e1, e2), (o1, o2) = prep(*b)
    return (redc(columns([(a[0], e1), (a[1], e2)]), form=form), redc(columns([(a[1], o1), (a[0], o2)]), form=form))


def pair_mul_sum(a, b, c, d, form="joined"):
    (e1, e2), (o1, o2) = prep(*b)
    (f1, f2), (q1, q2) = prep(*d)
    return (redc4([(a[0], e1), (a[1], e2), (c[0], f1), (c[1], f2)], form),
            redc4([(a[1], o1), (a[0], o2), (c[1], q1), (c[0], q2)], form))


def pair_sqr(a, kb, form="joined"):
    """even: (a0 + a1 by limbs) x (a0 - a1 + KB p); odd: a0 x (a1 + a1 by limbs)"""
    a0, a1 = a
    xe = tuple(u + v for u, v in zip(a0, a1))
    ye = f29_sub(a0, a1, kb)
    yo = tuple(2 * v for v in a1)
    assert all(v < 1 << 30 for v in xe + yo)
    return redc(columns([(xe, ye)]), form=form), redc(columns([(a0, yo)]), form=form)


# ------------------------------------------------------------------ operands
def L(x):
    return fc.limbs29(x)


def values(k, few=False):
    """values below k p as limb tuples: the edges of tests/field_cases.py"""
    xs = fc.keys29(k, few=True) if few else fc.edges29(k)
    return [L(x) for x in xs]


def wide_operands():
    """operands with limbs up to 2^30 (fc.nonnorm_ops: k16 - z for edge z < 8p, all-ones), and the
    doubled all-ones operand 2^30 - 2 per limb"""
    return fc.nonnorm_ops() + [tuple([(1 << 30) - 2] * 13 + [0x60])]


def rnd(rng, k):
    return L(rng.randrange(k * P))


def cases_sqr():
    """squares: normalized operands below 16p (P < 10p and R < 6p in x29_madd)"""
    rng = random.Random(SEED)
    xs = values(16) + [tuple([M29] * 13 + [0xCF])]
    return [(x,) for x in fc.dedup(xs)] + [(rnd(rng, 16),) for _ in range(1500)]


def cases_mul():
    rng = random.Random(SEED + 1)
    E, K = values(16), values(16, few=True)
    out = list(itertools.product(E, K)) + list(itertools.product(K, E))
    out += [(a, w) for a in K for w in wide_operands()]  # one factor with 2^30 limbs
    out = fc.dedup(out)
    return out + [(rnd(rng, 16), rnd(rng, 16)) for _ in range(1500)]


def cases_mul2():
    rng = random.Random(SEED + 2)
    K = values(16, few=True)
    W = wide_operands()
    out = list(itertools.product(K, K, K, K))
    out += [(a, b, c, w) for a in K[:3] for b in K[:3] for c in K[:3] for w in W]  # as PairOps::mul feeds it
    out = fc.dedup(out)
    return out + [tuple(rnd(rng, 16) for _ in range(4)) for _ in range(1500)]


def cases_redc4():
    rng = random.Random(SEED + 3)
    K, K8 = values(16, few=True)[:3], values(8, few=True)[:3]
    W = wide_operands()
    Wk = [W[5], W[-3], W[-1], W[0]]
    out = [(a, b, a2, w, c, d, c2, w2) for a, b, a2, c, d, c2 in itertools.product(K[:2], K8[:2], K[:2], K[:2], K8[:2], K[:2])
           for w, w2 in itertools.product(Wk, Wk)]
    out += [(K[0], K8[0], K[1], w, K[1], K8[1], K[0], W[-2]) for w in W]
    out = fc.dedup(out)
    for _ in range(1500):
        out.append((rnd(rng, 16), rnd(rng, 8), rnd(rng, 16), rng.choice(W), rnd(rng, 16), rnd(rng, 8), rnd(rng, 16),
                    rng.choice(W)))
    return out


def elems(k, few=True):
    """Fq2 operands as (c0 limbs, c1 limbs), both coefficients below k p"""
    V = values(k, few)
    Kf = values(k, few=True)[:3]
    return fc.dedup([(a, b) for a in V for b in Kf] + [(b, a) for a in V for b in Kf])


def rnde(rng, k):
    return (rnd(rng, k), rnd(rng, k))


def cases_pair_mul():
    """first operand as loose as x29_madd feeds it (t < 10p), second below 8p"""
    rng = random.Random(SEED + 4)
    A, B = elems(10), elems(8, few=False)
    Ak = A[:4]
    out = fc.dedup([(a, b) for a in Ak for b in B] + [(a, b) for a in A for b in B[:6]])
    return out + [(rnde(rng, 10), rnde(rng, 8)) for _ in range(1000)]


def cases_pair_mul_sum():
    rng = random.Random(SEED + 5)
    A, B = elems(10)[:6], elems(8)[:8]
    out = fc.dedup(list(itertools.product(A[:3], B, A[:3], B[:4])) + list(itertools.product(A, B[:2], A, B[:2])))
    return out + [(rnde(rng, 10), rnde(rng, 8), rnde(rng, 10), rnde(rng, 8)) for _ in range(1000)]


def cases_pair_sqr(kb):
    rng = random.Random(SEED + 6 + kb)
    return [(e,) for e in elems(kb, few=False)] + [(rnde(rng, kb),) for _ in range(1000)]


def cases_prep():
    rng = random.Random(SEED + 9)
    return [(e,) for e in elems(8, few=False)] + [(rnde(rng, 8),) for _ in range(500)]


def S(cols):
    return redc(cols, form="seeded")


def two(cases):
    """cases of a lockstep pair: every case next to the one half the list further"""
    h = len(cases) // 2
    return [a + b for a, b in zip(cases, cases[h:] + cases[:h])]


# name -> (cases, lanes per case, model: case -> tuple of per-lane output word tuples)
def suites():
    return {
        # the lockstep pairs: seeded scans, the same words as the single joined ones
        "f29_sqr_x2": (two(cases_sqr()), 1, lambda c: (S(sqr_columns(c[0])) + S(sqr_columns(c[1])) +
                                                       redc(columns([(c[0], c[0])])) + redc(columns([(c[1], c[1])])),)),
        "f29_mul_x2": (two(cases_mul()), 1, lambda c: (S(columns([c[0:2]])) + S(columns([c[2:4]])),)),
        "f29_mul2_x2": (two(cases_mul2()), 1, lambda c: (S(columns([c[0:2], c[2:4]])) + S(columns([c[4:6], c[6:8]])),)),
        "pair_mul_x2": (two(cases_pair_mul()), 2,
                        lambda c: tuple(x + y for x, y in zip(pair_mul(c[0], c[1], "seeded"), pair_mul(c[2], c[3], "seeded")))),
        "pair_sqr_x2<16,8>": (list(zip((c[0] for c in cases_pair_sqr(16)), itertools.cycle(c[0] for c in cases_pair_sqr(8)))), 2,
                              lambda c: tuple(x + y for x, y in zip(pair_sqr(c[0], 16, "seeded"), pair_sqr(c[1], 8, "seeded")))),
        "f29_mul": (cases_mul(), 1, lambda c: (redc(columns([c])),)),
        "f29_mul2": (cases_mul2(), 1, lambda c: (redc(columns([c[0:2], c[2:4]])),)),
        "f29_redc_sum4": (cases_redc4(), 1, lambda c: (redc4([c[0:2], c[2:4], c[4:6], c[6:8]]),)),
        "pair_mul": (cases_pair_mul(), 2, lambda c: pair_mul(*c)),
        "pair_mul_sum": (cases_pair_mul_sum(), 2, lambda c: pair_mul_sum(*c)),
        "pair_sqr_b<8>": (cases_pair_sqr(8), 2, lambda c: pair_sqr(c[0], 8)),
        "pair_sqr_b<16>": (cases_pair_sqr(16), 2, lambda c: pair_sqr(c[0], 16)),
        "pair_prep": (cases_prep(), 2, lambda c: tuple(y1 + y2 for y1, y2 in prep(*c[0]))),
    }


def rows(name, case):
    """input rows (one per lane) of a case"""
    if not name.startswith("pair_"):
        return [[w for x in case for w in x]]
    return [[w for e in case for w in e[lane]] for lane in (0, 1)]
