"""Operands, preconditions and big-integer references for the device field / curve functions that
tests/native/field_ops.hip wraps (tests/test_gpu_field_ops.py runs them, tests/test_field_cases.py
checks this module on the CPU).

Everything here is plain Python `int` arithmetic mod p (BLS12-381 base field) and mod r (scalar
field): Fq2 as pairs, textbook affine addition / doubling for y^2 = x^3 + b. Nothing is taken from
the kernels' formulas. A Suite is one wrapped op with
  cases   operand tuples (raw values as the device sees them: Montgomery form, lazy representatives),
  pre     the documented precondition of the op, per case (the CPU test asserts it for every case, so
          a GPU failure is the kernel's and not the input's),
  check   compares the raw device output of one case with the reference; returns None or a message.
The directed operands sit on the bounds the headers document (ff29.hpp, fq2pair.hpp, curve29.hpp):
a change to a bound there has to change the tables here with it. The "xyzz" family is the 32-bit-limb
XYZZ layer of curve_dev.hpp (preprocessing, keygen, the batch verifier's combinations): canonical
words in and out, every branch of its formulas named by a tag on the cases aimed at it.
"""
import itertools
import random
from functools import lru_cache

P = 0x1A0111EA397FE69A4B1BA7B6434BACD764774B84F38512BF6730D2A0F6B0F6241EABFFFEB153FFFFB9FEFFFFFFFFAAAB
R = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001
M29 = (1 << 29) - 1
R29 = 1 << 406  # Montgomery radix of the radix-2^29 layer
R29I = pow(R29, -1, P)
RQ = 1 << 384  # Montgomery radices of the 32-bit layer
RR = 1 << 256
CAP = 65536
SEED = 0x29F1E1D


# ------------------------------------------------------------------ limbs and words
@lru_cache(maxsize=None)
def limbs29(x):
    """14 limbs: thirteen of 29 bits and the rest in the top one"""
    assert 0 <= x < 1 << (377 + 32)
    return tuple((x >> (29 * i)) & M29 for i in range(13)) + (x >> 377,)


def val29(l):
    return sum(int(v) << (29 * i) for i, v in enumerate(l))


def as_limbs(x):
    return limbs29(x) if isinstance(x, int) else tuple(x)


def as_val(x):
    return x if isinstance(x, int) else val29(x)


@lru_cache(maxsize=None)
def words(x, n):
    assert 0 <= x < 1 << (32 * n)
    return tuple((x >> (32 * i)) & 0xFFFFFFFF for i in range(n))


def val32(w):
    return sum(int(v) << (32 * i) for i, v in enumerate(w))


def normalized(l):
    return all(0 <= v <= M29 for v in l[:13]) and 0 <= l[13] < 1 << 29


# ------------------------------------------------------------------ directed operand sets
def dedup(xs):
    seen, out = set(), []
    for x in xs:
        if x not in seen:
            seen.add(x)
            out.append(x)
    return out


def canon_edges(p, n):
    """canonical (< p) operands of the 32-bit layer, n words"""
    mont = 1 << (32 * n)
    top = p >> (32 * (n - 1))
    low_ones = (1 << (32 * (n - 1))) - 1
    xs = [0, 1, 2, p - 1, p - 2, (p + 1) // 2, (p - 1) // 2, mont % p, mont * mont % p]
    xs += [low_ones, ((top - 1) << (32 * (n - 1))) | low_ones]
    for k in range(n):
        limb = (p >> (32 * k)) & 0xFFFFFFFF
        xs += [p - (limb << (32 * k)), p - (1 << (32 * k)), 1 << (32 * k), (1 << (32 * k)) - 1]
        if limb:
            xs.append(p - (limb << (32 * k)) + ((limb - 1) << (32 * k)))
    return dedup(x for x in xs if 0 <= x < p)


def all_ones29(bound):
    """thirteen low limbs 2^29 - 1 under the largest top limb that keeps the value < bound"""
    low = (1 << 377) - 1
    top = bound >> 377
    if (top << 377) | low >= bound:
        top -= 1
    return (top << 377) | low if top >= 0 else None


def edges29(k):
    """operands of the radix-2^29 layer below k p (k any positive integer)"""
    b = k * P
    xs = [0, 1, P - 1, P, P + 1, b - 1, b - 2]
    for j in range(k):
        xs += [j * P, j * P + 1, j * P - 1]
    xs.append(all_ones29(b))
    for i in range(14):
        xs += [1 << (29 * i), (1 << (29 * i)) - 1]
    return dedup(x for x in xs if x is not None and 0 <= x < b)


def keys29(k, few=False):
    b = k * P
    xs = [b - 1, all_ones29(b), 0, P, 1]
    if not few:
        xs += [P - 1, b - P + 1, (1 << 377) - 1]
    return dedup(x for x in xs if x is not None and 0 <= x < b)


def rand29(rng, k):
    return rng.randrange(k * P)


def star(lists, keys, cap=CAP):
    """every operand of every position against every combination of the other positions' keys, and
    the full cross product where it fits"""
    n = len(lists)
    total = 1
    for l in lists:
        total *= len(l)
    out = []
    if total <= cap // 2:
        out = list(itertools.product(*lists))
    else:
        out = list(itertools.product(*keys))
        for pos in range(n):
            others = [keys[i] if i != pos else lists[pos] for i in range(n)]
            out += itertools.product(*others)
    out = dedup(out)
    assert len(out) <= cap, len(out)
    return out


def with_random(cases, gen, count, cap=CAP):
    rng = random.Random(SEED + len(cases))
    room = max(0, min(count, cap - len(cases)))
    return cases + [gen(rng) for _ in range(room)]


class Suite:
    def __init__(self, name, op, form, cases, pre, check, group=1, kind="raw", operands=None):
        self.name, self.op, self.form, self.cases, self.pre, self.check = name, op, form, cases, pre, check
        self.group = group  # lane groups that hold the same operands (split ops: 2)
        self.kind = kind  # how the test hands the output to check: raw words, "q", "qpred", "point"
        self.operands = operands or (lambda c: list(c))  # the part of a case that goes to the device
        assert 0 < len(cases) <= CAP, (name, len(cases))


def bound_err(v, limbs, kb, what=""):
    if not normalized(limbs):
        return "%s limbs not normalized: %s" % (what, [hex(x) for x in limbs])
    if not v < kb * P:
        return "%s value 0x%x not below %d p" % (what, v, kb)
    return None


# ------------------------------------------------------------------ 32-bit layer
def _mont_mul(p, mont):
    inv = pow(mont, -1, p)
    return lambda a, b: a * b * inv % p


# fe_inv<FrCfg> took its exponent as r's low limb minus 2 without the borrow (r's low limb is 1), so
# it raised to r - 2 + 2^32 and every inverse but those of 0 and the Montgomery one was wrong
FR_INV_REGRESSION = [(2,), (RR % R * 2 % R,), (R - 1,)]


def suites32():
    out = []
    rng = random.Random(SEED)
    for name, p, n, mont, opm, opl, opi in (("fr", R, 8, RR, 0, 3, 8), ("fq", P, 12, RQ, 1, 4, 9)):
        E = canon_edges(p, n)
        mm = _mont_mul(p, mont)
        pairs = with_random(list(itertools.product(E, E)), lambda g: (g.randrange(p), g.randrange(p)), 4000)
        in_field = lambda c, p=p: all(0 <= x < p for x in c)

        def chk_mul(c, o, n=n, mm=mm):
            want = words(mm(c[0], c[1]), n)
            if tuple(o[:n]) != want:
                return "asm product differs"
            if tuple(o[n:]) != want:
                return "cios product differs"

        out.append(Suite(name + "_mul_asm_cios", opm, "W%d" % n, pairs, in_field, chk_mul))

        def chk_lin(c, o, n=n, p=p):
            a, b = c
            for k, want in enumerate(((a + b) % p, (a - b) % p, -a % p, 2 * a % p)):
                if tuple(o[k * n:(k + 1) * n]) != words(want, n):
                    return ("add", "sub", "neg", "dbl")[k] + " differs"

        out.append(Suite(name + "_add_sub_neg_dbl", opl, "W%d" % n, pairs, in_field, chk_lin))

        inv_cases = [(x,) for x in E] + [(rng.randrange(p),) for _ in range(64)]
        if n == 8:
            inv_cases = FR_INV_REGRESSION + inv_cases

        def chk_inv(c, o, n=n, p=p, mont=mont):
            want = mont * mont * pow(c[0], -1, p) % p if c[0] else 0
            if tuple(o) != words(want, n):
                return "inverse differs"

        out.append(Suite(name + "_inv", opi, "W%d" % n, inv_cases, in_field, chk_inv))

    # both slots of the two-product form: edge x random, random x edge, edge x edge
    E = canon_edges(R, 8)
    mm = _mont_mul(R, RR)
    K = [0, 1, R - 1, R - 2, (1 << 224) - 1 + (0x73EDA752 << 224), RR % R, (R + 1) // 2, (1 << 32) - 1]
    rr = lambda: (rng.randrange(R), rng.randrange(R))
    x2 = []
    for a, b in itertools.product(E, K):
        x2 += [(a, b) + rr(), rr() + (a, b), (b, a) + rr(), rr() + (b, a)]
    for a, b in itertools.product(K, K):
        x2 += [(a, b, c, d) for c, d in itertools.product(K, K)]
    x2 += [(a, b, b, a) for a, b in itertools.product(E, E)]
    x2 = with_random(x2[:CAP - 4000], lambda g: tuple(g.randrange(R) for _ in range(4)), 4000)

    def chk_x2(c, o):
        if tuple(o[:8]) != words(mm(c[0], c[1]), 8):
            return "slot 0 differs"
        if tuple(o[8:]) != words(mm(c[2], c[3]), 8):
            return "slot 1 differs"

    out.append(Suite("fr_mul_x2", 2, "W8", x2, lambda c: all(0 <= x < R for x in c), chk_x2))

    mont_cases = [(x,) for x in E] + [(rng.randrange(R),) for _ in range(2000)]

    def chk_fr_mont(c, o):
        a = c[0]
        if tuple(o[:8]) != words(a * RR % R, 8):
            return "to_mont differs"
        if tuple(o[8:16]) != words(a * pow(RR, -1, R) % R, 8):
            return "from_mont differs"
        if tuple(o[16:]) != words(a, 8):
            return "round trip differs"

    out.append(Suite("fr_mont", 5, "W8", mont_cases, lambda c: 0 <= c[0] < R, chk_fr_mont))
    qcases = [(x,) for x in canon_edges(P, 12)] + [(rng.randrange(P),) for _ in range(2000)]

    def chk_fq_mont(c, o):
        if tuple(o) != words(c[0] * pow(RQ, -1, P) % P, 12):
            return "from_mont differs"

    out.append(Suite("fq_from_mont", 7, "W12", qcases, lambda c: 0 <= c[0] < P, chk_fq_mont))

    can = [R - 1, R, R + 1, RR - 1, 0, 1, R - 2, R + 2]
    for k in range(8):
        can += [R + (1 << (32 * k)), R - (1 << (32 * k)), R ^ (1 << (32 * k + 31)), R & ~(0xFFFFFFFF << (32 * k))]
    can = dedup(x for x in can if 0 <= x < RR) + [rng.randrange(RR) for _ in range(500)]
    out.append(Suite("fr_is_canonical", 6, "W8", [(x,) for x in can], lambda c: 0 <= c[0] < RR,
                     lambda c, o: None if int(o[0]) == (1 if c[0] < R else 0) else "wrong answer"))

    # Fq2 of the 32-bit layer
    Eq = canon_edges(P, 12)
    Kq = [0, 1, P - 1, RQ % P, ((0x1A0111E9) << 352) | ((1 << 352) - 1)]
    el = dedup([(a, b) for a in Eq for b in Kq] + [(b, a) for a in Eq for b in Kq])
    kel = list(itertools.product(Kq, Kq))
    f2c = dedup(list(itertools.product(el, kel)) + list(itertools.product(kel, el)))[:20000]
    rq2 = lambda g: (g.randrange(P), g.randrange(P))
    f2c = with_random(f2c, lambda g: (rq2(g), rq2(g)), 3000)
    ri = pow(RQ, -1, P)

    def chk_f2(c, o):
        a, b = c
        m = f2_mul(a, b)
        s = f2_mul(a, a)
        want = words(m[0] * ri % P, 12) + words(m[1] * ri % P, 12)
        if tuple(o[:24]) != want:
            return "f2_mul differs"
        if tuple(o[24:]) != words(s[0] * ri % P, 12) + words(s[1] * ri % P, 12):
            return "f2_sqr differs"

    inf2 = lambda c: all(0 <= x < P for e in c for x in e)
    out.append(Suite("f2_mul_sqr", 10, "W24", f2c, inf2, chk_f2))
    inv2 = [(e,) for e in el[:400]] + [(rq2(rng),) for _ in range(32)]

    def chk_f2inv(c, o):
        a = c[0]
        if a == (0, 0):
            want = (0, 0)
        else:
            i = f2_inv(a)
            want = (i[0] * RQ * RQ % P, i[1] * RQ * RQ % P)
        if tuple(o) != words(want[0], 12) + words(want[1], 12):
            return "f2_inv differs"

    out.append(Suite("f2_inv", 11, "W24", inv2, inf2, chk_f2inv))
    return out


# ------------------------------------------------------------------ Fq / Fq2 reference arithmetic
def f2_mul(a, b):
    return ((a[0] * b[0] - a[1] * b[1]) % P, (a[0] * b[1] + a[1] * b[0]) % P)


def f2_inv(a):
    n = pow(a[0] * a[0] + a[1] * a[1], -1, P)
    return (a[0] * n % P, -a[1] * n % P)


class Fld:
    """Fq (deg 1: int) or Fq2 (deg 2: pair), textbook"""

    def __init__(self, deg):
        self.deg = deg
        self.zero = 0 if deg == 1 else (0, 0)
        self.one = 1 if deg == 1 else (1, 0)

    def red(self, a):
        return a % P if self.deg == 1 else (a[0] % P, a[1] % P)

    def add(self, a, b):
        return (a + b) % P if self.deg == 1 else ((a[0] + b[0]) % P, (a[1] + b[1]) % P)

    def sub(self, a, b):
        return (a - b) % P if self.deg == 1 else ((a[0] - b[0]) % P, (a[1] - b[1]) % P)

    def neg(self, a):
        return self.sub(self.zero, a)

    def mul(self, a, b):
        return a * b % P if self.deg == 1 else f2_mul(a, b)

    def inv(self, a):
        return pow(a, -1, P) if self.deg == 1 else f2_inv(a)

    def muli(self, a, k):
        return a * k % P if self.deg == 1 else (a[0] * k % P, a[1] * k % P)

    def coeffs(self, a):
        return (a,) if self.deg == 1 else a

    def from_coeffs(self, c):
        return c[0] if self.deg == 1 else tuple(c)


FQ1, FQ2 = Fld(1), Fld(2)
INF = None


def aff_dbl(F, A):
    """2A on y^2 = x^3 + b (any b), A = (x, y) with y != 0"""
    if A is INF:
        return INF
    x, y = A
    assert y != F.zero
    lam = F.mul(F.muli(F.mul(x, x), 3), F.inv(F.muli(y, 2)))
    x3 = F.sub(F.sub(F.mul(lam, lam), x), x)
    return (x3, F.sub(F.mul(lam, F.sub(x, x3)), y))


def aff_add(F, A, B):
    if A is INF:
        return B
    if B is INF:
        return A
    if A[0] == B[0]:
        return aff_dbl(F, A) if A[1] == B[1] else INF
    lam = F.mul(F.sub(B[1], A[1]), F.inv(F.sub(B[0], A[0])))
    x3 = F.sub(F.sub(F.mul(lam, lam), A[0]), B[0])
    return (x3, F.sub(F.mul(lam, F.sub(A[0], x3)), A[1]))


def aff_neg(F, A):
    return INF if A is INF else (A[0], F.neg(A[1]))


def aff_mul(F, k, A):
    acc = INF
    for bit in bin(k)[2:]:
        acc = aff_dbl(F, acc)
        if bit == "1":
            acc = aff_add(F, acc, A)
    return acc


def to_dev(F, a):
    """canonical radix-2^29 Montgomery form (R = 2^406), per coefficient"""
    return F.from_coeffs([c * R29 % P for c in F.coeffs(a)])


def from_dev(F, v):
    return F.from_coeffs([c * R29I % P for c in F.coeffs(v)])


# ------------------------------------------------------------------ radix-2^29 field ops (one value per lane)
def _redc_check(kb, want_of):
    def chk(c, o):
        v = val29(o)
        e = bound_err(v, o, kb)
        if e:
            return e
        if (v - want_of(c)) % P:
            return "value 0x%x not congruent to the reference" % v

    return chk


def nonnorm_ops():
    """operands with limbs below 2^30, value <= 16p: the borrow-free k16(i) - z_i form (fq2pair.hpp)
    for edge z < 8p, and all-ones low limbs"""
    P16 = limbs29(16 * P)
    k16 = [P16[0] + (1 << 29)] + [P16[i] + (1 << 29) - 1 for i in range(1, 13)] + [P16[13] - 1]
    out = []
    for z in edges29(8):
        zl = limbs29(z)
        out.append(tuple(k16[i] - zl[i] for i in range(14)))
    out.append(tuple([(1 << 30) - 1] * 13 + [0xCD]))  # < 16p with the low limbs' excess
    out.append(tuple([(1 << 30) - 1] * 13 + [0]))
    return out


def redc4_pre(c):
    """f29_redc_sum4's precondition: per chain (products 0, 1 and 2, 3) at most one product with a
    factor whose limbs reach 2^29 (and then < 2^30), every other factor normalized; the sum of the
    four products below 2^406 p"""
    for chain in (c[0:4], c[4:8]):
        wide = 0
        for a, b in (chain[0:2], chain[2:4]):
            la, lb = as_limbs(a), as_limbs(b)
            if not all(0 <= v < 1 << 30 for v in la + lb):
                return False
            na, nb = normalized(la), normalized(lb)
            if not na and not nb:
                return False
            wide += (not na) or (not nb)
        if wide > 1:
            return False
    total = sum(as_val(c[2 * i]) * as_val(c[2 * i + 1]) for i in range(4))
    return total < R29 * P


def suites29():
    out = []
    E16, K16 = edges29(16), keys29(16)
    lt = lambda *ks: (lambda c: all(isinstance(x, int) and 0 <= x < k * P for x, k in zip(c, ks)))

    mul = with_random(star([E16, E16], [K16, K16]), lambda g: (rand29(g, 16), rand29(g, 16)), 4000)
    out.append(Suite("f29_mul", 20, "F29", mul, lt(16, 16), _redc_check(2, lambda c: c[0] * c[1] * R29I)))
    kf = keys29(16, few=True)
    mul2 = with_random(star([E16] * 4, [kf] * 4, CAP - 4000), lambda g: tuple(rand29(g, 16) for _ in range(4)), 4000)
    out.append(Suite("f29_mul2", 21, "F29", mul2, lt(16, 16, 16, 16),
                     _redc_check(2, lambda c: (c[0] * c[1] + c[2] * c[3]) * R29I)))

    # f29_redc_sum4 on its precondition: b1 and b3 (the second product of each chain) carry 2^30 limbs
    NN = nonnorm_ops()
    knn = [NN[i] for i in (5, 6, len(NN) - 2, len(NN) - 1, 0)]  # k16 - (8p - 1), k16 - (8p - 2), all-ones, k16 - 0
    E8, K8 = edges29(8), keys29(8, few=True)
    r4 = []
    ka = [16 * P - 1, all_ones29(16 * P), 0]
    for a in E16:  # every a against the worst partners
        for kk in ka:
            r4.append((a, K8[0], kk, knn[0], kk, K8[1], a, knn[2]))
            r4.append((kk, K8[1], a, knn[2], a, K8[0], kk, knn[1]))
    for b in E8:
        for kk in ka[:2]:
            r4.append((kk, b, kk, knn[2], kk, b, kk, knn[0]))
    for y in NN:
        for kk in ka[:2]:
            r4.append((kk, K8[0], kk, y, kk, K8[1], kk, knn[2]))
            r4.append((kk, K8[1], kk, knn[2], kk, K8[0], kk, y))
    # the wide factor in the other slots a chain allows: first product's factor, or the a side
    r4.append((ka[1], knn[2], ka[1], K8[1], ka[1], K8[1], ka[1], knn[2]))
    r4.append((knn[2], ka[1], ka[1], K8[1], ka[1], K8[1], knn[2], ka[1]))
    r4 += list(itertools.product(ka, K8[:2], ka, knn[:3], ka, K8[:2], ka, knn[:3]))
    rng = random.Random(SEED + 4)
    for _ in range(4000):
        ys = [rng.choice(NN) if rng.random() < .5 else tuple(rng.randrange(1 << 30) for _ in range(13)) + (rng.randrange(0xC0),)
              for _ in range(2)]
        r4.append((rand29(rng, 16), rand29(rng, 8), rand29(rng, 16), ys[0], rand29(rng, 16), rand29(rng, 8),
                   rand29(rng, 16), ys[1]))
    r4 = dedup(r4)[:CAP]
    out.append(Suite("f29_redc_sum4", 22, "F29", r4, redc4_pre,
                     _redc_check(2, lambda c: sum(as_val(c[2 * i]) * as_val(c[2 * i + 1]) for i in range(4)) * R29I)))

    add = with_random(star([E8, E8], [K8, K8]), lambda g: (rand29(g, 8), rand29(g, 8)), 2000)

    def chk_add(c, o):
        v = val29(o)
        return bound_err(v, o, 16) or (None if v == c[0] + c[1] else "sum differs")

    out.append(Suite("f29_add", 23, "F29", add, lt(8, 8), chk_add))
    for op, k in ((24, 2), (25, 4), (26, 8), (27, 16)):
        Ek = edges29(k)
        sub = with_random(star([E16, Ek], [K16, keys29(k)]), lambda g, k=k: (rand29(g, 16), rand29(g, k)), 2000)

        def chk_sub(c, o, k=k):
            v = val29(o)
            return bound_err(v, o, 16 + k) or (None if v == c[0] - c[1] + k * P else "difference differs")

        out.append(Suite("f29_sub<%d>" % k, op, "F29", sub, lt(16, k), chk_sub))
    for op, k in ((28, 1), (29, 2), (30, 4), (31, 8)):
        cs = [(x,) for x in edges29(2 * k)] + [(rand29(rng, 2 * k),) for _ in range(2000)]

        def chk_csub(c, o, k=k):
            v = val29(o)
            return bound_err(v, o, k) or (None if v == (c[0] - k * P if c[0] >= k * P else c[0]) else "wrong value")

        out.append(Suite("f29_csub<%d>" % k, op, "F29", cs, lt(2 * k), chk_csub))
    cn = [(x,) for x in edges29(2)] + [(rand29(rng, 2),) for _ in range(2000)]
    out.append(Suite("f29_canon", 32, "F29", cn, lt(2),
                     lambda c, o: bound_err(val29(o), o, 1) or (None if val29(o) == c[0] % P else "not the canonical value")))
    for op, k in ((33, 4), (34, 8), (35, 16)):
        rd = [(x,) for x in edges29(k)] + [(rand29(rng, k),) for _ in range(2000)]
        out.append(Suite("f29_reduce<%d>" % k, op, "F29", rd, lt(k), _redc_check(2, lambda c: c[0])))

    out.append(Suite("f29_predicates", 36, "F29", [(x,) for x in pred_values()], lt(16), chk_pred_f29))

    pk = [(x,) for x in edges29(8)] + [(rand29(rng, 8),) for _ in range(2000)]

    def chk_pack(c, o):
        if tuple(o[:12]) != words(c[0], 12):
            return "packed words differ"
        if tuple(o[12:]) != limbs29(c[0]):
            return "round trip differs"

    out.append(Suite("f29_pack_unpack", 37, "F29", pk, lt(8), chk_pack))
    up = [x for x in pk] + [((1 << 384) - 1,), (1 << 383,), ((1 << 384) - (1 << 377),)]
    up += [(rng.randrange(1 << 384),) for _ in range(1000)]
    out.append(Suite("f29_unpack", 38, "W12", up, lambda c: 0 <= c[0] < 1 << 384,
                     lambda c, o: None if tuple(o) == limbs29(c[0]) else "limbs differ"))
    return out


PRED_BOUNDS = (2, 4, 4, 8, 16)  # zero2, zero4, zero_lt<4>, zero_lt<8>, zero_lt<16>: x < this many p


def pred_values():
    """multiples of p, their neighbours, and values that share limb 0 with a multiple of p but
    differ elsewhere; all < 16p"""
    xs = list(edges29(16))
    for j in range(16):
        jp = j * P
        xs.append(jp & M29)  # limb 0 alone
        for i in range(1, 14):
            xs += [jp ^ (1 << (29 * i)), jp + (1 << (29 * i)), jp ^ (1 << (29 * i + 28))]
        if j:
            xs += [jp - (1 << 29), jp - P + (P & M29) - ((jp - P) & M29)]
    rng = random.Random(SEED + 9)
    for _ in range(1000):
        j = rng.randrange(16)
        xs.append(((rng.randrange(16 * P) >> 29) << 29 | (j * P & M29)))
    xs += [rand29(rng, 16) for _ in range(1000)]
    return dedup(x for x in xs if 0 <= x < 16 * P)


def chk_pred_f29(c, o):
    x = c[0]
    for k, b in enumerate(PRED_BOUNDS):
        if x < b * P and int(o[k]) != (1 if x % P == 0 else 0):
            return "predicate %d (x < %d p) gave %d" % (k, b, o[k])
    if int(o[5]) != (1 if x == 0 else 0):
        return "is_zero_raw gave %d" % o[5]


# ------------------------------------------------------------------ the three Fq2 forms
Q_FORMS = (("F2_29", 40, "F2"), ("FP29", 50, "PAIR"), ("FP29A", 60, "PAIR"))


def elems29(k, few=False):
    """Fq2 operands with both coefficients below k p: every edge in one coefficient against the keys
    in the other"""
    E, K = edges29(k), keys29(k, few)
    return dedup([(a, b) for a in E for b in K] + [(b, a) for a in E for b in K])


def kelems29(k):
    K = keys29(k, few=True)[:3]
    return list(itertools.product(K, K))


def rande(k):
    return lambda g: (rand29(g, k), rand29(g, k))


def chk_q(kb, want_of):
    def chk(c, o):
        for i in (0, 1):
            v = val29(o[i])
            e = bound_err(v, o[i], kb, "c%d" % i)
            if e:
                return e
        got = (val29(o[0]) % P, val29(o[1]) % P)
        w = want_of(c)
        if got != (w[0] % P, w[1] % P):
            return "not congruent to the reference"

    return chk


def q_ri(a):
    return (a[0] * R29I % P, a[1] * R29I % P)


def suitesq():
    out = []
    ltq = lambda *ks: (lambda c: all(0 <= x < k * P for e, k in zip(c, ks) for x in e))
    E8 = elems29(8)
    mul = with_random(star([E8, E8], [kelems29(8)] * 2, 40000), lambda g: (rande(8)(g), rande(8)(g)), 3000)
    for name, base, form in Q_FORMS:
        out.append(Suite(name + "_mul", base, form, mul, ltq(8, 8), chk_q(2, lambda c: q_ri(f2_mul(c[0], c[1]))), kind="q"))
        # first operands as loose as x29_madd feeds them to the fused form (t < 10p); second operands'
        # odd-lane coefficient up to 8p - 1 (k16's top limb)
        ka = 10 if name == "FP29A" else 8
        Ea = elems29(ka, few=True)
        kaf = [(ka * P - 1, ka * P - 1), (all_ones29(ka * P), ka * P - 1)]
        E8f = elems29(8, few=True)
        k8s = [(8 * P - 1, 8 * P - 1), (0, 8 * P - 1)]
        ms = star([Ea, E8f, Ea, E8f], [kaf, k8s, kaf, k8s], 30000)
        ms = with_random(ms, lambda g, ka=ka: (rande(ka)(g), rande(8)(g), rande(ka)(g), rande(8)(g)), 3000)

        def want_ms(c):
            x, y = f2_mul(c[0], c[1]), f2_mul(c[2], c[3])
            return q_ri(((x[0] + y[0]) % P, (x[1] + y[1]) % P))

        out.append(Suite(name + "_mul_sum", base + 1, form, ms, ltq(ka, 8, ka, 8),
                         chk_q(2 if name == "FP29A" else 4, want_ms), kind="q"))
        for sub, kb in ((2, 8), (3, 16)):
            sq = [(e,) for e in elems29(kb)]
            sq = with_random(sq, lambda g, kb=kb: (rande(kb)(g),), 3000)
            out.append(Suite("%s_sqr_b<%d>" % (name, kb), base + sub, form, sq, ltq(kb),
                             chk_q(2, lambda c: q_ri(f2_mul(c[0], c[0]))), kind="q"))
        # one, and the pair-combined predicates: both coefficients from the predicate values, with
        # exactly one of them a multiple of p among the cases
        pv = pred_values()
        zs = [j * P for j in range(16)]
        pe = dedup([(z, x) for x in pv[:400] for z in (0, P, 3 * P, 7 * P, 15 * P)] +
                   [(x, z) for x in pv[:400] for z in (0, P, 3 * P, 7 * P, 15 * P)] +
                   list(itertools.product(zs, zs)) + [(x, x) for x in pv])

        def chk_pred(c, o):
            one, flags = o
            e = chk_q(2, lambda c: (R29 % P, 0))(c, one)
            if e:
                return "one: " + e
            x = c[0]
            for lane in flags:
                for k, b in enumerate(PRED_BOUNDS):
                    if max(x) < b * P and int(lane[k]) != (1 if x[0] % P == 0 and x[1] % P == 0 else 0):
                        return "predicate %d (x < %d p) gave %d" % (k, b, lane[k])
                if int(lane[5]) != (1 if x == (0, 0) else 0):
                    return "is_zero_raw gave %d" % lane[5]

        out.append(Suite(name + "_one_predicates", base + 4, form, [(e,) for e in pe], ltq(16), chk_pred, kind="qpred"))
    return out


# ------------------------------------------------------------------ curve formulas
def coord_reps(F, v, kb, which):
    """representatives of a field element per coefficient; `which` picks one combination index"""
    cs = F.coeffs(v)
    return F.from_coeffs([c + ((which >> (4 * i)) % kb) * P for i, c in enumerate(cs)])


def xyzz(F, A, s, jx=0, jy=0, jzz=0, jzzz=0, kx=8, ky=4):
    """XYZZ (device form) of the affine point A scaled by s: X = x s^2, Y = y s^3, ZZ = s^2,
    ZZZ = s^3, shifted to the representatives picked by jx .. jzzz"""
    s2 = F.mul(s, s)
    s3 = F.mul(s2, s)
    X, Y = to_dev(F, F.mul(A[0], s2)), to_dev(F, F.mul(A[1], s3))
    return (coord_reps(F, X, kx, jx), coord_reps(F, Y, ky, jy), coord_reps(F, to_dev(F, s2), 2, jzz),
            coord_reps(F, to_dev(F, s3), 2, jzzz))


def inf_xyzz(F, A):
    """infinity as the kernels hold it: ZZ == 0 literally, the other coordinates arbitrary"""
    z = F.zero
    return (to_dev(F, A[0]), to_dev(F, A[1]), z, to_dev(F, A[1]))


def edge_field(F, rng, i):
    """field elements whose DEVICE form is an edge value: canonical edges, per coefficient"""
    E = [x for x in edges29(1) if x]
    pick = lambda k: E[k % len(E)]
    if F.deg == 1:
        return from_dev(F, pick(i))
    return from_dev(F, (pick(i), pick(i * 7 + 3) if i % 3 else 0))


def base_points(F, rng, n, edge=None):
    """(x, y) with y != 0, on the curve with b = y^2 - x^3: edge device coordinates and random ones"""
    edge = edge or edge_field
    pts = []
    i = 0
    while len(pts) < n:
        if i < 2 * n // 3:
            A = (edge(F, rng, 5 * i + 1), edge(F, rng, 11 * i + 2))
        else:
            A = (F.from_coeffs([rng.randrange(P) for _ in range(F.deg)]),
                 F.from_coeffs([rng.randrange(1, P) for _ in range(F.deg)]))
        i += 1
        if A[1] == F.zero:
            continue
        try:  # multiples used below must exist and avoid y == 0 (points of order two: out of scope)
            ms = [aff_mul(F, k, A) for k in (2, 3, 4, 5, 6)]
        except (AssertionError, ValueError):
            continue
        if any(m is INF or m[1] == F.zero for m in ms):
            continue
        pts.append(A)
    return pts


def scalars_s(F, rng):
    E = [1, 2, P - 1, from_dev(FQ1, all_ones29(P)), from_dev(FQ1, 1), from_dev(FQ1, P - 1)]
    if F.deg == 1:
        return E + [rng.randrange(1, P)]
    return [(E[0], 0), (0, E[2]), (E[3], E[4]), (E[5], E[3]), (rng.randrange(P), rng.randrange(1, P))]


def all_rep_idx(F, kb):
    """indices for coord_reps covering every representative of every coefficient"""
    return [a | (b << 4) for a in range(kb) for b in (range(kb) if F.deg == 2 else (0,))]


def point_pre(F, p, kx, ky):
    return (all(0 <= c < kx * P for c in F.coeffs(p[0])) and all(0 <= c < ky * P for c in F.coeffs(p[1])) and
            all(0 <= c < 2 * P for c in F.coeffs(p[2]) + F.coeffs(p[3])))


def check_point(F, o, want, kx, ky):
    """o: device X, Y, ZZ, ZZZ as limb rows per coefficient; want: affine point or INF"""
    vals = []
    for name, rows, kb in zip(("X", "Y", "ZZ", "ZZZ"), o, (kx, ky, 2, 2)):
        cs = []
        for r in rows:
            v = val29(r)
            e = bound_err(v, r, kb, name)
            if e:
                return e
            cs.append(v)
        vals.append(cs)
    if want is INF:
        return None if all(v == 0 for v in vals[2]) else "expected infinity as a literal ZZ == 0"
    X, Y, ZZ, ZZZ = (from_dev(F, F.from_coeffs([v % P for v in cs])) for cs in vals)
    if ZZ == F.zero or ZZZ == F.zero:
        return "unexpected infinity / zero ZZ, ZZZ"
    if F.mul(F.mul(ZZ, ZZ), ZZ) != F.mul(ZZZ, ZZZ):
        return "ZZ^3 != ZZZ^2"
    got = (F.mul(X, F.inv(ZZ)), F.mul(Y, F.inv(ZZZ)))
    return None if got == (F.red(want[0]), F.red(want[1])) else "affine point differs from the reference"


def madd_cases(F, n_pts):
    """(acc, ax, ay, neg, want): generic additions, P + P through every representative pair,
    P + (-P), infinity accumulator"""
    rng = random.Random(SEED + 17 + F.deg)
    cases = []
    ridx_x, ridx_y = all_rep_idx(F, 8), all_rep_idx(F, 4)
    for ia, A in enumerate(base_points(F, rng, n_pts)):
        mult = {k: aff_mul(F, k, A) for k in range(1, 7)}
        ss = scalars_s(F, rng)
        for t, (k, m) in enumerate(((1, 2), (2, 1), (3, 2), (1, 4), (5, 1))):
            for neg in (0, 1):
                B = mult[m]
                Bin = aff_neg(F, B) if neg else B  # the kernel negates it back
                s = ss[(t + neg) % len(ss)]
                jx, jy = rng.choice(ridx_x), rng.choice(ridx_y)
                acc = xyzz(F, mult[k], s, jx, jy, rng.randrange(2) * 0x11, rng.randrange(2) * 0x11)
                cases.append((acc, to_dev(F, Bin[0]), to_dev(F, Bin[1]), neg, aff_add(F, mult[k], B)))
        # generic additions with X at its extreme representatives per coefficient (P = U2 - X + 8p then
        # spans its whole documented range, up to 10p in one coefficient next to 0 in the other)
        for jx in dedup([0, ridx_x[-1], ridx_x[-1] & 0x0F, ridx_x[-1] & 0xF0]):
            for jy in (0, ridx_y[-1]):
                acc = xyzz(F, mult[2], ss[jx % len(ss)], jx, jy)
                cases.append((acc, to_dev(F, mult[3][0]), to_dev(F, mult[3][1]), 0, mult[5]))
        # loosest accumulator everywhere, generic
        acc = xyzz(F, mult[3], ss[0], 0x77, 0x33, 0x11, 0x11)
        cases.append((acc, to_dev(F, mult[1][0]), to_dev(F, mult[1][1]), 0, mult[4]))
        # P + P and P + (-P): every representative of X and of Y
        for k in (1, 2):
            B = mult[k]
            s = ss[k % len(ss)]
            for jx in ridx_x:
                for jy in ridx_y if ia == 0 or jx in (0, ridx_x[-1]) else (ridx_y[jx % len(ridx_y)],):
                    for neg in (0, 1):
                        for same in (True, False):
                            Bk = B if same else aff_neg(F, B)  # what the kernel ends up adding
                            Bin = aff_neg(F, Bk) if neg else Bk
                            acc = xyzz(F, B, s, jx, jy, (jx & 1) * 0x11, (jy & 1) * 0x11)
                            cases.append((acc, to_dev(F, Bin[0]), to_dev(F, Bin[1]), neg,
                                          aff_dbl(F, B) if same else INF))
        for jy in ridx_y:  # every Y representative with the plain X as well
            acc = xyzz(F, mult[1], ss[-1], 0, jy)
            cases.append((acc, to_dev(F, A[0]), to_dev(F, A[1]), 0, mult[2]))
        for neg in (0, 1):
            Bin = aff_neg(F, A) if neg else A
            cases.append((inf_xyzz(F, mult[2]), to_dev(F, Bin[0]), to_dev(F, Bin[1]), neg, A))
    if F.deg == 2:
        cases += madd_wide_p_cases(F, rng)
    return cases


def wide_p_gap(F, c):
    """for an x29_madd<Fq2> case: P.c1 - P.c0 of P = U2 - X + 8p, with U2 = ax ZZ taken canonical (a REDC
    of operands of a few p is below p (1 + 2^-20): R = 2^406 against p < 2^381)"""
    acc, ax = c[0], c[1]
    u = to_dev(F, F.mul(from_dev(F, ax), from_dev(F, F.red(acc[2]))))
    return (u[1] - acc[0][1]) - (u[0] - acc[0][0])


def madd_wide_p_cases(F, rng, count=16):
    """generic Fq2 additions with P.c1 - P.c0 > 8p (X.c0 at x + 7p, X.c1 at x, and U2 to match): the
    square of P needs a0 - a1 + 16p, 8p is not enough (sqr_b<16> in x29_madd)"""
    out = []
    while len(out) < count:
        A = ((rng.randrange(P), rng.randrange(P)), (rng.randrange(P), rng.randrange(1, P)))
        s = (rng.randrange(P), rng.randrange(1, P))
        try:
            B = aff_dbl(F, A)
            C = aff_add(F, B, A)
        except (AssertionError, ValueError):
            continue
        c = (xyzz(F, B, s, 0x07, rng.randrange(4), 0, 0), to_dev(F, A[0]), to_dev(F, A[1]), 0, C)
        if wide_p_gap(F, c) > 8 * P + (P >> 8):
            out.append(c)
    return out


def add_cases(F, n_pts, kx, ky):
    """(p, q, want, loose) for x29_add / x29_add_split. loose: one side is infinity, so the other is
    returned as it came, with the loose input bounds (X < 8p, Y < 4p) instead of < 2p"""
    rng = random.Random(SEED + 31 + F.deg)
    cases = []
    ridx_x, ridx_y = all_rep_idx(F, kx), all_rep_idx(F, ky)
    for A in base_points(F, rng, n_pts):
        mult = {k: aff_mul(F, k, A) for k in range(1, 7)}
        ss = scalars_s(F, rng)
        pick = lambda: (rng.choice(ridx_x), rng.choice(ridx_y), rng.randrange(2) * 0x11, rng.randrange(2) * 0x11)
        for t, (k, m) in enumerate(((1, 2), (2, 1), (3, 2), (1, 4), (5, 1))):
            p = xyzz(F, mult[k], ss[t % len(ss)], *pick(), kx=kx, ky=ky)
            q = xyzz(F, mult[m], ss[(t + 2) % len(ss)], *pick(), kx=kx, ky=ky)
            cases.append((p, q, aff_add(F, mult[k], mult[m]), False))
        for jx in ridx_x[::max(1, len(ridx_x) // 8)] + [ridx_x[-1]]:
            for jy in ridx_y[::max(1, len(ridx_y) // 4)] + [ridx_y[-1]]:
                for same in (True, False):
                    p = xyzz(F, mult[2], ss[1], jx, jy, 0x11, 0, kx=kx, ky=ky)
                    B = mult[2] if same else aff_neg(F, mult[2])
                    q = xyzz(F, B, ss[2], ridx_x[-1] - jx if F.deg == 1 else jx ^ 0x11 if kx > 1 else 0, jy, 0, 0x11,
                             kx=kx, ky=ky)
                    cases.append((p, q, aff_dbl(F, mult[2]) if same else INF, False))
        p = xyzz(F, mult[3], ss[0], *pick(), kx=kx, ky=ky)
        cases.append((p, inf_xyzz(F, A), mult[3], True))
        cases.append((inf_xyzz(F, A), p, mult[3], True))
        cases.append((inf_xyzz(F, A), inf_xyzz(F, mult[2]), INF, True))
    return cases


def dbl_cases(F, n_pts, kx, ky):
    rng = random.Random(SEED + 47 + F.deg)
    cases = []
    ridx_x, ridx_y = all_rep_idx(F, kx), all_rep_idx(F, ky)
    for A in base_points(F, rng, n_pts):
        ss = scalars_s(F, rng)
        for k in (1, 2):
            B = aff_mul(F, k, A)
            for jx in ridx_x[::max(1, len(ridx_x) // 8)] + [ridx_x[-1]]:
                for jy in ridx_y:
                    cases.append((xyzz(F, B, ss[(k + jy) % len(ss)], jx, jy, (jx & 1) * 0x11, (jy & 1) * 0x11,
                                       kx=kx, ky=ky), aff_dbl(F, B)))
        cases.append((inf_xyzz(F, A), INF))
    return cases


def aff_dbl_cases(F, n_pts):
    rng = random.Random(SEED + 59 + F.deg)
    cases = []
    ridx = all_rep_idx(F, 2)
    for A in base_points(F, rng, n_pts):
        for B in (A, aff_mul(F, 2, A), aff_neg(F, A)):
            for jx in ridx:
                for jy in ridx:
                    cases.append((coord_reps(F, to_dev(F, B[0]), 2, jx), coord_reps(F, to_dev(F, B[1]), 2, jy),
                                  aff_dbl(F, B)))
    return cases


def suitesc():
    out = []
    for name, F, base, form in (("F29", FQ1, 80, "F29"), ("FP29A", FQ2, 90, "PAIR")):
        n = 24 if F.deg == 1 else 10
        mc = madd_cases(F, n)
        out.append(Suite("x29_madd<%s>" % name, base, form, mc,
                         lambda c, F=F: point_pre(F, c[0], 8, 4) and all(0 <= v < P for v in F.coeffs(c[1]) + F.coeffs(c[2])),
                         lambda c, o, F=F: check_point(F, o, c[4], 8, 4), kind="point",
                         operands=lambda c: [c[0], c[1], c[2], ("w", c[3])]))
        ad = aff_dbl_cases(F, n)
        out.append(Suite("x29_from_aff_dbl<%s>" % name, base + 1, form, ad,
                         lambda c, F=F: all(0 <= v < 2 * P for v in F.coeffs(c[0]) + F.coeffs(c[1])),
                         lambda c, o, F=F: check_point(F, o, c[2], 2, 2), kind="point", operands=lambda c: list(c[:2])))
        ac = add_cases(F, n, 8, 4)
        out.append(Suite("x29_add<%s>" % name, base + 2, form, ac,
                         lambda c, F=F: point_pre(F, c[0], 8, 4) and point_pre(F, c[1], 8, 4),
                         lambda c, o, F=F: check_point(F, o, c[2], *((8, 4) if c[3] else (2, 2))), kind="point",
                         operands=lambda c: list(c[:2])))
        dc = dbl_cases(F, n, 8, 4)
        out.append(Suite("x29_dbl<%s>" % name, base + 3, form, dc, lambda c, F=F: point_pre(F, c[0], 8, 4),
                         lambda c, o, F=F: check_point(F, o, c[1], 2, 2), kind="point", operands=lambda c: [c[0]]))
    for name, F, base, form in (("F29", FQ1, 100, "F29"), ("FP29", FQ2, 102, "PAIR")):
        n = 24 if F.deg == 1 else 10
        ac = add_cases(F, n, 8, 4)
        out.append(Suite("x29_add_split<%s>" % name, base, form, ac,
                         lambda c, F=F: point_pre(F, c[0], 8, 4) and point_pre(F, c[1], 8, 4),
                         lambda c, o, F=F: check_point(F, o, c[2], *((8, 4) if c[3] else (2, 2))), group=2,
                         kind="point",
                         operands=lambda c: list(c[:2])))
        dc = dbl_cases(F, n, 8, 4)
        out.append(Suite("x29_dbl_split<%s>" % name, base + 1, form, dc, lambda c, F=F: point_pre(F, c[0], 8, 4),
                         lambda c, o, F=F: check_point(F, o, c[1], 2, 2), group=2, kind="point",
                         operands=lambda c: [c[0]]))
    return out


# ------------------------------------------------------------------ 32-bit-limb XYZZ layer (curve_dev.hpp)
# One whole point per lane, Montgomery R = 2^384, every coordinate canonical on the way in and on the
# way out (the 32-bit layer returns canonical words). A case ends with the reference point and a tag
# naming the branch it is aimed at (tests/test_field_cases.py asserts that every tag is present).
RQI = pow(RQ, -1, P)
MUL_SMALL_K = (0, 1, 2, 3, 1 << 31, (1 << 32) - 1)


def to_dev32(F, a):
    return F.from_coeffs([c * RQ % P for c in F.coeffs(a)])


def from_dev32(F, v):
    return F.from_coeffs([c * RQI % P for c in F.coeffs(v)])


def aff32(F, A):
    return (to_dev32(F, A[0]), to_dev32(F, A[1]))


def edge_field32(F, rng, i):
    """field elements whose Montgomery (R = 2^384) form is an edge value of the 12-word layout"""
    E = [x for x in canon_edges(P, 12) if x]
    pick = lambda k: E[k % len(E)]
    if F.deg == 1:
        return from_dev32(F, pick(i))
    return from_dev32(F, (pick(i), pick(i * 7 + 3) if i % 3 else 0))


def xyzz32(F, A, s):
    """the representative of the affine point A with ZZ = s^2, ZZZ = s^3 (s != 0)"""
    s2 = F.mul(s, s)
    s3 = F.mul(s2, s)
    return tuple(to_dev32(F, v) for v in (F.mul(A[0], s2), F.mul(A[1], s3), s2, s3))


def inf_xyzz32(F, A):
    """infinity: ZZ == 0 literally; X, Y and ZZZ hold something else (only ZZ may be consulted)"""
    return aff32(F, A) + (F.zero, to_dev32(F, A[1]))


def scalars32(F, rng):
    """s of the ZZ-scaled representatives: 1 (ZZ = ZZZ = the Montgomery one, as xyzz_from_aff leaves
    it), small, p - 1, s with an edge Montgomery form, random"""
    E = [1, 2, P - 1, from_dev32(FQ1, 1), from_dev32(FQ1, P - 1)]
    if F.deg == 1:
        return E + [rng.randrange(1, P)]
    return [(1, 0), (0, E[2]), (E[3], E[4]), (E[1], 0), (rng.randrange(P), rng.randrange(1, P))]


def canon32(F, *elems):
    return all(0 <= c < P for e in elems for c in F.coeffs(e))


def fields32(F, o, count):
    """(the first `count` field elements of the flat word list o, None) or (None, message) if a
    coefficient is not canonical"""
    n = 12 * F.deg
    out = []
    for k in range(count):
        cs = [val32(o[n * k + 12 * i:n * k + 12 * i + 12]) for i in range(F.deg)]
        if any(c >= P for c in cs):
            return None, "%s not canonical" % ("X", "Y", "ZZ", "ZZZ")[k % 4]
        out.append(F.from_coeffs(cs))
    return out, None


def check_point32(F, o, want):
    """o: X, Y, ZZ, ZZZ as flat 32-bit words; want: affine point or INF"""
    vals, e = fields32(F, o, 4)
    if e:
        return e
    if want is INF:
        return None if vals[2] == F.zero else "expected infinity as a literal ZZ == 0"
    X, Y, ZZ, ZZZ = (from_dev32(F, v) for v in vals)
    if ZZ == F.zero or ZZZ == F.zero:
        return "unexpected infinity / zero ZZ, ZZZ"
    if F.mul(F.mul(ZZ, ZZ), ZZ) != F.mul(ZZZ, ZZZ):
        return "ZZ^3 != ZZZ^2"
    got = (F.mul(X, F.inv(ZZ)), F.mul(Y, F.inv(ZZZ)))
    return None if got == (F.red(want[0]), F.red(want[1])) else "affine point differs from the reference"


def zmadd_cases(F, n_pts):
    """(acc, ax, ay, neg, want, tag)"""
    rng = random.Random(SEED + 71 + F.deg)
    cases = []
    for A in base_points(F, rng, n_pts, edge_field32):
        mult = {k: aff_mul(F, k, A) for k in range(1, 7)}
        ss = scalars32(F, rng)
        for t, (k, m) in enumerate(((1, 2), (2, 1), (3, 2), (1, 4), (5, 1))):
            for neg in (0, 1):
                B = mult[m]
                Bin = aff_neg(F, B) if neg else B  # the kernel negates it back
                acc = xyzz32(F, mult[k], ss[(t + neg) % len(ss)])
                cases.append((acc,) + aff32(F, Bin) + (neg, aff_add(F, mult[k], B), "generic"))
        for k in (1, 2):  # P + P and P + (-P), the accumulator in every representative
            B = mult[k]
            for s in ss:
                for neg in (0, 1):
                    for same in (True, False):
                        Bk = B if same else aff_neg(F, B)  # what the kernel ends up adding
                        Bin = aff_neg(F, Bk) if neg else Bk
                        cases.append((xyzz32(F, B, s),) + aff32(F, Bin) +
                                     (neg, aff_dbl(F, B) if same else INF, "P + P" if same else "P - P"))
        for neg in (0, 1):
            Bin = aff_neg(F, A) if neg else A
            cases.append((inf_xyzz32(F, mult[2]),) + aff32(F, Bin) + (neg, A, "infinite accumulator"))
    return cases


def zadd_cases(F, n_pts):
    """(p, q, want, tag)"""
    rng = random.Random(SEED + 73 + F.deg)
    cases = []
    for A in base_points(F, rng, n_pts, edge_field32):
        mult = {k: aff_mul(F, k, A) for k in range(1, 7)}
        ss = scalars32(F, rng)
        for t, (k, m) in enumerate(((1, 2), (2, 1), (3, 2), (1, 4), (5, 1))):
            p, q = xyzz32(F, mult[k], ss[t % len(ss)]), xyzz32(F, mult[m], ss[(t + 2) % len(ss)])
            cases.append((p, q, aff_add(F, mult[k], mult[m]), "generic"))
        for i, s in enumerate(ss):  # equal and opposite points in different representatives
            for s2 in (s, ss[(i + 1) % len(ss)]):
                for same in (True, False):
                    B = mult[2] if same else aff_neg(F, mult[2])
                    cases.append((xyzz32(F, mult[2], s), xyzz32(F, B, s2), aff_dbl(F, mult[2]) if same else INF,
                                  "P + P" if same else "P - P"))
        p = xyzz32(F, mult[3], ss[-1])
        cases.append((p, inf_xyzz32(F, A), mult[3], "infinite right"))
        cases.append((inf_xyzz32(F, A), p, mult[3], "infinite left"))
        cases.append((inf_xyzz32(F, A), inf_xyzz32(F, mult[2]), INF, "both infinite"))
    return cases


def zdbl_cases(F, n_pts):
    """(p, want, tag)"""
    rng = random.Random(SEED + 79 + F.deg)
    cases = []
    for A in base_points(F, rng, n_pts, edge_field32):
        for k in (1, 2):
            B = aff_mul(F, k, A)
            for s in scalars32(F, rng):
                cases.append((xyzz32(F, B, s), aff_dbl(F, B), "generic"))
        cases.append((inf_xyzz32(F, A), INF, "infinity"))
    return cases


def zaff_dbl_cases(F, n_pts):
    """(ax, ay, want, tag)"""
    rng = random.Random(SEED + 83 + F.deg)
    cases = []
    for A in base_points(F, rng, n_pts, edge_field32):
        for B in (A, aff_mul(F, 2, A), aff_neg(F, A)):
            cases.append(aff32(F, B) + (aff_dbl(F, B), "generic"))
    return cases


def zmul_small_cases(F, n_pts):
    """(p, k, want, tag)"""
    rng = random.Random(SEED + 89 + F.deg)
    cases = []
    pts = base_points(F, rng, 2 * n_pts, edge_field32)
    done = 0
    for A in pts:
        ks = list(MUL_SMALL_K) + [rng.randrange(4, 1 << 32), rng.randrange(4, 1 << 16)]
        try:  # a multiple of y == 0 on the way (a point of small order on A's own curve): another point
            want = {k: aff_mul(F, k, A) for k in ks}
        except (AssertionError, ValueError):
            continue
        ss = scalars32(F, rng)
        for i, k in enumerate(ks):
            for s in (ss[0], ss[(i + 1) % len(ss)]):
                cases.append((xyzz32(F, A, s), k, want[k], "k = 0" if k == 0 else "generic"))
            cases.append((inf_xyzz32(F, A), k, INF, "infinite point"))
        done += 1
        if done == n_pts:
            break
    assert done == n_pts
    return cases


def zfrom_aff_cases(F, n_pts):
    """(ax, ay, want, tag): want is the point itself, or INF for the (0, 0) sentinel"""
    rng = random.Random(SEED + 97 + F.deg)
    cases = [(F.zero, F.zero, INF, "sentinel")]
    for A in base_points(F, rng, n_pts, edge_field32):
        cases.append(aff32(F, A) + (A, "generic"))
        # one zero coordinate is not the sentinel
        cases.append((F.zero, to_dev32(F, A[1]), (F.zero, A[1]), "x zero"))
        cases.append((to_dev32(F, A[0]), F.zero, (A[0], F.zero), "y zero"))
    if F.deg == 2:  # nor is a single nonzero coefficient anywhere
        for pos in range(4):
            v = [0, 0, 0, 0]
            v[pos] = to_dev32(FQ1, rng.randrange(1, P))
            x, y = (v[0], v[1]), (v[2], v[3])
            cases.append((x, y, (from_dev32(F, x), from_dev32(F, y)), "one coefficient"))
    return cases


def chk_zfrom_aff(F, c, o):
    n = 48 * F.deg
    flag = int(o[n])
    if flag != (1 if c[2] is INF else 0):
        return "xyzz_is_inf gave %d" % flag
    e = check_point32(F, o[:n], c[2])
    if e or c[2] is INF:
        return e
    vals, _ = fields32(F, o, 4)
    one = to_dev32(F, F.one)
    if (vals[0], vals[1]) != (c[0], c[1]) or vals[2] != one or vals[3] != one:
        return "not the affine point with ZZ = ZZZ = 1"


def chk_zdbl(F, c, o):
    n = 48 * F.deg
    e = check_point32(F, o[:n], c[1])
    if e:
        return "into another point: " + e
    e = check_point32(F, o[n:], c[1])
    if e:
        return "in place: " + e


def suitesz():
    out = []
    for name, F, base, form in (("Fq", FQ1, 110, "W12"), ("Fq2", FQ2, 120, "W24")):
        n = 12 if F.deg == 1 else 6
        pt = lambda p, F=F: canon32(F, *p)
        out.append(Suite("xyzz_madd<%s>" % name, base, form, zmadd_cases(F, n),
                         lambda c, F=F, pt=pt: (pt(c[0]) and canon32(F, c[1], c[2]) and c[3] in (0, 1) and
                                                (c[1], c[2]) != (F.zero, F.zero)),  # xyzz_madd takes no infinity
                         lambda c, o, F=F: check_point32(F, o, c[4]), operands=lambda c: [c[0], c[1], c[2], ("w", c[3])]))
        out.append(Suite("xyzz_add<%s>" % name, base + 1, form, zadd_cases(F, n), lambda c, pt=pt: pt(c[0]) and pt(c[1]),
                         lambda c, o, F=F: check_point32(F, o, c[2]), operands=lambda c: list(c[:2])))
        out.append(Suite("xyzz_dbl<%s>" % name, base + 2, form, zdbl_cases(F, n), lambda c, pt=pt: pt(c[0]),
                         lambda c, o, F=F: chk_zdbl(F, c, o), operands=lambda c: [c[0]]))
        out.append(Suite("xyzz_from_aff_dbl<%s>" % name, base + 3, form, zaff_dbl_cases(F, n),
                         lambda c, F=F: canon32(F, c[0], c[1]) and c[1] != F.zero,
                         lambda c, o, F=F: check_point32(F, o, c[2]), operands=lambda c: list(c[:2])))
        out.append(Suite("xyzz_mul_small<%s>" % name, base + 4, form, zmul_small_cases(F, n // 2),
                         lambda c, pt=pt: pt(c[0]) and 0 <= c[1] < 1 << 32,
                         lambda c, o, F=F: check_point32(F, o, c[2]), operands=lambda c: [c[0], ("w", c[1])]))
        out.append(Suite("xyzz_from_aff_is_inf<%s>" % name, base + 5, form, zfrom_aff_cases(F, n),
                         lambda c, F=F: canon32(F, c[0], c[1]),
                         lambda c, o, F=F: chk_zfrom_aff(F, c, o), operands=lambda c: list(c[:2])))
    return out


# ------------------------------------------------------------------ lane layout
def lanes_per_element(form):
    return 2 if form == "PAIR" else 1


def flatten(x, form, lane):
    """the words one lane reads for operand x. Forms: "W8" / "W12" / "W24" 32-bit words (Fq2: c0 then
    c1), "F29" limbs, "F2" an Fq2 value's c0 then c1 limbs, "PAIR" the lane's own coefficient (even
    lane c0, odd lane c1). ("w", v) is one plain word, a 14-tuple raw limbs."""
    if isinstance(x, int):
        return limbs29(x) if form[0] != "W" else words(x, 8 if form == "W8" else 12)
    if x and x[0] == "w":
        return (x[1],)
    if form[0] != "W" and len(x) == 14 and all(isinstance(v, int) for v in x):
        return tuple(x)
    if form == "PAIR" and len(x) == 2 and all(isinstance(v, int) for v in x):
        return limbs29(x[lane])
    out = ()
    for e in x:
        out += flatten(e, form, lane)
    return out


def encode(suite, case):
    """the rows (one per lane) of one lane group for a case"""
    ops = suite.operands(case)
    return [flatten(ops, suite.form, lane) for lane in range(lanes_per_element(suite.form))]


def decode(suite, rows):
    """one lane group's output rows in the shape suite.check takes"""
    pair = suite.form == "PAIR"
    r = rows[0]
    if suite.kind == "raw":
        return r
    if suite.kind == "q":
        return (rows[0][:14], rows[1][:14]) if pair else (r[:14], r[14:28])
    if suite.kind == "qpred":
        if pair:
            return ((rows[0][:14], rows[1][:14]), [rows[0][14:20], rows[1][14:20]])
        return ((r[:14], r[14:28]), [r[28:34]])
    assert suite.kind == "point"
    if pair:
        return [[rows[0][14 * k:14 * k + 14], rows[1][14 * k:14 * k + 14]] for k in range(4)]
    return [[r[14 * k:14 * k + 14]] for k in range(4)]


FAMILIES = {"limb32": suites32, "f29": suites29, "fq2": suitesq, "curve": suitesc, "xyzz": suitesz}
# the suites of each family by name (the GPU test is parametrised over these without generating the
# cases at collection time; tests/test_field_cases.py checks that the lists match)
NAMES = {
    "limb32": ["fr_mul_asm_cios", "fr_add_sub_neg_dbl", "fr_inv", "fq_mul_asm_cios", "fq_add_sub_neg_dbl", "fq_inv",
               "fr_mul_x2", "fr_mont", "fq_from_mont", "fr_is_canonical", "f2_mul_sqr", "f2_inv"],
    "f29": ["f29_mul", "f29_mul2", "f29_redc_sum4", "f29_add", "f29_sub<2>", "f29_sub<4>", "f29_sub<8>", "f29_sub<16>",
            "f29_csub<1>", "f29_csub<2>", "f29_csub<4>", "f29_csub<8>", "f29_canon", "f29_reduce<4>", "f29_reduce<8>",
            "f29_reduce<16>", "f29_predicates", "f29_pack_unpack", "f29_unpack"],
    "fq2": [f + s for f in ("F2_29", "FP29", "FP29A")
            for s in ("_mul", "_mul_sum", "_sqr_b<8>", "_sqr_b<16>", "_one_predicates")],
    "curve": ["x29_madd<F29>", "x29_from_aff_dbl<F29>", "x29_add<F29>", "x29_dbl<F29>", "x29_madd<FP29A>",
              "x29_from_aff_dbl<FP29A>", "x29_add<FP29A>", "x29_dbl<FP29A>", "x29_add_split<F29>",
              "x29_dbl_split<F29>", "x29_add_split<FP29>", "x29_dbl_split<FP29>"],
    "xyzz": [s + "<%s>" % f for f in ("Fq", "Fq2")
             for s in ("xyzz_madd", "xyzz_add", "xyzz_dbl", "xyzz_from_aff_dbl", "xyzz_mul_small", "xyzz_from_aff_is_inf")],
}
_cache = {}


def suites(family):
    if family not in _cache:
        _cache[family] = FAMILIES[family]()
    return _cache[family]


def suite(family, name):
    return next(s for s in suites(family) if s.name == name)
