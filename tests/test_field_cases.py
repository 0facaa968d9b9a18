"""CPU checks of tests/field_cases.py, the operands and references of tests/test_gpu_field_ops.py:
every generated operand meets the documented precondition of the op it is fed to (so a GPU failure is
the kernel's and not the input's), the curve reference agrees with the oracle on real G1 / G2 points,
the Montgomery constants in the headers equal values recomputed from p and r, and the test-only
device library compiles for gfx950."""
import os
import random
import re
import shutil
import subprocess

import pytest

import bls12_381 as bls
import field_cases as fc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "r1cs-spartan_amd", "csrc")
P, R = fc.P, fc.R


def test_moduli_match_oracle():
    assert fc.P == bls.Q and fc.R == bls.R


@pytest.mark.parametrize("family", sorted(fc.FAMILIES))
def test_names_and_preconditions(family):
    """value bounds, limb bounds and (f29_redc_sum4) the per-chain limb condition, for every case"""
    ss = fc.suites(family)
    assert [s.name for s in ss] == fc.NAMES[family]
    for s in ss:
        bad = [i for i, c in enumerate(s.cases) if not s.pre(c)]
        assert not bad, "%s: %d cases violate the op's precondition, first %d" % (s.name, len(bad), bad[0])
        # what reaches the device is what the precondition spoke of: normalized limbs unless the op
        # admits 2^30 limbs (f29_redc_sum4), and one row per lane of equal length
        rows = [fc.encode(s, c) for c in s.cases[:200]]
        assert len({len(r) for g in rows for r in g}) == 1
        assert all(0 <= w < 1 << 32 for g in rows for r in g for w in r)


def test_directed_operands_present():
    """the edge values the bound arguments speak of are in the tables"""
    for k in (1, 2, 4, 8, 16, 10, 6):
        E = fc.edges29(k)
        assert max(E) == k * P - 1 and all(0 <= x < k * P for x in E)
        for j in range(k):
            assert j * P in E and (j * P + 1) in E
        ones = fc.all_ones29(k * P)
        assert ones in E and fc.limbs29(ones)[:13] == (fc.M29,) * 13
        assert ones + (1 << 377) >= k * P  # the largest admissible top limb
    for p, n in ((R, 8), (P, 12)):
        E = fc.canon_edges(p, n)
        mont = 1 << (32 * n)
        for x in (0, 1, 2, p - 1, p - 2, (p + 1) // 2, (p - 1) // 2, mont % p, mont * mont % p):
            assert x in E
        assert all(0 <= x < p for x in E)
    # f29_redc_sum4: the borrow-free operand of 8p - 1 and the all-ones wide operand reach the kernel
    s = fc.suite("f29", "f29_redc_sum4")
    wide = {tuple(x) for c in s.cases for x in c if not isinstance(x, int)}
    assert any(max(w[:13]) == (1 << 30) - 1 for w in wide)
    z = fc.limbs29(8 * P - 1)
    p16 = fc.limbs29(16 * P)
    k16 = (p16[0] + (1 << 29),) + tuple(p16[i] + (1 << 29) - 1 for i in range(1, 13)) + (p16[13] - 1,)
    assert fc.val29(k16) == 16 * P
    assert tuple(k16[i] - z[i] for i in range(14)) in wide
    # the madd P + P cases cover every representative pair of X (8) and Y (4)
    m = fc.suite("curve", "x29_madd<F29>")
    seen = {(c[0][0] // P, c[0][1] // P) for c in m.cases if c[4] is not fc.INF}
    assert seen == {(a, b) for a in range(8) for b in range(4)}
    # and the Fq2 additions reach P.c1 - P.c0 > 8p, where sqr_b<16>'s 16p is needed
    m2 = fc.suite("curve", "x29_madd<FP29A>")
    assert sum(fc.wide_p_gap(fc.FQ2, c) > 8 * P for c in m2.cases if c[4] is not fc.INF and c[0][2] != (0, 0)) >= 16


def test_lane_layout_roundtrip():
    s = fc.suite("fq2", "FP29A_mul")
    c = s.cases[7]
    rows = fc.encode(s, c)
    assert len(rows) == 2 and len(rows[0]) == 28
    assert rows[0][:14] == fc.limbs29(c[0][0]) and rows[1][:14] == fc.limbs29(c[0][1])
    assert rows[0][14:] == fc.limbs29(c[1][0]) and rows[1][14:] == fc.limbs29(c[1][1])
    m = fc.suite("curve", "x29_madd<FP29A>")
    rows = fc.encode(m, m.cases[0])
    assert len(rows[0]) == 6 * 14 + 1 and rows[0][-1] == rows[1][-1] == m.cases[0][3]
    x = 8 * P - 1
    assert fc.val29(fc.limbs29(x)) == x and fc.val32(fc.words(x, 12)) == x


@pytest.mark.parametrize("curve,F", [(bls.G1, fc.FQ1), (bls.G2, fc.FQ2)], ids=["G1", "G2"])
def test_curve_reference_matches_oracle(curve, F):
    A = curve.gen
    assert fc.aff_dbl(F, A) == curve.mul_affine(A, 2)
    acc = fc.INF
    for k in range(1, 12):
        acc = fc.aff_add(F, acc, A)  # k = 2 takes the doubling branch
        assert acc == curve.mul_affine(A, k)
        assert fc.aff_mul(F, k, A) == acc
    k1, k2 = 0x1234567, 0xFEDCBA987
    B, C = curve.mul_affine(A, k1), curve.mul_affine(A, k2)
    assert fc.aff_add(F, B, C) == curve.mul_affine(A, k1 + k2)
    assert fc.aff_add(F, B, fc.aff_neg(F, B)) is fc.INF
    assert fc.aff_add(F, B, fc.INF) == B and fc.aff_add(F, fc.INF, C) == C
    assert fc.aff_neg(F, B) == curve.neg_affine(B)


def test_checkers_reject_wrong_results():
    """the assertions of the GPU test bite: a wrong representative bound, a non-normalized limb, a
    value off by one and a wrong point are all reported"""
    s = fc.suite("f29", "f29_mul")
    c = s.cases[100]
    good = c[0] * c[1] * fc.R29I % P
    assert s.check(c, list(fc.limbs29(good))) is None
    assert s.check(c, list(fc.limbs29(good + P))) is None  # another representative below 2p
    assert s.check(c, list(fc.limbs29(good + 2 * P)))
    assert s.check(c, list(fc.limbs29((good + 1) % P)))
    l = list(fc.limbs29(good + P))
    if l[1]:
        l[0] += 1 << 29
        l[1] -= 1
        assert s.check(c, l)
    m = fc.suite("curve", "x29_madd<F29>")
    c = next(c for c in m.cases if c[4] is not fc.INF)
    want = c[4]
    o = [[list(fc.limbs29(fc.to_dev(fc.FQ1, v)))] for v in (want[0], want[1], 1, 1)]
    assert m.check(c, o) is None
    o[0] = [list(fc.limbs29(fc.to_dev(fc.FQ1, (want[0] + 1) % P)))]
    assert m.check(c, o)
    inf = next(c for c in m.cases if c[4] is fc.INF)
    assert m.check(inf, o)


XYZZ_TAGS = {
    "xyzz_madd": {"generic", "P + P", "P - P", "infinite accumulator"},
    "xyzz_add": {"generic", "P + P", "P - P", "infinite left", "infinite right", "both infinite"},
    "xyzz_dbl": {"generic", "infinity"},
    "xyzz_from_aff_dbl": {"generic"},
    "xyzz_mul_small": {"generic", "k = 0", "infinite point"},
    "xyzz_from_aff_is_inf": {"generic", "sentinel", "x zero", "y zero"},
}


@pytest.mark.parametrize("field", ["Fq", "Fq2"])
def test_xyzz_case_tables_reach_every_branch(field):
    """the 32-bit XYZZ family: every branch of curve_dev.hpp's formulas has cases aimed at it, with the
    reference result that branch must give; xyzz_madd runs with neg false and true in each of them; the
    equal / opposite points come in several ZZ-scaled representatives; xyzz_mul_small gets every
    directed k with a finite and with an infinite point"""
    F = fc.FQ1 if field == "Fq" else fc.FQ2
    for op, tags in XYZZ_TAGS.items():
        s = fc.suite("xyzz", "%s<%s>" % (op, field))
        assert {c[-1] for c in s.cases} == tags | ({"one coefficient"} if (op, field) == ("xyzz_from_aff_is_inf", "Fq2") else set())
        for c in s.cases:
            want, tag = c[-2], c[-1]
            if tag in ("P - P", "both infinite", "infinity", "k = 0", "infinite point", "sentinel"):
                assert want is fc.INF, (op, tag)
            else:
                assert want is not fc.INF, (op, tag)
    m = fc.suite("xyzz", "xyzz_madd<%s>" % field)
    assert {(c[5], c[3]) for c in m.cases} == {(t, n) for t in XYZZ_TAGS["xyzz_madd"] for n in (0, 1)}
    for s, tag in ((m, "P + P"), (m, "P - P"), (fc.suite("xyzz", "xyzz_add<%s>" % field), "P + P")):
        assert len({c[0][2] for c in s.cases if c[-1] == tag}) >= 5  # distinct ZZ of the first operand
    for c in m.cases:  # the accumulator really is a representative of the point the tag speaks of
        if c[5] in ("P + P", "P - P"):
            X, Y, ZZ, ZZZ = (fc.from_dev32(F, v) for v in c[0])
            a = (fc.from_dev32(F, c[1]), fc.from_dev32(F, c[2]))
            if c[3]:
                a = fc.aff_neg(F, a)
            assert F.mul(a[0], ZZ) == X
            assert F.mul(a[1], ZZZ) == (Y if c[5] == "P + P" else F.neg(Y))
    ms = fc.suite("xyzz", "xyzz_mul_small<%s>" % field)
    for inf in (False, True):
        assert {c[1] for c in ms.cases if (c[0][2] == F.zero) == inf} >= set(fc.MUL_SMALL_K)
    for c in fc.suite("xyzz", "xyzz_add<%s>" % field).cases:
        assert (c[0][2] == F.zero) == (c[3] in ("infinite left", "both infinite"))
        assert (c[1][2] == F.zero) == (c[3] in ("infinite right", "both infinite"))


@pytest.mark.parametrize("field", ["Fq", "Fq2"])
def test_xyzz_checker_accepts_the_reference_and_rejects_wrong_points(field):
    F = fc.FQ1 if field == "Fq" else fc.FQ2
    m = fc.suite("xyzz", "xyzz_madd<%s>" % field)
    flat = lambda pt: [w for e in pt for cf in F.coeffs(e) for w in fc.words(cf, 12)]
    c = next(c for c in m.cases if c[5] == "generic")
    s = fc.scalars32(F, random.Random(1))[2]
    assert m.check(c, flat(fc.xyzz32(F, c[4], F.one))) is None
    assert m.check(c, flat(fc.xyzz32(F, c[4], s))) is None  # any representative of the right point
    good = fc.xyzz32(F, c[4], s)
    assert m.check(c, flat(fc.xyzz32(F, fc.aff_neg(F, c[4]), s)))  # the wrong point
    assert m.check(c, flat(good[:2] + (F.zero, good[3])))  # infinity where a point is due
    assert m.check(c, flat(good[:3] + (fc.to_dev32(F, F.one),)))  # ZZ^3 != ZZZ^2
    noncanon = flat(good)
    noncanon[:12] = fc.words(F.coeffs(good[0])[0] + P, 12)  # the same value, one p higher
    assert m.check(c, noncanon) == "X not canonical"
    inf = next(c for c in m.cases if c[5] == "P - P")
    assert m.check(inf, flat(good))  # a point where infinity is due
    assert m.check(inf, flat(good[:2] + (F.zero, F.zero))) is None
    f = fc.suite("xyzz", "xyzz_from_aff_is_inf<%s>" % field)
    sen = next(c for c in f.cases if c[3] == "sentinel")
    one = fc.to_dev32(F, F.one)
    assert f.check(sen, flat((one, one, F.zero, F.zero)) + [1]) is None
    assert f.check(sen, flat((one, one, F.zero, F.zero)) + [0])
    g = next(c for c in f.cases if c[3] == "x zero")
    assert f.check(g, flat((g[0], g[1], one, one)) + [0]) is None
    assert f.check(g, flat((one, one, F.zero, F.zero)) + [1])  # taken for the sentinel
    d = fc.suite("xyzz", "xyzz_dbl<%s>" % field)
    c = next(c for c in d.cases if c[2] == "generic")
    ok, bad = flat(fc.xyzz32(F, c[1], s)), flat(fc.xyzz32(F, fc.aff_neg(F, c[1]), s))
    assert d.check(c, ok + ok) is None and d.check(c, ok + bad) and d.check(c, bad + ok)


# ------------------------------------------------------------------ header constants
def _read(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def _array(text, name):
    m = re.search(r"\b%s\[\d+\]\s*=\s*\{([^}]*)\}" % re.escape(name), text)
    assert m, name
    return [int(x.rstrip("uU"), 16) for x in re.findall(r"0x[0-9a-fA-F]+[uU]?", m.group(1))]


def _scalar(text, pattern):
    m = re.search(pattern, text)
    assert m, pattern
    return int(m.group(1), 16)


def test_q29_constants():
    t = _read("ff29.hpp")
    q = t[t.index("struct Q29"):]
    assert fc.val29(_array(q, "P")) == P
    for k in (2, 4, 8, 16):
        l = _array(q, "P%d" % k)
        assert len(l) == 14 and fc.normalized(l) and fc.val29(l) == k * P
    assert tuple(_array(q, "ONE")) == fc.limbs29((1 << 406) % P)
    assert tuple(_array(q, "TO_R1")) == fc.limbs29((1 << 384) % P)
    # REDC by FROM_R1 maps x R1 to x R2: FROM_R1 = R2^2 / R1 mod p
    assert tuple(_array(q, "FROM_R1")) == fc.limbs29((1 << 406) ** 2 * pow(1 << 384, -1, P) % P)
    assert _scalar(q, r"uint32_t PINV\s*=\s*0x([0-9a-fA-F]+)") == -pow(P, -1, 1 << 29) % (1 << 29)
    assert _scalar(q, r"uint32_t INV5555\s*=\s*0x([0-9a-fA-F]+)") == pow(0x5555, -1, 1 << 32)
    assert (1 << 29) - (P & fc.M29) == 0x5555


def test_ff_dev_constants():
    t = _read("ff_dev.hpp")
    assert fc.val32(_array(t, "kFrP")) == R and fc.val32(_array(t, "kFqP")) == P
    assert fc.val32(_array(t, "kFrOne")) == (1 << 256) % R
    assert fc.val32(_array(t, "kFrR2")) == (1 << 512) % R
    assert fc.val32(_array(t, "kFqOne")) == (1 << 384) % P
    fr = t[t.index("struct FrCfg"):t.index("struct FqCfg")]
    fq = t[t.index("struct FqCfg"):t.index("kFrP")]
    assert _scalar(fr, r"INV\s*=\s*0x([0-9a-fA-F]+)") == -pow(R, -1, 1 << 32) % (1 << 32)
    assert _scalar(fq, r"INV\s*=\s*0x([0-9a-fA-F]+)") == -pow(P, -1, 1 << 32) % (1 << 32)


@pytest.mark.skipif(not (shutil.which("hipcc") or os.path.exists("/opt/rocm/bin/hipcc")), reason="no hipcc")
def test_field_ops_compiles_for_gfx950():
    """host and gfx950 device passes of the test-only library, front end only (a few seconds; the code
    generation is the `testlib` target of csrc/Makefile, part of `all`)"""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    src = os.path.join(ROOT, "tests", "native", "field_ops.hip")
    r = subprocess.run([hipcc, "-std=c++17", "--offload-arch=gfx950", "-fsyntax-only", "-Wall", "-Wno-unused-function",
                        "-Wno-unused-variable", "-I", CSRC, src], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    mk = _read("Makefile")
    assert re.search(r"^all:.*\$\(TESTLIB\)", mk, re.M) and "tests/native/field_ops.hip" in mk
