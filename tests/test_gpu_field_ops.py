"""The device field and curve functions, one at a time, against big-integer references at the operands
where their bound arguments are tight (tests/field_cases.py). tests/native/field_ops.hip wraps each
inline function of ff_dev.hpp / ff_asm.hpp (32-bit limbs), ff29.hpp, fq2pair.hpp, curve29.hpp, curve_dev.hpp
(the 32-bit-limb XYZZ formulas) and the split additions of msm_impl.hpp in a kernel of its own; the
product library is not involved.

32-bit layer: exact word equality; its XYZZ points: canonical words, the reference point. Radix-2^29 layer: a rewrite may return another representative, so
the assertions are congruence mod p, the value bound the header documents for the op, and normalized
limbs; predicates and infinity (a literal ZZ == 0) are exact. The bound comments of ff29.hpp,
fq2pair.hpp and curve29.hpp are what the case tables encode: change a bound there and the table
changes with it.

Lane layout: whole 64-lane waves, padded with the first case. A lane-pair (Fq2) case also runs a
second time one pair further, so it meets both pair positions of a quad (lanes 0-1 and 2-3); a split
op holds its operands on both lane groups and both must return bit-identical words."""
import copy
import ctypes
import os
import subprocess

import numpy as np
import pytest

import field_cases as fc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SO = os.path.join(ROOT, "tests", "native", "libfield_ops.so")


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(SO):  # a failing build fails the test; it never skips
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "r1cs-spartan_amd", "csrc"), "testlib"])
    L = ctypes.CDLL(SO)
    L.spx_field_op.restype = ctypes.c_int
    L.spx_field_op.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64,
                               ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int)]
    return L


def run_op(L, op, rows):
    ni, no = ctypes.c_int(0), ctypes.c_int(0)
    assert L.spx_field_op(op, None, None, 0, ctypes.byref(ni), ctypes.byref(no)) == 0, "unknown op %d" % op
    inp = np.ascontiguousarray(np.array(rows, dtype=np.uint32))
    assert inp.ndim == 2 and inp.shape[1] == ni.value, (inp.shape, ni.value)
    assert inp.shape[0] % 64 == 0
    out = np.zeros((inp.shape[0], no.value), dtype=np.uint32)
    err = L.spx_field_op(op, inp.ctypes.data, out.ctypes.data, inp.shape[0], ctypes.byref(ni), ctypes.byref(no))
    if err != 0:  # nothing more is launched on a device that reported an error
        pytest.exit("HIP error %d in field op %d" % (err, op), returncode=3)
    return out


def layout(s):
    """(rows, rows per case, start row of the second pass or None)"""
    per_case = []
    for c in s.cases:
        per_case.append(fc.encode(s, c) * s.group)
    rpc = len(per_case[0])
    rows = [r for g in per_case for r in g]
    second = None
    if rpc == 2:  # lane pairs: run again an odd number of pairs further
        if len(per_case) % 2 == 0:
            rows += per_case[0]
        second = len(rows)
        rows += [r for g in per_case for r in g]
    while len(rows) % 64:
        rows += per_case[0]
    return rows, rpc, second


def run_suite(L, s):
    rows, rpc, second = layout(s)
    out = run_op(L, s.op, rows)
    n = len(s.cases)
    if second is not None:
        assert second // 2 % 2 == 1
        assert np.array_equal(out[:n * rpc], out[second:second + n * rpc]), \
            "%s: a case gives different words in the two pair positions of a quad" % s.name
    lst = out[:n * rpc].tolist()
    bad = []
    half = rpc // s.group
    for i, c in enumerate(s.cases):
        g = lst[i * rpc:(i + 1) * rpc]
        if s.group == 2 and g[:half] != g[half:]:
            msg = "the two lane groups of a split op differ"
        else:
            msg = s.check(c, fc.decode(s, g[:half]))
        if msg:
            bad.append("case %d: %s; operands %r" % (i, msg, s.operands(c)))
    assert not bad, "%s: %d of %d cases wrong; first: %s" % (s.name, len(bad), n, " | ".join(bad[:3]))


@pytest.mark.parametrize("name", fc.NAMES["limb32"])
def test_limb32_ops(lib, name):
    """fr_mul_asm / fq_mul_asm / fe_mul_cios / fr_mul_x2_asm, fe_add / sub / neg / dbl, Montgomery
    conversions, fr_is_canonical, fe_inv, f2_mul / f2_sqr / f2_inv: exact words"""
    run_suite(lib, fc.suite("limb32", name))


@pytest.mark.parametrize("name", fc.NAMES["f29"])
def test_f29_ops(lib, name):
    """ff29.hpp: products (< 2p), f29_redc_sum4 on its per-chain limb precondition, add / sub<K> /
    csub<K> / reduce<K> / canon, the zero predicates (exact), pack / unpack"""
    run_suite(lib, fc.suite("f29", name))


@pytest.mark.parametrize("name", fc.NAMES["fq2"])
def test_fq2_forms(lib, name):
    """F2_29, PairOps<FP29, false>, PairOps<FP29A, true>: mul, mul_sum, sqr_b<8 / 16>, one, and the
    pair-combined predicates, against Python Fq2"""
    run_suite(lib, fc.suite("fq2", name))


@pytest.mark.parametrize("name", fc.NAMES["curve"])
def test_curve_formulas(lib, name):
    """x29_madd / x29_from_aff_dbl / x29_add / x29_dbl and the split forms against textbook affine
    arithmetic: generic, P + P through every representative, P + (-P), infinity on either side"""
    run_suite(lib, fc.suite("curve", name))


@pytest.mark.parametrize("name", fc.NAMES["xyzz"])
def test_xyzz32_layer(lib, name):
    """curve_dev.hpp over Fq and Fq2 (32-bit limbs): xyzz_madd (neg false / true), xyzz_add, xyzz_dbl (into
    another point and in place), xyzz_from_aff_dbl, xyzz_mul_small (k = 0, 1, 2, 3, 2^31, 2^32 - 1),
    xyzz_from_aff with xyzz_is_inf, against textbook affine arithmetic: generic, P + P and P + (-P) through
    several ZZ-scaled representatives, infinity on either side, the (0, 0) sentinel. Exact: infinity is
    a literal ZZ == 0, otherwise (X / ZZ, Y / ZZZ) is the reference point, ZZ^3 == ZZZ^2, canonical words"""
    run_suite(lib, fc.suite("xyzz", name))


def test_regression_fr_inv_exponent_borrow(lib):
    """fe_inv<FrCfg> once dropped the borrow of r - 2 (r's low limb is 1): the named cases"""
    s = copy.copy(fc.suite("limb32", "fr_inv"))
    s.cases = list(fc.FR_INV_REGRESSION)
    run_suite(lib, s)
