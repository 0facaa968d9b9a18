"""The field functions on the accumulation's mixed-addition path, on the device, word for word against
the integer models of tests/accum_cases.py: the Montgomery scan joined (f29_mul, f29_mul2,
f29_redc_sum4) and seeded in lockstep pairs (f29_mul_x2, f29_mul2_x2, the symmetric squares
f29_sqr_x2 next to f29_mul(a, a) of the same operands), and PairOps<FP29A>'s mul / mul_sum /
sqr_b<8 / 16> / mul_x2 / sqr_x2<16, 8> with the operands prepared from one exchange.
tests/native/accum_ops.hip wraps each in a kernel of its own over whole 64-lane waves; the product
library is not involved. tests/test_accum_refs.py ties the models to big-integer arithmetic and to the
documented bounds on the CPU.

A lane-pair case also runs a second time one pair further, so it meets both pair positions of a quad."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import accum_cases as ac

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SO = os.path.join(ROOT, "tests", "native", "libaccum_ops.so")
SUITES = ac.suites()


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(SO):  # a failing build fails the test; it never skips
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "r1cs-spartan_amd", "csrc"), "accumlib"])
    L = ctypes.CDLL(SO)
    L.spx_accum_op.restype = ctypes.c_int
    L.spx_accum_op.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64,
                               ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int)]
    return L


def run_op(L, op, rows):
    ni, no = ctypes.c_int(0), ctypes.c_int(0)
    assert L.spx_accum_op(op, None, None, 0, ctypes.byref(ni), ctypes.byref(no)) == 0, "unknown op %d" % op
    inp = np.ascontiguousarray(np.array(rows, dtype=np.uint32))
    assert inp.ndim == 2 and inp.shape[1] == ni.value, (inp.shape, ni.value)
    assert inp.shape[0] % 64 == 0
    out = np.zeros((inp.shape[0], no.value), dtype=np.uint32)
    err = L.spx_accum_op(op, inp.ctypes.data, out.ctypes.data, inp.shape[0], ctypes.byref(ni), ctypes.byref(no))
    if err != 0:  # nothing more is launched on a device that reported an error
        pytest.exit("HIP error %d in accumulation op %d" % (err, op), returncode=3)
    return out


@pytest.mark.parametrize("name", list(SUITES))
def test_words_equal_the_model(lib, name):
    cases, lanes, model = SUITES[name]
    per_case = [ac.rows(name, c) for c in cases]
    assert all(len(r) == lanes for r in per_case)
    rows = [r for g in per_case for r in g]
    second = None
    if lanes == 2:  # run again an odd number of pairs further
        if len(per_case) % 2 == 0:
            rows += per_case[0]
        second = len(rows)
        assert second // 2 % 2 == 1
        rows += [r for g in per_case for r in g]
    while len(rows) % 64:
        rows += per_case[0]
    out = run_op(lib, ac.OPS[name], rows)
    n = len(cases) * lanes
    if second is not None:
        assert np.array_equal(out[:n], out[second:second + n]), \
            "%s: a case gives different words in the two pair positions of a quad" % name
    got = out[:n].tolist()
    bad = []
    for i, c in enumerate(cases):
        want = [list(w) for w in model(c)]
        if got[i * lanes:(i + 1) * lanes] != want:
            bad.append("case %d: got %r, want %r; operands %r" % (i, got[i * lanes:(i + 1) * lanes], want, c))
    assert not bad, "%s: %d of %d cases differ; first: %s" % (name, len(bad), len(cases), bad[0])
