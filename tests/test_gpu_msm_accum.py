"""spx_msm_g1 / spx_msm_g2 through the bucket accumulation's rewritten field code, byte-equal to the
oracle: n = 2^8 and 2^10 in-process, n = 2^12 under the wide window plan (SPX_MSM_WIDE_MIN_LOG=8, c = 17
with folded signs) in a child process, with the inputs of tests/msm_accum_check.py: the scalars 0, 1,
r - 1, (r - 1) / 2, (r + 1) / 2 and random ones, every third base at infinity, a base repeated with the
same scalar and a whole input of one base (the doubling exit of the mixed addition), a base with its
negation and a whole input of such pairs (the infinity exit). And one proof at log_n = 8, byte-equal to
the oracle's."""
import os
import subprocess
import sys

import pytest

import msm_accum_check as mc

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def bases(spx, ctx):
    return mc.finite_bases(spx, ctx, 10)


@pytest.mark.parametrize("lg", [8, 10])
@pytest.mark.parametrize("curve", ["g1", "g2"])
def test_msm_exits_and_edge_scalars(spx, ctx, oc, bases, curve, lg):
    res = mc.run(spx, oc, ctx, curve, bases[curve], 1 << lg)
    assert [name for name, _, _ in res] == ["mixed", "one base", "base, negation"]
    for name, ok, is_inf in res:
        assert ok, "%s 2^%d %s differs from the oracle" % (name, lg, curve)
        assert is_inf == (name == "base, negation"), name


def test_msm_exits_wide_plan():
    """n = 2^12 with c = 17 and 15 windows"""
    e = dict(os.environ)
    for k in ("SPX_SORT_FORM", "SPX_MSM_CAP_SCALE"):
        e.pop(k, None)
    e["SPX_MSM_WIDE_MIN_LOG"] = "8"
    r = subprocess.run([sys.executable, "-u", os.path.join(HERE, "msm_accum_check.py"), "12"], env=e, timeout=120,
                       capture_output=True, text=True)
    print(r.stdout)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "all equal" in r.stdout


def test_proof_log_n_8(spx, ctx, oc):
    log_n, log_v = 8, 3
    inst = oc.Instance(0, log_n, log_v, 0xACC8)
    ppc = oc.PP.keygen(log_n, 77)
    pp = spx.PublicParameter.load(ctx, ppc.serialize())
    pk = spx.MLArgumentForR1CS.index(ctx, *[spx.Csr(M.n, M.row_ptr, M.col, M.val) for M in inst.mats])
    got = spx.MLArgumentForR1CS.prove(pk, inst.v_bytes, inst.w_bytes, pp)
    assert got == oc.prove(inst.mats, inst.v_bytes, inst.w_bytes, ppc, 0, 0)
