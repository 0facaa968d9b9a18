"""The wide MSM window plan: c = 17 with 15 signed windows (a scalar above (r - 1) / 2 is replaced by
its negative and the sign of its references flipped), which MSMs of >= 2^18 points take by default.
SPX_MSM_WIDE_MIN_LOG=10 brings it down to 2^10 .. 2^12 points, where the oracle is quick; every case
runs tests/msm_wide_check.py in a child process, so the setting is in place before a public parameter
is preprocessed, and compares with the oracle's MSM or proof byte for byte."""
import os
import subprocess
import sys

import pytest

import msm_wide_check as wc

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


def _child(args, **env):
    e = dict(os.environ)
    for k in ("SPX_MSM_WIDE_MIN_LOG", "SPX_SORT_FORM", "SPX_MSM_CAP_SCALE"):
        e.pop(k, None)
    e.update(env)
    r = subprocess.run([sys.executable, "-u", os.path.join(HERE, "msm_wide_check.py")] + [str(a) for a in args], env=e,
                       timeout=120, capture_output=True, text=True)
    print(r.stdout)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "all equal" in r.stdout


@pytest.fixture(scope="module")
def ref(spx, ctx, oc, tmp_path_factory):
    """the public parameter (GPU keygen) and the oracle's proof at log_n = 12, computed once and handed
    to the child processes as files"""
    d = tmp_path_factory.mktemp("msm_wide")
    pp = spx.MLProofForR1CS.setup(ctx, wc.LOG_N, wc.PP_SEED)
    ppb = pp.serialize_uncompressed()
    del pp
    inst = oc.Instance(0, wc.LOG_N, wc.LOG_V, wc.INST_SEED)
    want = oc.prove(inst.mats, inst.v_bytes, inst.w_bytes, oc.PP.load(ppb), 0, 0)
    (d / "pp").write_bytes(ppb)
    (d / "want").write_bytes(want)
    return str(d)


@pytest.mark.parametrize("form", ["auto", "staged", "direct"])
def test_msm_edge_scalars(form):
    """msm_g1 / msm_g2 at n = 2^10: random scalars with 0, 1, r - 1, (r - 1) / 2, (r + 1) / 2, the largest
    top digit, the carry through every window, the 2^16 tie and their negatives among them, with finite
    bases and with every third base at infinity; one scalar n times (hot buckets); every digit 1 at n = 2^12 (a bin above the sort's staging). By the sort's
    own choice of form, and under each forced form."""
    env = {} if form == "auto" else {"SPX_SORT_FORM": form}
    _child(["msm"], SPX_MSM_WIDE_MIN_LOG="10", **env)


@pytest.mark.parametrize("G", [1, 2, 4])
def test_proof_wide(ref, G):
    """a full proof at log_n = 12: the commitment and levels 0 and 1 wide, the other levels narrow;
    unsharded and over 2 and 4 virtual ranks (split instances of 2^16 buckets)"""
    _child(["proof", ref, G, "wide10"], SPX_MSM_WIDE_MIN_LOG="10")


def test_proof_wide_dense_rerun(ref):
    """halved compacted-key capacity on 4 ranks: the wide batches overflow and are rerun dense"""
    _child(["proof", ref, 4, "wide10", "reruns"], SPX_MSM_WIDE_MIN_LOG="10", SPX_MSM_CAP_SCALE="0.5")


def test_proof_wide_off(ref):
    """SPX_MSM_WIDE_MIN_LOG=0: no wide level, the same bytes"""
    _child(["proof", ref, 1, "off"], SPX_MSM_WIDE_MIN_LOG="0")


def test_proof_lowest_threshold_fits_the_bucket_limit(ref):
    """the setting is clamped to 8: levels 0 .. 3 (2^11 .. 2^8 points) and the commitment are wide, an
    opening batch of all levels stays within the sort's bucket limit, the same bytes"""
    _child(["proof", ref, 1, "wide8"], SPX_MSM_WIDE_MIN_LOG="3")
