"""One MSM of 2^10 points per curve under the wide window plan (SPX_MSM_WIDE_MIN_LOG=8: c = 17, 2^16
buckets, nearly all of them empty: the bucket weighting's full-depth tree) against the oracle. Run as a
child process by tests/test_gpu_weighting.py, so that the setting is in place before the library is
loaded. Exit status 0 = all equal."""
import os
import sys


def main():
    here = os.path.dirname(os.path.abspath(__file__))
    sys.path.insert(0, here)
    from conftest import ensure_oracle_lib, load_product

    ensure_oracle_lib()
    import oracle_c as oc
    from msm_wide_check import edge_and_random
    from test_gpu_parity import _pp_bases

    spx = load_product()
    n = 1 << 10
    assert spx.msm_window_plan(n) == (17, 15), spx.msm_window_plan(n)
    ctx = spx.Context(0)
    g1, g2 = _pp_bases(oc, 10, 0x3E1)
    sc = edge_and_random(n, 23)
    ok = spx.msm_g1(ctx, g1, sc) == oc.msm_g1(g1, sc, n) and spx.msm_g2(ctx, g2, sc) == oc.msm_g2(g2, sc, n)
    print("all equal" if ok else "FAILED", flush=True)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
