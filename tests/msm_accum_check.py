"""MSM inputs aimed at the exits of the bucket accumulation's mixed addition (x29_madd in k_accum_aff),
shared by tests/test_gpu_msm_accum.py in-process (n = 2^8, 2^10) and, run as a child process so that
SPX_MSM_WIDE_MIN_LOG is in place before the library is loaded, at n = 2^12 under the wide window plan:

  msm_accum_check.py LOG_N      every case below for msm_g1 and msm_g2 against the oracle; exit 0 = all equal

Cases (name, bases, scalars):
  mixed            the scalars 0, 1, r - 1, (r - 1) / 2, (r + 1) / 2 and random ones; every third base at
                   infinity; a base repeated next to itself with the same scalar; a base next to its
                   negation with the same scalar
  one base         the same base n times, scalars cycling through four values: the first two references
                   of every bucket are the same point, so the addition leaves through the doubling exit
  base, negation   pairs (B, -B) with one scalar per pair: a bucket's references cancel pair by pair
                   through the infinity exit; the result is infinity
"""
import os
import random
import sys

from msm_wide_check import FIXED, HALF, R, fr, pp_bases

Q = 0x1A0111EA397FE69A4B1BA7B6434BACD764774B84F38512BF6730D2A0F6B0F6241EABFFFEB153FFFFB9FEFFFFFFFFAAAB
EDGE = [0, 1, R - 1, HALF, HALF + 1]
SIZE = {"g1": 96, "g2": 192}
PP_SEED = 0xACC


def negate(curve, b):
    from bls12_381 import g1_from_uncompressed, g1_uncompressed, g2_from_uncompressed, g2_uncompressed

    if curve == "g1":
        x, y = g1_from_uncompressed(b)
        return g1_uncompressed((x, -y % Q))
    x, y = g2_from_uncompressed(b)
    return g2_uncompressed((x, (-y[0] % Q, -y[1] % Q)))


def infinity(curve):
    from bls12_381 import g1_uncompressed, g2_uncompressed

    return g1_uncompressed(None) if curve == "g1" else g2_uncompressed(None)


def cases(curve, fin, n):
    """fin: at least n finite uncompressed bases"""
    rs = random.Random(0xACC0 + n + len(curve))
    inf = infinity(curve)
    pts = [inf if i % 3 == 0 else fin[i] for i in range(n)]
    sc = [rs.randrange(1, R) for _ in range(n)]
    for i, e in zip((1, 2, 4, 5, 13), EDGE):  # on finite bases
        sc[i] = e
    pts[7], sc[7] = pts[8], sc[8]                  # repeated base, same scalar
    pts[11], sc[11] = negate(curve, pts[10]), sc[10]  # base and negation, same scalar
    assert all(pts[i] != inf for i in (1, 2, 4, 5, 13, 7, 8, 10, 11)) and set(EDGE) <= set(sc)
    out = [("mixed", pts, sc)]
    four = [1, FIXED, R - 1, rs.randrange(R)]
    out.append(("one base", [fin[1]] * n, [four[i % 4] for i in range(n)]))
    pairs = [fin[i // 2] if i % 2 == 0 else negate(curve, fin[i // 2]) for i in range(n)]
    ps = [rs.randrange(1, R) for _ in range(n // 2)]
    out.append(("base, negation", pairs, [ps[i // 2] for i in range(n)]))
    return out


def run(spx, oc, ctx, curve, fin, n):
    """[(case name, equal?, oracle's result is infinity?)]"""
    res = []
    for name, pts, sc in cases(curve, fin, n):
        b, s = b"".join(pts), fr(sc)
        assert len(b) == SIZE[curve] * n and len(sc) == n
        if curve == "g1":
            got, want = spx.msm_g1(ctx, b, s), oc.msm_g1(b, s, n)
        else:
            got, want = spx.msm_g2(ctx, b, s), oc.msm_g2(b, s, n)
        res.append((name, got == want, want == infinity(curve)))
    return res


def finite_bases(spx, ctx, nv):
    g1, g2 = pp_bases(spx.MLProofForR1CS.setup(ctx, nv, PP_SEED).serialize_uncompressed(), nv)
    return {"g1": [g1[96 * i:96 * (i + 1)] for i in range(1 << nv)], "g2": [g2[192 * i:192 * (i + 1)] for i in range(1 << nv)]}


def main():
    here = os.path.dirname(os.path.abspath(__file__))
    sys.path.insert(0, here)
    from conftest import ensure_oracle_lib, load_product

    ensure_oracle_lib()
    import oracle_c as oc

    spx = load_product()
    lg = int(sys.argv[1])
    ctx = spx.Context(0)
    if os.environ.get("SPX_MSM_WIDE_MIN_LOG"):
        assert spx.msm_window_plan(1 << lg) == (17, 15), spx.msm_window_plan(1 << lg)
    fin = finite_bases(spx, ctx, lg)
    fails = []
    for curve in ("g1", "g2"):
        for name, ok, is_inf in run(spx, oc, ctx, curve, fin[curve], 1 << lg):
            print("%-16s 2^%d %s %s" % (name, lg, curve, "ok" if ok else "DIFFERS"), flush=True)
            if not ok or is_inf != (name == "base, negation"):
                fails.append((name, curve, ok, is_inf))
    print("FAILED: %s" % fails if fails else "all equal", flush=True)
    return 1 if fails else 0


if __name__ == "__main__":
    sys.exit(main())
