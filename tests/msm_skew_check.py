"""Skewed-scalar MSM inputs (0 / 1 witnesses and their kin) at n = 2^14, the smallest size that takes
the c = 16 / 16-window key path, shared by tests/test_gpu_msm_skew.py, which also runs this file as a
child process whose SPX_SORT_FORM (staged | direct) forces one form of the bucket sort: the all-ones,
random-bits, {0, 1, r - 1} and half-repeated inputs on G1 and G2, each byte-equal to the oracle and
with at most kSeg = 4 partials left to the weighting leaf for any bucket. Exit status 0 = all equal."""
import os
import random
import sys

R = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001
LOG_N = 14
N = 1 << LOG_N
K_SEG = 4  # msm_common.hpp
PP_SEED = 0x5CE3


def fr(values):
    return b"".join(int(x).to_bytes(32, "little") for x in values)


def pp_bases(b, nv):
    """uncompressed G1 / G2 bases of level 0 (2^nv points each) from a serialised public parameter
    (the offsets of tests/test_gpu_parity.py::_pp_bases)."""
    n = 1 << nv
    g1 = b[24 : 24 + 96 * n]
    pos = 16
    for i in range(nv):
        pos += 8 + 96 * (n >> i)
    pos += 8 + 8
    g2 = b[pos : pos + 192 * n]
    return g1, g2


def all_ones():
    return fr([1]) * N


def random_bits(seed=11):
    rs = random.Random(seed)
    return fr(rs.getrandbits(1) for _ in range(N))


def level0_shape(seed=12):
    """q_L[b] = z[2b+1] - z[2b] of a 0 / 1 witness: 0, 1 and r - 1"""
    rs = random.Random(seed)
    return fr((0, 1, 0, R - 1)[rs.getrandbits(2)] for _ in range(N))


FIXED = 0x5A17C0DE9B3F4E21D7A6C5B4F3E2D1C0B9A8978685746352413F2E1D0C0BFAE9 % R  # full width: 16 non-zero digits


def half_repeated(seed=13):
    """uniform random and one fixed full-width scalar interleaved: 16 hot buckets inside ordinary bins"""
    rs = random.Random(seed)
    return fr(FIXED if i & 1 else rs.randrange(R) for i in range(N))


def cycle_1234():
    """buckets 0..3 hot: four hot buckets in one chunk of the weighting leaf (kTreeChunkLog = 2)"""
    return fr(1 + (i & 3) for i in range(N))


def uniform(seed=14):
    rs = random.Random(seed)
    return fr(rs.randrange(R) for _ in range(N))


def bucket_counts(scalars, c=16, windows=16):
    """references per bucket (|signed digit| - 1) of the c-bit signed-digit windows, as the library cuts them"""
    cnt = {}
    for i in range(len(scalars) // 32):
        s = int.from_bytes(scalars[32 * i : 32 * i + 32], "little")
        carry = 0
        for _ in range(windows):
            v = (s & ((1 << c) - 1)) + carry
            s >>= c
            carry = 1 if v > (1 << (c - 1)) else 0
            d = v - (1 << c) if carry else v
            if d:
                cnt[abs(d) - 1] = cnt.get(abs(d) - 1, 0) + 1
    return cnt


FORCED_FORM_CASES = [("all ones", all_ones), ("random bits", random_bits), ("{0,1,r-1}", level0_shape),
                     ("half repeated", half_repeated)]


def main():
    here = os.path.dirname(os.path.abspath(__file__))
    sys.path.insert(0, here)
    from conftest import ensure_oracle_lib, load_product

    ensure_oracle_lib()
    import oracle_c as oc

    spx = load_product()
    ctx = spx.Context(0)
    g1, g2 = pp_bases(spx.MLProofForR1CS.setup(ctx, LOG_N, PP_SEED).serialize_uncompressed(), LOG_N)
    fails = []
    for name, make in FORCED_FORM_CASES:
        sc = make()
        for grp, got, want in (("g1", spx.msm_g1(ctx, g1, sc), oc.msm_g1(g1, sc, N)),
                               ("g2", spx.msm_g2(ctx, g2, sc), oc.msm_g2(g2, sc, N))):
            ok = got == want
            print("%-16s %s %s" % (name, grp, "ok" if ok else "DIFFERS"), flush=True)
            if not ok:
                fails.append((name, grp))
    st = ctx.msm_skew_stats()
    print("skew stats", st, flush=True)
    if st[2] < 1 or st[3] > K_SEG:
        fails.append(("skew stats", st))
    print("FAILED: %s" % fails if fails else "all equal", flush=True)
    return 1 if fails else 0


if __name__ == "__main__":
    sys.exit(main())
