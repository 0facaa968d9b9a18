"""The wide MSM window plan (c = 17, 15 signed windows; scalars above (r - 1) / 2 negated) at sizes a
test can afford, shared by tests/test_gpu_msm_wide.py, which runs this file as a child process so that
SPX_MSM_WIDE_MIN_LOG (and SPX_SORT_FORM, SPX_MSM_CAP_SCALE) are in place before the library is
loaded and a public parameter is preprocessed.

  msm_wide_check.py msm
      msm_g1 / msm_g2 at n = 2^10 against the oracle: random scalars with the edge scalars of the
      recoding among them (also with every third base at infinity), and one scalar n times (hot
      buckets). The same equal-scalar case at
      n = 2^12 with every digit 1: bucket 0 takes 15 x 2^12 references, more than the bin staging
      of the sort (kBinStage = 36864; 15 x 2^10 cannot reach it).
  msm_wide_check.py proof DIR G EXPECT [reruns]
      a full proof at log_n = 12 on G in-process ranks (1: unsharded), byte-equal to DIR/want (the
      oracle's proof, computed once by the test module; DIR/pp holds the public parameter). EXPECT
      names the window plan the public parameter must report: wide10, wide8 or off. `reruns`: the
      compacted keys must have overflowed and the batches rerun dense.
Exit status 0 = all equal."""
import os
import random
import sys
import threading

R = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001
HALF = (R - 1) // 2
C, W = 17, 15
LOG_N, LOG_V = 12, 3
INST_SEED, PP_SEED = 0x17A, 0x17B
MAX_BUCKETS = 1 << 19  # kMsmMaxBuckets (kernels.hpp)


def fr(values):
    return b"".join(int(x).to_bytes(32, "little") for x in values)


def recode(s):
    """(sign flip, the 15 signed 17-bit digits) as the library cuts a canonical scalar; asserts that no
    carry leaves window 14"""
    flip = s > HALF
    if flip:
        s = R - s
    carry, out = 0, []
    for _ in range(W):
        v = (s & ((1 << C) - 1)) + carry
        s >>= C
        carry = 1 if v > (1 << (C - 1)) else 0
        out.append(v - (1 << C) if carry else v)
    assert s == 0 and carry == 0, "carry out of window 14"
    return flip, out


def from_windows(ws):
    return sum(int(v) << (C * i) for i, v in enumerate(ws))


TOP = HALF >> (C * (W - 1))  # 0xE7DB: the largest top window of a folded scalar
# the folded values (<= (r - 1) / 2) the digit pass has to get right; each goes in with its negative
FOLDED = [
    1,
    HALF,                                      # the last scalar that is not negated
    ((TOP - 1) << (C * (W - 1))) | ((1 << (C * (W - 1))) - 1),  # windows 0..13 all 0x1FFFF under top - 1:
                                               # the carry runs through every window, top digit = TOP
    (1 << (C * (W - 1))) - 1,                  # windows 0..13 all 0x1FFFF, the carry ends as top digit 1
    from_windows([1 << (C - 1)] * (W - 1)),    # every window 2^16: the tie, each digit stays positive
    from_windows([(1 << (C - 1)) + 1] * (W - 1)),  # one past the tie: every digit negative, carry into the top
    from_windows([1] * W),
]
EDGE = [0] + FOLDED + [R - t for t in FOLDED]  # R - 1, (r + 1) / 2 among them


def edge_and_random(n, seed):
    rs = random.Random(seed)
    sc = EDGE + [rs.randrange(R) for _ in range(n - len(EDGE))]
    rs.shuffle(sc)
    assert max(recode(s)[1][W - 1] for s in sc) == max(TOP, recode(HALF)[1][W - 1])  # the largest top digit is in
    assert {0, 1, R - 1, HALF, HALF + 1} <= set(sc)
    return fr(sc)


FIXED = 0x5A17C0DE9B3F4E21D7A6C5B4F3E2D1C0B9A8978685746352413F2E1D0C0BFAE9 % R  # above (r - 1) / 2: negated


def pp_bases(b, nv):
    """uncompressed G1 / G2 bases of level 0 from a serialised public parameter (tests/msm_skew_check.py)"""
    n = 1 << nv
    g1 = b[24 : 24 + 96 * n]
    pos = 16
    for i in range(nv):
        pos += 8 + 96 * (n >> i)
    pos += 8 + 8
    g2 = b[pos : pos + 192 * n]
    return g1, g2


def expected_plan(expect, nv):
    """(c, windows) of the commitment MSM and of every opening level under the named setting"""
    wide_min = {"wide10": 10, "wide8": 8, "off": 0}[expect]

    def plan(size):
        k = size.bit_length() - 1
        if wide_min and k >= wide_min:
            return (17, 15)
        c = 16 if k >= 14 else max(3, k - 2)
        return (c, (256 + c - 1) // c)

    return plan(1 << nv), [plan(1 << (nv - i - 1)) for i in range(nv)]


def run_msm(spx, oc):
    ctx = spx.Context(0)
    g1, g2 = pp_bases(spx.MLProofForR1CS.setup(ctx, LOG_N, PP_SEED).serialize_uncompressed(), LOG_N)
    assert spx.msm_window_plan(1 << 10) == (17, 15) and spx.msm_window_plan(1 << 9)[0] < 16
    from bls12_381 import g1_uncompressed, g2_uncompressed

    fails = []
    cases = [("edge + random", 10, edge_and_random(1 << 10, 21), 0),
             ("one scalar n times", 10, fr([FIXED]) * (1 << 10), 0),
             ("every digit 1, n times", 12, fr([from_windows([1] * W)]) * (1 << 12), 0),
             # finite and infinite references in one wave, under folded digits (flipped reference signs)
             ("edge + random, every third base infinite", 10, edge_and_random(1 << 10, 22), 3)]
    for name, lg, sc, inf_every in cases:
        n = 1 << lg
        b1, b2 = g1[: 96 * n], g2[: 192 * n]
        if inf_every:
            b1 = b"".join(g1_uncompressed(None) if i % inf_every == 0 else b1[96 * i : 96 * (i + 1)] for i in range(n))
            b2 = b"".join(g2_uncompressed(None) if i % inf_every == 0 else b2[192 * i : 192 * (i + 1)] for i in range(n))
        before = ctx.msm_skew_stats()
        for grp, got, want in (("g1", spx.msm_g1(ctx, b1, sc), oc.msm_g1(b1, sc, n)),
                               ("g2", spx.msm_g2(ctx, b2, sc), oc.msm_g2(b2, sc, n))):
            ok = got == want
            print("%-40s 2^%d %s %s" % (name, lg, grp, "ok" if ok else "DIFFERS"), flush=True)
            if not ok:
                fails.append((name, grp))
        st = ctx.msm_skew_stats()
        print("skew stats", st, flush=True)
        if not name.startswith("edge + random") and st[2] <= before[2]:
            fails.append((name, "no hot bucket reduced", st))
    print("FAILED: %s" % fails if fails else "all equal", flush=True)
    return 1 if fails else 0


def run_proof(spx, oc, d, G, expect, want_reruns):
    with open(os.path.join(d, "pp"), "rb") as f:
        ppb = f.read()
    with open(os.path.join(d, "want"), "rb") as f:
        want = f.read()
    inst = oc.Instance(0, LOG_N, LOG_V, INST_SEED)
    group = spx.CommGroup(G) if G > 1 else None
    out, plans, reruns, errs = [None] * G, [None] * G, [0] * G, []

    def rank(r):
        try:
            c = spx.Context(0)
            if group is not None:
                c.set_comm_group(group, r)
            pp = spx.PublicParameter.load(c, ppb)
            plans[r] = (pp.window_plan(-1), [pp.window_plan(i) for i in range(LOG_N)])
            pk = spx.MLArgumentForR1CS.index(c, *[spx.Csr(M.n, M.row_ptr, M.col, M.val) for M in inst.mats])
            out[r] = spx.MLArgumentForR1CS.prove(pk, inst.v_bytes, inst.w_bytes, pp)
            reruns[r] = c.msm_reruns()
        except Exception as e:
            errs.append(repr(e))

    ths = [threading.Thread(target=rank, args=(r,)) for r in range(G)]
    for t in ths:
        t.start()
    for t in ths:
        t.join(timeout=120)
    fails = list(errs)
    print("plan", plans[0], "reruns", reruns, flush=True)
    for r in range(G):
        if plans[r] != expected_plan(expect, LOG_N):
            fails.append(("rank %d plan" % r, plans[r]))
        elif sum(1 << (c - 1) for c, _ in plans[r][1]) > MAX_BUCKETS:
            fails.append(("rank %d: an opening batch's buckets pass the limit" % r, plans[r]))
        if out[r] != want:
            fails.append("rank %d proof differs" % r)
    if want_reruns and sum(reruns) == 0:
        fails.append("the compacted keys did not overflow")
    print("FAILED: %s" % fails if fails else "all equal", flush=True)
    return 1 if fails else 0


def main():
    here = os.path.dirname(os.path.abspath(__file__))
    sys.path.insert(0, here)
    from conftest import ensure_oracle_lib, load_product

    ensure_oracle_lib()
    import oracle_c as oc

    spx = load_product()
    if sys.argv[1] == "msm":
        return run_msm(spx, oc)
    return run_proof(spx, oc, sys.argv[2], int(sys.argv[3]), sys.argv[4], "reruns" in sys.argv[5:])


if __name__ == "__main__":
    sys.exit(main())
