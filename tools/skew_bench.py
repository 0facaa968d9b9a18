#!/usr/bin/env python3
"""Running time of the prover on skewed scalars (0 / 1 witnesses) against uniform ones, with the MSM's
hot-bucket reduction on and off (spx_ctx_set_msm_hot).

Index: the booleanity circuit at 2^log_n (A = B = C = identity: row i is z_i * z_i = z_i). Witnesses of
that one index: seeded random bits (satisfying), and uniform random Fr (unsatisfying; the prover does
the same work as on the benchmark's witnesses). For each witness and each of hot = on, off:
  * index-cached single-proof latency, one proof in flight: median of --proofs after --warmup, host wall
    around spx_prove_witness as bench.py times it;
  * spx_kernel_stats per proof of the MSM ids (sort, accumulation, weighting);
  * spx_msm_skew_stats.
One throughput line: --inflight proofs in flight, bits witness, on and off. With --headline, bench.py's
headline workload (its circuit-3n index and 64 distinct witnesses, one step) is proved once and the
contexts' skew statistics summed: its batches with a hot bucket must be 0.
JSON to stdout and to --out (default profiles/skew_bench.json)."""
import argparse
import ctypes
import json
import os
import random
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402  (its package loader, kernel names and headline workload)

R = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001
MSM_IDS = {"msm_sort": 6, "msm_acc_g1": 7, "msm_acc_g2": 8, "msm_accx_g1": 9, "msm_accx_g2": 10, "msm_reduce_g1": 11,
           "msm_reduce_g2": 12}


def identity_csr(spx, n):
    rp = (ctypes.c_uint64 * (n + 1)).from_buffer_copy(np.arange(n + 1, dtype=np.uint64).tobytes())
    col = (ctypes.c_uint32 * n).from_buffer_copy(np.arange(n, dtype=np.uint32).tobytes())
    one = np.zeros((n, 32), dtype=np.uint8)
    one[:, 0] = 1
    return spx.Csr(n, rp, col, one.tobytes())


def bits_witness(n, seed):
    z = np.zeros((n, 32), dtype=np.uint8)
    z[:, 0] = np.random.default_rng(seed).integers(0, 2, n, dtype=np.uint8)
    z[0, 0] = 1
    return z.tobytes()


def uniform_witness(n, seed):
    rs = random.Random(seed)
    out = bytearray(32 * n)
    for i in range(n):
        x = rs.getrandbits(255)
        while x >= R:
            x = rs.getrandbits(255)
        out[32 * i : 32 * i + 32] = x.to_bytes(32, "little")
    return bytes(out)


def msm_kernel_stats(spx, L, c, div):
    out = {}
    for name, k in MSM_IDS.items():
        cnt, ms, by = ctypes.c_uint64(), ctypes.c_double(), ctypes.c_double()
        spx._check(L.spx_kernel_stats(c.h, k, ctypes.byref(cnt), ctypes.byref(ms), ctypes.byref(by)))
        out[name] = {"launches": cnt.value / div, "ms": round(ms.value / div, 4)}
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--log-n", type=int, default=20)
    ap.add_argument("--log-v", type=int, default=5)
    ap.add_argument("--proofs", type=int, default=20, help="timed proofs per latency figure (median)")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--inflight", type=int, default=8)
    ap.add_argument("--throughput-proofs", type=int, default=48)
    ap.add_argument("--headline", action="store_true", help="also prove bench.py's headline witnesses and report their skew")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "skew_bench.json"))
    a = ap.parse_args()
    spx = bench.load_product()
    L = spx.lib()
    n, nv = 1 << a.log_n, 32 << a.log_v
    ctxs = {"on": spx.Context(0), "off": spx.Context(0)}
    ctxs["on"].set_msm_hot(1)
    ctxs["off"].set_msm_hot(0)
    pp = spx.MLProofForR1CS.setup(ctxs["on"], a.log_n, 0xC0FFEE)
    M = identity_csr(spx, n)
    pks = {m: spx.MLArgumentForR1CS.index(c, M, M, M) for m, c in ctxs.items()}
    zs = {"uniform": uniform_witness(n, 2), "bits": bits_witness(n, 1)}
    res = {"tool": "tools/skew_bench.py", "log_n": a.log_n, "index": "booleanity (A = B = C = identity)",
           "proofs": a.proofs, "warmup": a.warmup, "latency": {}, "throughput": {}}
    proofs = {}
    for wname in ("uniform", "bits"):  # uniform first: the cumulative leaf maximum then shows the bits witness's
        z = zs[wname]
        res["latency"][wname] = {}
        for mode, c in ctxs.items():
            wit = spx.Witness(c, z[:nv], z[nv:])
            run = lambda: spx.MLArgumentForR1CS.prove_witness(pks[mode], wit, pp, mode="fs", seed=7, cached=True)
            for _ in range(a.warmup):
                p = run()
            proofs.setdefault(wname, p)
            assert p == proofs[wname], "hot on / off gave different proofs"
            s0 = c.msm_skew_stats()
            ts = []
            for _ in range(a.proofs):
                t0 = time.perf_counter()
                run()
                ts.append((time.perf_counter() - t0) * 1e3)
            # kernel durations in a pass of their own (the events add host work to the timed one)
            spx._check(L.spx_kernel_stats_enable(c.h, 1))
            for _ in range(3):
                run()
            ks = msm_kernel_stats(spx, L, c, 3)
            spx._check(L.spx_kernel_stats_enable(c.h, 0))
            s1 = c.msm_skew_stats()
            res["latency"][wname][mode] = {
                "ms_median": round(statistics.median(ts), 3), "ms_min": round(min(ts), 3), "ms_max": round(max(ts), 3),
                "kernels_per_proof": ks,
                "msm_ms_per_proof": round(sum(v["ms"] for v in ks.values()), 3),
                "skew_stats_delta": [s1[0] - s0[0], s1[1] - s0[1], s1[2] - s0[2]], "leaf_max_cumulative": s1[3]}
            del wit
    lat = res["latency"]
    res["bits_over_uniform_hot_on"] = round(lat["bits"]["on"]["ms_median"] / lat["uniform"]["on"]["ms_median"], 4)
    res["bits_over_uniform_hot_off"] = round(lat["bits"]["off"]["ms_median"] / lat["uniform"]["off"]["ms_median"], 4)
    # throughput: --inflight proofs in flight, bits witness
    tctx = [spx.Context(0) for _ in range(a.inflight)]
    wit = spx.Witness(tctx[0], zs["bits"][:nv], zs["bits"][nv:])
    tpk = spx.MLArgumentForR1CS.index(tctx[0], M, M, M)
    for mode, flag in (("on", 1), ("off", 0)):
        for c in tctx:
            c.set_msm_hot(flag)
        many = lambda k: spx.MLArgumentForR1CS.prove_many(tctx, tpk, [wit] * k, pp, mode="fs", seed=7, cached=True)
        many(2 * a.inflight)
        t0 = time.perf_counter()
        got = many(a.throughput_proofs)
        el = time.perf_counter() - t0
        assert all(p == proofs["bits"] for p in got)
        res["throughput"][mode] = {"proofs_in_flight": a.inflight, "proofs": a.throughput_proofs,
                                   "proofs_per_s": round(a.throughput_proofs / el, 2),
                                   "constraints_per_s": round(a.throughput_proofs * n / el, 1)}
    del wit, tpk
    if a.headline:
        P = 64
        syn, mats, hz, _ = bench.synth_instance(spx, 3, a.log_n, a.log_v, 0x5EED0000 + a.log_n, P, 0xB0B0)
        hctx = [spx.Context(0) for _ in range(a.inflight)]
        hpk = spx.IndexPK(hctx[0], bench.index_from_c(spx, hctx[0], mats), a.log_n)
        hw = [spx.Witness(hctx[0], z[:nv], z[nv:]) for z in hz]
        del hz
        spx.MLArgumentForR1CS.prove_many(hctx, hpk, hw, pp, mode="fs", seed=7)
        tot = [0, 0, 0, 0]
        for c in hctx:
            s = c.msm_skew_stats()
            tot = [tot[0] + s[0], tot[1] + s[1], tot[2] + s[2], max(tot[3], s[3])]
        res["headline_witnesses"] = {"workload": "bench.py circuit-3n 2^%d, %d distinct witnesses, one step" % (a.log_n, P),
                                     "skew_stats": tot}
        assert tot[1] == 0, "bench.py's witnesses took the hot path: %s" % tot
        del hw, hpk
    line = json.dumps(res)
    print(line, flush=True)
    with open(a.out, "w") as f:
        f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
