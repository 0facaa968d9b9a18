#!/usr/bin/env python3
"""Verifier throughput: a loop of spx_verify against one spx_verify_many over the same proofs.

Index: bench.py's circuit-3n at 2^log_n with --batch distinct witnesses, each proved once. Timed, with
the index-cached matrix transcript and without it:
  (i)  a loop of spx_verify over the proofs (the single-proof path: two products of log_n + 1 pairings
       and 2 (log_n + 1) + 1 host decompressions per proof);
  (ii) one spx_verify_many over the same proofs (one product of log_n + 2 pairings per batch, the points
       decompressed and combined on the GPU).
Each figure is the median of --reps runs after --warmup, host wall time, with the spx_verify_stats
deltas of one (ii) run. One JSON line to stdout, and to --out when given."""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402  (its package loader and headline workload)


def timed(fn, reps, warmup, label):
    ts = []
    for i in range(warmup + reps):
        t0 = time.perf_counter()
        fn()
        dt = time.perf_counter() - t0
        print("%s run %d: %.3f s" % (label, i, dt), file=sys.stderr, flush=True)
        if i >= warmup:
            ts.append(dt)
    return statistics.median(ts), min(ts), max(ts)


PHASES = ["parse_replay", "algebra", "points_wait", "matrix_eval", "combine", "pairing", "single_path"]


def phase_ms(spx, ctx):
    """host wall ms of the last spx_verify_many's phases (spx_last_timings)"""
    buf = (ctypes.c_double * 32)()
    n = ctypes.c_int(0)
    spx._check(spx.lib().spx_last_timings(ctx.h, buf, 32, ctypes.byref(n)))
    return {PHASES[i]: round(buf[i] / 1e3, 3) for i in range(min(n.value, len(PHASES)))}


def subgroup_arms(spx, ctx, pk, pp, vs, proofs, vp, a, res):
    """--subgroup: spx_verify_many with the subgroup check off and on (the same protocol as the default
    run's verify_many figure; the off arm is that figure again), then spx_pp_check_subgroup of the public
    parameter beside spx_pp_load of its bytes and the host function's per-point time x the point count."""
    A = spx.MLArgumentForR1CS
    for cached in (True, False):
        key = "cached" if cached else "uncached"
        res[key] = {}

        def many():
            assert A.verify_many(pk, vs, proofs, vp, cached=cached) == [True] * len(proofs)

        arms = ((0, "check_off"), (1, "check_on"))
        ts, last = {0: [], 1: []}, {}
        warm = a.warmup + 1  # the default run's untimed first call and its warm-up
        for i in range(warm + a.reps):  # the two arms alternate, so drift falls on both
            for mode, arm in arms:
                ctx.set_subgroup_check(mode)
                s0, g0 = spx.verify_stats(ctx), ctx.subgroup_stats()
                t0 = time.perf_counter()
                many()
                dt = time.perf_counter() - t0
                print("%s %s verify_many run %d: %.3f s" % (key, arm, i, dt), file=sys.stderr, flush=True)
                # the counters' deltas and the phases of the arm's last run
                last[mode] = (s0, g0, spx.verify_stats(ctx), ctx.subgroup_stats(), phase_ms(spx, ctx))
                if i >= warm:
                    ts[mode].append(dt)
        for mode, arm in arms:
            s0, g0, s1, g1, phases = last[mode]
            med, lo, hi = statistics.median(ts[mode]), min(ts[mode]), max(ts[mode])
            res[key][arm] = {
                "verify_many_ms_per_proof": round(1e3 * med / a.batch, 3),
                "verify_many_s": [round(med, 4), round(lo, 4), round(hi, 4)],
                "verify_stats_delta": [y - x for x, y in zip(s0, s1)],
                "subgroup_stats_delta": [y - x for x, y in zip(g0, g1)],
                "verify_many_phase_ms": phases}
        ctx.set_subgroup_check(0)
        res[key]["strict_cost_ms_per_batch"] = round(
            1e3 * (res[key]["check_on"]["verify_many_s"][0] - res[key]["check_off"]["verify_many_s"][0]), 3)
    # the public parameter
    nv = a.log_n
    npts = 2 * ((2 << nv) - 2) + 2
    med, lo, hi = timed(lambda: pp.check_subgroup(), a.reps, a.warmup, "pp_check_subgroup")
    data = pp.serialize_uncompressed()
    h = ctypes.c_void_p()

    def load():
        spx._check(spx.lib().spx_pp_load(ctx.h, data, len(data), ctypes.byref(h)))
        spx._check(spx.lib().spx_pp_free(h))

    l_med, l_lo, l_hi = timed(load, min(a.reps, 3), 1, "pp_load")
    # the host function on the first points of level 0 of each curve
    k = 32
    g1_at = 24
    g2_at = 16 + sum(8 + (96 << (nv - i)) for i in range(nv)) + 16
    host = {}
    for cid, at, ps in ((1, g1_at, 96), (2, g2_at, 192)):
        pts = [data[at + ps * j : at + ps * (j + 1)] for j in range(k)]
        t0 = time.perf_counter()
        assert all(spx.point_in_subgroup_host(cid, p) for p in pts)
        host[cid] = (time.perf_counter() - t0) / k
    res["pp"] = {
        "nv": nv, "points": npts, "bytes": len(data),
        "pp_check_subgroup_ms": [round(1e3 * med, 3), round(1e3 * lo, 3), round(1e3 * hi, 3)],
        "pp_load_ms": [round(1e3 * l_med, 3), round(1e3 * l_lo, 3), round(1e3 * l_hi, 3)],
        "host_us_per_point": {"g1": round(1e6 * host[1], 2), "g2": round(1e6 * host[2], 2)},
        "host_alternative_ms": round(1e3 * (npts // 2) * (host[1] + host[2]), 1)}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--subgroup", action="store_true",
                    help="measure the subgroup membership checks instead: spx_verify_many with the check off and on, "
                         "and spx_pp_check_subgroup beside spx_pp_load and the host function (DESIGN 6b)")
    ap.add_argument("--log-n", type=int, default=16)
    ap.add_argument("--log-v", type=int, default=5)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    spx = bench.load_product()
    n, nv = 1 << a.log_n, 32 << a.log_v
    ctx = spx.Context(0)
    pp = spx.MLProofForR1CS.setup(ctx, a.log_n, 0xC0FFEE)
    vp = spx.verifier_parameter(pp)
    syn, mats, zs, _ = bench.synth_instance(spx, 3, a.log_n, a.log_v, 0x5EED0000 + a.log_n, a.batch, 0xB0B0)
    pk = spx.IndexPK(ctx, bench.index_from_c(spx, ctx, mats), a.log_n)
    vs = [z[:nv] for z in zs]
    proofs = [spx.MLArgumentForR1CS.prove(pk, z[:nv], z[nv:], pp, cached=True) for z in zs]
    del zs
    print("proved %d proofs of %d bytes" % (len(proofs), len(proofs[0])), file=sys.stderr, flush=True)
    res = {"tool": "tools/verify_bench.py", "log_n": a.log_n, "batch": a.batch, "reps": a.reps, "warmup": a.warmup,
           "proof_bytes": len(proofs[0])}
    A = spx.MLArgumentForR1CS
    if a.subgroup:
        res["tool"] += " --subgroup"
        subgroup_arms(spx, ctx, pk, pp, vs, proofs, vp, a, res)
    for cached in (() if a.subgroup else (True, False)):
        def loop():
            for v, p in zip(vs, proofs):
                assert A.verify(pk, v, p, vp, cached=cached)

        def many():
            assert A.verify_many(pk, vs, proofs, vp, cached=cached) == [True] * len(proofs)

        key = "cached" if cached else "uncached"
        s0 = spx.verify_stats(ctx)
        many()
        s1 = spx.verify_stats(ctx)
        phases = phase_ms(spx, ctx)
        m_med, m_min, m_max = timed(many, a.reps, a.warmup, key + " verify_many")
        l_med, l_min, l_max = timed(loop, a.reps, a.warmup, key + " verify loop")
        res[key] = {
            "verify_loop_ms_per_proof": round(1e3 * l_med / a.batch, 3),
            "verify_many_ms_per_proof": round(1e3 * m_med / a.batch, 3),
            "verify_loop_s": [round(l_med, 4), round(l_min, 4), round(l_max, 4)],
            "verify_many_s": [round(m_med, 4), round(m_min, 4), round(m_max, 4)],
            "speedup": round(l_med / m_med, 2),
            "verify_stats_delta": [y - x for x, y in zip(s0, s1)],
            "verify_many_phase_ms": phases}
    line = json.dumps(res)
    print(line, flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
