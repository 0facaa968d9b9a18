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


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
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
    for cached in (True, False):
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
