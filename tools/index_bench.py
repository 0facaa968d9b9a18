#!/usr/bin/env python3
"""Time of spx_index with the host builder and with the GPU builder (spx_ctx_set_index_build), one GPU,
one process.

Workloads: circuit-3n (spx_synth kind 3) at 2^16 and 2^20, ref-shaped (kind 1: one dense row of about n
entries in A and B) at 2^16. For each, the two builders alternate on one context: one warm-up each, then
the median of --reps calls each. Timed is the C call spx_index through ctypes on the generator's arrays
(no Python conversions: this is not bench.py's index_s), host wall clock around the call. Beside it, from
spx_index_stats: the call's own wall time, the part of it the calling thread spent absorbing A, B, C into
the cached transcript, and for the GPU builder the device time of its kernels (HIP events,
spx_last_timings[0]). The host builder at this commit is the yardstick.
JSON to stdout and to --out (default profiles/index_bench.json)."""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402  (its package loader and generator bindings)

WORKLOADS = [("circuit-3n", 3, 16), ("circuit-3n", 3, 20), ("ref-shaped", 1, 16)]


def one_build(spx, L, ctx, mats, mode):
    ctx.set_index_build(mode)
    h = ctypes.c_void_p()
    a, b, c = mats
    t0 = time.perf_counter()
    rc = L.spx_index(ctx.h, ctypes.byref(a), ctypes.byref(b), ctypes.byref(c), ctypes.byref(h))
    wall = (time.perf_counter() - t0) * 1e3
    spx._check(rc)
    st = (ctypes.c_uint64 * 8)()
    spx._check(L.spx_index_stats(h, st))
    assert st[0] == mode
    kern = list(ctx.last_timings().values())[0] / 1e3 if mode == 1 else 0.0
    spx._check(L.spx_index_free(h))
    return {"wall_ms": wall, "call_ms": st[6] / 1e3, "absorb_ms": st[7] / 1e3, "kernels_ms": kern}, list(st)[1:6]


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--log-v", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "index_bench.json"))
    a = ap.parse_args()
    spx = bench.load_product()
    L = spx.lib()
    ctx = spx.Context(0)
    res = {"tool": "tools/index_bench.py", "reps": a.reps, "timed": "spx_index through ctypes, host wall ms, median",
           "workloads": []}
    for name, kind, log_n in WORKLOADS:
        # the generator's param: the witness seed of circuit-3n, the density (0: one dense row) of ref-shaped
        syn, mats, _, nnz = bench.synth_instance(spx, kind, log_n, a.log_v, 0x5EED0000 + log_n, 1, 0xB0B0 if kind == 3 else 0)
        runs = {0: [], 1: []}
        shape = None
        for rep in range(a.reps + 1):  # rep 0: the warm-up of each builder
            for mode in (0, 1):
                r, st = one_build(spx, L, ctx, mats, mode)
                assert shape in (None, st), "the builders disagree on the index's shape"
                shape = st
                if rep:
                    runs[mode].append(r)
        row = {"workload": name, "log_n": log_n, "nnz": nnz, "sliced": shape[0], "long_rows": shape[3], "long_cols": shape[4]}
        for mode, key in ((0, "host"), (1, "gpu")):
            row[key] = {k: round(statistics.median(r[k] for r in runs[mode]), 3) for k in runs[mode][0]}
            row[key]["wall_ms_min"] = round(min(r["wall_ms"] for r in runs[mode]), 3)
            row[key]["wall_ms_max"] = round(max(r["wall_ms"] for r in runs[mode]), 3)
            row[key]["absorb_share"] = round(row[key]["absorb_ms"] / row[key]["call_ms"], 3)
        row["host_over_gpu"] = round(row["host"]["wall_ms"] / row["gpu"]["wall_ms"], 2)
        res["workloads"].append(row)
        L.spx_synth_free(syn)
    ctx.set_index_build(0)
    print(json.dumps(res), flush=True)
    with open(a.out, "w") as f:
        f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
