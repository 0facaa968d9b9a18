#!/usr/bin/env python3
"""Public-parameter structure check, derived verifier parameter and views ("Public-parameter
structure and views") at one size on one GPU.

A generated parameter of --nv variables (default 20). Timed, each the median of --reps runs after
--warmup, host wall time:
  * spx_pp_check_structure, with its two stages (spx_last_timings) and the device time of stage 1's two
    k_fold_check launches, whose algorithmic bytes (3 points per pair) over that time are given as a
    fraction of the 8 TB/s HBM peak; beside spx_pp_check_subgroup and spx_pp_load of the same parameter;
  * spx_pp_derive_vp;
  * spx_pp_view at nv - 2 and nv - 4 with its spx_pp_mem_info, beside spx_pp_load of the same-size
    parameters and theirs; and the device bytes of the parameters of nv - 4 .. nv variables loaded
    natively against one parameter of nv variables with four views.
One JSON line to stdout, and to --out when given."""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402  (its package loader)

HBM_PEAK = 8e12  # bytes / s


def timed(fn, reps, warmup, label):
    ts, last = [], None
    for i in range(warmup + reps):
        t0 = time.perf_counter()
        last = fn()
        dt = time.perf_counter() - t0
        print("%s run %d: %.4f s" % (label, i, dt), file=sys.stderr, flush=True)
        if i >= warmup:
            ts.append(dt)
    return [round(1e3 * statistics.median(ts), 3), round(1e3 * min(ts), 3), round(1e3 * max(ts), 3)], last


def stage_ms(spx, ctx):
    buf = (ctypes.c_double * 32)()
    n = ctypes.c_int(0)
    spx._check(spx.lib().spx_last_timings(ctx.h, buf, 32, ctypes.byref(n)))
    assert n.value == 3
    return [buf[i] / 1e3 for i in range(3)]


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--nv", type=int, default=20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    nv = a.nv
    spx = bench.load_product()
    ctx = spx.Context(0)
    t0 = time.perf_counter()
    pp = spx.MLProofForR1CS.setup(ctx, nv, 0xC0FFEE)
    res = {"tool": "tools/pp_bench.py", "nv": nv, "reps": a.reps, "warmup": a.warmup,
           "pp_generate_ms": round(1e3 * (time.perf_counter() - t0), 1), "pp_mem_info": pp.mem_info()}

    # ---- structure check, stage by stage, beside the subgroup check and a load
    stages = []

    def check():
        assert pp.check_structure() == (0, None, 1)
        stages.append(stage_ms(spx, ctx))

    wall, _ = timed(check, a.reps, a.warmup, "pp_check_structure")
    stages = stages[a.warmup:]
    fold_wall, opening, fold_dev = (statistics.median(s[i] for s in stages) for i in range(3))
    pairs = 2 * ((1 << nv) - 1)  # both curves
    fold_bytes = 3 * ((1 << nv) - 1) * (96 + 192)
    res["check_structure"] = {
        "wall_ms": wall, "stage1_fold_ms": round(fold_wall, 3), "stage2_opening_ms": round(opening, 3),
        "fold_kernels_ms": round(fold_dev, 3), "pairs": pairs, "fold_algorithmic_bytes": fold_bytes,
        "fold_fraction_of_hbm_peak": round(fold_bytes / (fold_dev / 1e3) / HBM_PEAK, 4)}
    res["check_subgroup_ms"], _ = timed(lambda: pp.check_subgroup(), a.reps, a.warmup, "pp_check_subgroup")
    res["derive_vp_ms"], vp = timed(lambda: pp.derive_vp(), a.reps, a.warmup, "pp_derive_vp")
    assert vp == spx.verifier_parameter(pp)
    data = pp.serialize_uncompressed()
    res["pp_bytes"] = len(data)

    def load(b):
        return lambda: spx.PublicParameter.load(ctx, b)

    res["pp_load_ms"], _ = timed(load(data), min(a.reps, 3), 1, "pp_load")
    del data

    # ---- views beside native loads of the same sizes
    res["views"] = {}
    native_total, view_total = pp.mem_info()[0], pp.mem_info()[0]
    for k in (1, 2, 3, 4):
        m = nv - k
        if m < 1:
            break
        ms, view = timed(lambda: pp.view(m), a.reps, a.warmup, "pp_view(%d)" % m)
        vb = view.serialize_uncompressed()
        lms, native = timed(load(vb), min(a.reps, 3), 1, "pp_load(%d)" % m)
        assert native.serialize_uncompressed() == vb
        del vb
        native_total += native.mem_info()[0]
        view_total += view.mem_info()[0]
        if k in (2, 4):
            res["views"][str(m)] = {"view_ms": ms, "view_mem_info": view.mem_info(), "load_ms": lms,
                                    "load_mem_info": native.mem_info()}
        del view, native
    res["device_bytes_native_%d_to_%d" % (max(nv - 4, 1), nv)] = native_total
    res["device_bytes_one_parameter_and_views"] = view_total
    line = json.dumps(res)
    print(line, flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
