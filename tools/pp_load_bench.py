#!/usr/bin/env python3
"""The compressed public-parameter form beside the uncompressed one ("Compressed public
parameters") on one GPU, at 2^16 and 2^20 (--nv).

Per size, a generated parameter; each figure the median of --reps runs after one warm-up, with the smallest
and the largest beside it:
  * host wall time of spx_pp_load and spx_pp_load_compressed, of spx_pp_serialize and
    spx_pp_serialize_compressed (each call ends in a device synchronise);
  * device time (an event pair around the kernel, the first entry of spx_last_timings) of the bulk
    decompression kernel of each curve over all 2^(nv+1) - 2 points of the parameter, and, in the same run and
    alternating with it, of the batch verifier's k_decompress over the same bytes (spx_g1_decompress /
    spx_g2_decompress record the same event pair); the ratio new / parent per point with its spread;
  * device time of the compression kernels over the same points.
The outputs of the two decompression kernels are compared before anything is timed.
One JSON line to stdout, and the whole result to --out."""
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


def med(ts, scale=1.0, digits=3):
    return [round(scale * statistics.median(ts), digits), round(scale * min(ts), digits), round(scale * max(ts), digits)]


def timed(fn, reps, label):
    ts, last = [], None
    for i in range(1 + reps):
        t0 = time.perf_counter()
        last = fn()
        dt = time.perf_counter() - t0
        print("%s run %d: %.4f s" % (label, i, dt), file=sys.stderr, flush=True)
        if i >= 1:
            ts.append(dt)
    return med(ts, 1e3), last


def kernel_us(spx, ctx, name):
    buf = (ctypes.c_double * 8)()
    n = ctypes.c_int(0)
    spx._check(spx.lib().spx_last_timings(ctx.h, buf, 8, ctypes.byref(n)))
    assert n.value >= 1, name
    return buf[0]


def points(data, nv, compressed):
    """the G1 and the G2 points of a serialized parameter, levels concatenated"""
    g1s = 48 if compressed else 96
    pos, out = 16, []
    for ps in (g1s, 2 * g1s):
        parts = []
        for i in range(nv):
            pos += 8
            parts.append(data[pos:pos + (ps << (nv - i))])
            pos += ps << (nv - i)
        pos += 8
        out.append(b"".join(parts))
    return out


def one_size(spx, ctx, nv, reps):
    t0 = time.perf_counter()
    pp = spx.MLProofForR1CS.setup(ctx, nv, 0xC0FFEE + nv)
    res = {"nv": nv, "points_per_curve": (2 << nv) - 2, "pp_generate_ms": round(1e3 * (time.perf_counter() - t0), 1)}
    res["serialize_uncompressed_ms"], unc = timed(pp.serialize_uncompressed, reps, "serialize %d" % nv)
    res["serialize_compressed_ms"], img = timed(pp.serialize_compressed, reps, "serialize_compressed %d" % nv)
    res["bytes"] = {"uncompressed": len(unc), "compressed": len(img)}
    del pp
    res["load_ms"], a = timed(lambda: spx.PublicParameter.load(ctx, unc), reps, "load %d" % nv)
    del a
    res["load_compressed_ms"], b = timed(lambda: spx.PublicParameter.load_compressed(ctx, img), reps, "load_compressed %d" % nv)
    assert b.serialize_uncompressed() == unc
    del b
    cpts, upts = points(img, nv, True), points(unc, nv, False)
    del img, unc
    n = res["points_per_curve"]
    res["kernels"] = {}
    for cid, name in ((1, "g1"), (2, "g2")):
        bulk, parent, compress = [getattr(spx, "%s_%s" % (name, f)) for f in ("decompress_bulk", "decompress", "compress")]
        data = cpts[cid - 1]
        assert bulk(ctx, data) == parent(ctx, data) and bulk(ctx, data)[0] == upts[cid - 1]  # also the warm-up
        tb, tp = [], []
        for i in range(reps):  # alternating
            bulk(ctx, data)
            tb.append(kernel_us(spx, ctx, "bulk"))
            parent(ctx, data)
            tp.append(kernel_us(spx, ctx, "parent"))
            print("%s 2^%d run %d: bulk %.1f us, k_decompress %.1f us" % (name, nv, i, tb[-1], tp[-1]), file=sys.stderr, flush=True)
        assert compress(ctx, upts[cid - 1]) == data
        tc = []
        for i in range(reps):
            compress(ctx, upts[cid - 1])
            tc.append(kernel_us(spx, ctx, "compress"))
        ratios = [x / y for x, y in zip(tb, tp)]
        res["kernels"][name] = {
            "decompress_bulk_us": med(tb, digits=1), "k_decompress_us": med(tp, digits=1),
            "decompress_bulk_ns_per_point": round(1e3 * statistics.median(tb) / n, 2),
            "k_decompress_ns_per_point": round(1e3 * statistics.median(tp) / n, 2),
            "ratio_new_over_parent": med(ratios, digits=4), "compress_us": med(tc, digits=1)}
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--nv", type=int, nargs="+", default=[16, 20])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pp_compressed.json"))
    a = ap.parse_args()
    spx = bench.load_product()
    ctx = spx.Context(0)
    res = {"tool": "tools/pp_load_bench.py", "reps": a.reps, "warmup": 1, "format": "[median, min, max]",
           "stage_log": os.environ.get("SPX_PP_STAGE_LOG", "default (20)"), "sizes": [one_size(spx, ctx, nv, a.reps) for nv in a.nv]}
    print(json.dumps(res), flush=True)
    with open(a.out, "w") as f:
        f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
