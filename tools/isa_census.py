#!/usr/bin/env python3
"""Static census of the vector instructions a kernel issues per mixed addition.

    tools/isa_census.py r1cs-spartan_amd/csrc/msm_g2.hip 'k_accum_aff<spx::Fq2>' [-D NAME=V ...]
    tools/isa_census.py --asm file.s KERNEL          (an assembly file made elsewhere)

Compiles one translation unit for gfx950 to assembly in a temporary directory (device pass only,
the library's flags), takes the named kernel (a substring of the demangled or mangled name), splits
its code into basic blocks at the labels, and prints per vector opcode the count and the weighted
issue slots over the blocks of the mixed-addition path, with the kernel's registers, scratch and
waves per SIMD. It needs no GPU.

The path: the compiler keeps the straight-line formula of x29_madd in a few large blocks (the U2 / S2
products, then everything from PP to ZZZ3) and the doubling exit (x29_from_aff_dbl) in another. With
--mads N (the limb products one mixed addition must hold: 5292 for G2, 3542 for G1) the path is
the large blocks, largest first, whose products fit N, plus what is left from the small blocks
between them in program order; it is an error if no such set holds exactly N. Without --mads every
block with at least --min-mads products counts (the doubling exit included). --blocks lists every
block, so the choice can be checked by eye; --path L1,L2 names the blocks.

Only instruction lines whose opcode begins with v_ are read. Weights are issue slots at two waves
per SIMD (tools/ubench_issue.hip): the opcodes of WEIGHT2 take two, every other
vector opcode one.
"""
import argparse
import collections
import os
import re
import subprocess
import sys
import tempfile

WEIGHT2 = ("v_mad_u64_u32", "v_mul_lo_u32", "v_mul_hi_u32", "v_lshrrev_b64", "v_lshlrev_b64", "v_lshl_add_u64")
FLAGS = ["-O3", "-std=c++17", "--offload-arch=gfx950", "--cuda-device-only", "-S"]


def compile_asm(src, defines, out):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    cmd = [hipcc] + FLAGS + ["-D" + d for d in defines] + ["-I", os.path.dirname(os.path.abspath(src)), src, "-o", out]
    subprocess.run(cmd, check=True, stderr=subprocess.DEVNULL)


def demangle(names):
    try:
        out = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True).stdout
        return out.splitlines()
    except (OSError, subprocess.CalledProcessError):
        return names


def kernel_body(lines, want):
    """(mangled name, body lines) of the one kernel whose mangled or demangled name contains `want`."""
    names = [m.group(1) for m in (re.match(r"\s*\.amdhsa_kernel\s+(\S+)", l) for l in lines) if m]
    hits = [n for n, d in zip(names, demangle(names)) if want in n or want in d]
    if len(hits) != 1:
        sys.exit("kernel %r matches %d of the %d kernels:\n  %s" % (want, len(hits), len(names), "\n  ".join(demangle(names))))
    name = hits[0]
    start = lines.index(name + ":") if (name + ":") in lines else next(
        i for i, l in enumerate(lines) if l.startswith(name + ":"))
    end = next(i for i in range(start, len(lines)) if lines[i].startswith(".Lfunc_end"))
    return name, lines[start + 1:end]


def blocks_of(body):
    """[(label, Counter of v_ opcodes)] in program order; a block starts at every label."""
    out = [("entry", collections.Counter())]
    for l in body:
        s = l.strip()
        m = re.match(r"(\.?[A-Za-z_][\w.$]*):", s)
        if m:
            out.append((m.group(1), collections.Counter()))
            continue
        if s.startswith("v_"):
            op = s.split()[0]
            for suf in ("_e32", "_e64", "_sdwa"):
                if op.endswith(suf):
                    op = op[: -len(suf)]
            out[-1][1][op] += 1
    return out


def meta(lines, name):
    g = {}
    for key in ("num_vgpr", "num_agpr", "private_seg_size"):
        m = next((re.search(r",\s*(\d+)\s*$", l) for l in lines if l.startswith("\t.set %s.%s," % (name, key)) or
                  l.strip().startswith(".set %s.%s," % (name, key))), None)
        g[key] = int(m.group(1)) if m else None
    v = (g["num_vgpr"] or 0) + (g["num_agpr"] or 0)
    alloc = max(8, (v + 7) // 8 * 8)
    g["waves_per_simd"] = min(8, 512 // alloc)
    return g


def weight(op):
    return 2 if op in WEIGHT2 else 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("src")
    ap.add_argument("kernel")
    ap.add_argument("--asm", action="store_true", help="src is an assembly file already")
    ap.add_argument("-D", action="append", default=[], dest="defines")
    ap.add_argument("--mads", type=int, default=0, help="limb products per mixed addition expected on the path")
    ap.add_argument("--path", default="", help="comma-separated block labels of the path")
    ap.add_argument("--min-mads", type=int, default=150, help="a path block holds at least this many limb products")
    ap.add_argument("--blocks", action="store_true", help="list every block that holds vector instructions")
    a = ap.parse_args()

    if a.asm:
        lines = open(a.src).read().splitlines()
    else:
        with tempfile.TemporaryDirectory() as d:
            out = os.path.join(d, "unit.s")
            compile_asm(a.src, a.defines, out)
            lines = open(out).read().splitlines()
    name, body = kernel_body(lines, a.kernel)
    blks = blocks_of(body)
    g = meta(lines, name)
    print("kernel %s" % demangle([name])[0])
    print("VGPRs %s  AGPRs %s  ScratchSize: %s  waves per SIMD %d" %
          (g["num_vgpr"], g["num_agpr"], g["private_seg_size"], g["waves_per_simd"]))
    MAD = WEIGHT2[0]
    if a.blocks:
        for lab, c in blks:
            if c:
                print("  block %-12s %6d vector instructions, %5d limb products" % (lab, sum(c.values()), c[MAD]))
    if a.path:
        want = set(a.path.split(","))
        path = [(l, c) for l, c in blks if l in want]
    else:
        big = [i for i, (l, c) in enumerate(blks) if c[MAD] >= a.min_mads]
        if a.mads:
            # the large blocks, largest first, while they fit the expected product count; what is
            # left (a column's first product scheduled into a neighbouring small block) from the
            # small blocks that lie between them in program order
            take, left = [], a.mads
            for i in sorted(big, key=lambda i: -blks[i][1][MAD]):
                if blks[i][1][MAD] <= left:
                    take.append(i)
                    left -= blks[i][1][MAD]
            for i in range(min(take, default=0), max(take, default=0)):
                k = blks[i][1][MAD]
                if i not in big and 0 < k <= left:
                    take.append(i)
                    left -= k
            if left:
                sys.exit("no set of blocks holds exactly %d limb products (list them with --blocks)" % a.mads)
            big = sorted(take)
        path = [blks[i] for i in big]
    tot = collections.Counter()
    for _, c in path:
        tot.update(c)
    print("path blocks: %s" % ", ".join("%s (%d)" % (l, sum(c.values())) for l, c in path))
    n = sum(tot.values())
    slots = sum(k * weight(op) for op, k in tot.items())
    print("%-24s %7s %7s" % ("opcode", "count", "slots"))
    for op, k in sorted(tot.items(), key=lambda kv: -kv[1] * weight(kv[0])):
        print("%-24s %7d %7d" % (op, k, k * weight(op)))
    prod = tot[MAD]
    print("%-24s %7d %7d" % ("total", n, slots))
    print("limb products %d (%.1f%% of the instructions, %.1f%% of the slots); other %d instructions, %d slots" %
          (prod, 100.0 * prod / max(n, 1), 200.0 * prod / max(slots, 1), n - prod, slots - 2 * prod))


if __name__ == "__main__":
    main()
