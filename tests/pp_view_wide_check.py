"""A view whose shared levels carry the wide MSM window plan, run by tests/test_gpu_pp_view.py as a child
process so that SPX_MSM_WIDE_MIN_LOG=8 is in place before the library preprocesses a public parameter.

The nv = 12 parent then has 17-bit windows on levels 0 .. 3 (2^11 .. 2^8 points); its nv = 10 view shares
levels 2 .. 11, of which the first two are wide. spx_pp_window_plan(view, j) must report the parent's plan
of level 2 + j, the commitment table is the view's own (2^10 points: wide), and a proof, a commitment and an
opening made with the view must equal those made with the same bytes loaded natively.
Exit status 0 = all equal."""
import os
import random
import sys

R = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001
PARENT_NV, VIEW_NV, WIDE_MIN = 12, 10, 8
PP_SEED, INST_SEED = 0x71E5, 0x71E6


def level_bits(nv, wide_min):
    """window bits of the opening levels (2^(nv - i - 1) points) under SPX_MSM_WIDE_MIN_LOG = wide_min"""
    out = []
    for i in range(nv):
        k = nv - i - 1
        out.append(17 if wide_min and k >= wide_min else 16 if k >= 14 else max(3, k - 2))
    return out


def main():
    here = os.path.dirname(os.path.abspath(__file__))
    sys.path.insert(0, here)
    from conftest import ensure_oracle_lib, load_product

    ensure_oracle_lib()
    import oracle_c as oc

    spx = load_product()
    assert os.environ.get("SPX_MSM_WIDE_MIN_LOG") == str(WIDE_MIN)
    ctx = spx.Context(0)
    parent = spx.MLProofForR1CS.setup(ctx, PARENT_NV, PP_SEED)
    view = parent.view(VIEW_NV)
    native = spx.PublicParameter.load(ctx, view.serialize_uncompressed())
    k = PARENT_NV - VIEW_NV
    fails = []
    pplan = [parent.window_plan(i) for i in range(PARENT_NV)]
    vplan = [view.window_plan(j) for j in range(VIEW_NV)]
    print("parent", pplan, "view", vplan, "commitment", view.window_plan(-1), flush=True)
    if [c for c, _ in pplan] != level_bits(PARENT_NV, WIDE_MIN):
        fails.append("parent plan")
    if vplan != pplan[k:] or [c for c, _ in vplan[:2]] != [17, 17]:
        fails.append("view plan is not the parent's")
    if view.window_plan(-1) != (17, 15) or view.window_plan(-1) != native.window_plan(-1):
        fails.append("commitment plan")
    inst = oc.Instance(0, VIEW_NV, 3, INST_SEED)
    pk = spx.MLArgumentForR1CS.index(ctx, *[spx.Csr(M.n, M.row_ptr, M.col, M.val) for M in inst.mats])
    got = spx.MLArgumentForR1CS.prove(pk, inst.v_bytes, inst.w_bytes, view)
    if got != spx.MLArgumentForR1CS.prove(pk, inst.v_bytes, inst.w_bytes, native):
        fails.append("proof differs from the native load's")
    if got != oc.prove(inst.mats, inst.v_bytes, inst.w_bytes, oc.PP.load(native.serialize_uncompressed()), 0, 0):
        fails.append("proof differs from the oracle's")
    rs = random.Random(5)
    table = spx.fr_bytes([rs.randrange(R) for _ in range(1 << VIEW_NV)])
    point = spx.fr_bytes([rs.randrange(R) for _ in range(VIEW_NV)])
    if spx.MLPolyCommit.commit(view, table) != spx.MLPolyCommit.commit(native, table):
        fails.append("commitment differs")
    if spx.MLPolyCommit.open(view, table, point) != spx.MLPolyCommit.open(native, table, point):
        fails.append("opening differs")
    if view.check_structure() != (0, None, 1):
        fails.append("structure check")
    print("FAILED: %s" % fails if fails else "all equal", flush=True)
    return 1 if fails else 0


if __name__ == "__main__":
    sys.exit(main())
