"""spx_pp_view ("Public-parameter structure and views"): the parameter of nv' variables
inside one of nv variables is its levels nv - nv' .. nv - 1, so a view borrows the parent's raw levels and
G2 opening tables (with the parent's window bits) and builds only its own G1 commitment table. Whatever
takes an spx_pp must not see the difference: serialized bytes, derived and trapdoor verifier parameters,
commitments, openings and whole proofs are compared byte for byte with the oracle's under the sliced
parameter, or with the same bytes loaded natively."""
import ctypes
import os
import random
import subprocess
import sys
import threading

import pytest

import pp_structure_cases as cases
import pp_view_wide_check as wc
import spartan

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
R = spartan.R
PARENT_NV, PARENT_SEED = 12, 0x71E3


def _csrs(spx, inst):
    return [spx.Csr(M.n, M.row_ptr, M.col, M.val) for M in inst.mats]


def _prove(spx, ctx, inst, pp, **kw):
    pk = spx.MLArgumentForR1CS.index(ctx, *_csrs(spx, inst))
    return spx.MLArgumentForR1CS.prove(pk, inst.v_bytes, inst.w_bytes, pp, **kw)


def _free(spx, pp):
    assert spx.lib().spx_pp_free(pp.h) == 0
    pp.h = None


# ------------------------------------------------------------------ oracle parent
@pytest.mark.parametrize("nv", [4, 2])
def test_view_of_the_degenerate_parameter_equals_the_oracle_slice(spx, ctx, oc, nv):
    fx = cases.degenerate()
    k = fx.nv - nv
    want_pp, want_vp = cases.sliced(fx.pp, fx.vp, k)
    want_bytes = want_pp.serialize_uncompressed()
    parent = spx.PublicParameter.load(ctx, fx.bytes)
    view = parent.view(nv)
    assert view.serialize_uncompressed() == want_bytes
    assert view.derive_vp() == want_vp.serialize_uncompressed()
    assert view.check_structure() == (0, None, 1) and view.check_subgroup() == (0, None)
    ppc = oc.PP.load(want_bytes)
    for mode in ("fs", "injected"):
        inst = oc.Instance(0, nv, 1, 0x5EED0000 + nv)
        want = oc.prove(inst.mats, inst.v_bytes, inst.w_bytes, ppc, 1 if mode == "injected" else 0, 66)
        assert _prove(spx, ctx, inst, view, mode=mode, seed=66) == want, mode


# ------------------------------------------------------------------ generated parent
@pytest.fixture(scope="module")
def parent(spx, ctx):
    return spx.MLProofForR1CS.setup(ctx, PARENT_NV, PARENT_SEED)


@pytest.fixture(scope="module")
def parent_vp(spx, parent):
    return spx.verifier_parameter(parent)


def _masks(vp, nv):
    """g, h and the last nv entries of g_mask_random, as the verifier parameter of nv variables"""
    total = int.from_bytes(vp[:8], "little")
    head = vp[8:8 + 96 + 192]
    masks = vp[8 + 96 + 192 + 8:]
    return nv.to_bytes(8, "little") + head + nv.to_bytes(8, "little") + masks[96 * (total - nv):]


@pytest.mark.parametrize("nv", [12, 11, 8])
def test_view_of_a_generated_parameter_equals_the_native_load(spx, ctx, oc, parent, parent_vp, nv):
    view = parent.view(nv)
    vb = view.serialize_uncompressed()
    native = spx.PublicParameter.load(ctx, vb)
    assert native.serialize_uncompressed() == vb
    if nv == PARENT_NV:
        assert vb == parent.serialize_uncompressed()
    inst = oc.Instance(0, nv, 3, 0x71E30000 + nv)
    proof = _prove(spx, ctx, inst, view)
    assert proof == _prove(spx, ctx, inst, native)
    vp = _masks(parent_vp, nv)
    assert spx.verifier_parameter(view) == vp and view.derive_vp() == vp and native.derive_vp() == vp
    pk = spx.MLArgumentForR1CS.index(ctx, *_csrs(spx, inst))
    assert spx.MLArgumentForR1CS.verify(pk, inst.v_bytes, proof, vp) is True
    rs = random.Random(nv)
    table = spx.fr_bytes([rs.randrange(R) for _ in range(1 << nv)])
    point = spx.fr_bytes([rs.randrange(R) for _ in range(nv)])
    com = spx.MLPolyCommit.commit(view, table)
    assert com == spx.MLPolyCommit.commit(native, table)
    value, opening = spx.MLPolyCommit.open(view, table, point)
    assert (value, opening) == spx.MLPolyCommit.open(native, table, point)
    assert spx.MLPolyCommit.verify(vp, com, point, value, opening) is True
    assert view.check_structure() == (0, None, 1)
    assert view.check_subgroup() == (0, None)
    # the shared levels keep the parent's window plan; the commitment table is the view's own size's
    k = PARENT_NV - nv
    assert [view.window_plan(j) for j in range(nv)] == [parent.window_plan(k + j) for j in range(nv)]
    assert view.window_plan(-1) == native.window_plan(-1)


def test_view_of_a_view_is_the_view(spx, parent):
    direct = parent.view(8)
    nested = parent.view(11).view(8)
    assert nested.serialize_uncompressed() == direct.serialize_uncompressed()
    assert nested.mem_info()[2] == parent.mem_info()[2]  # both count handles on the root's storage


def test_round_level_session_and_prove_many_take_a_view(spx, ctx, oc, parent):
    """the round-level prover (spx_prover_*) and spx_prove_many with a view: the same messages and proofs as
    with the native load"""
    from test_gpu_interactive import _drive

    nv, log_v, seed = 8, 2, 0x1A7E
    view = parent.view(nv)
    native = spx.PublicParameter.load(ctx, view.serialize_uncompressed())
    inst = oc.Instance(0, nv, log_v, 0x71E38888)
    pk = spx.MLArgumentForR1CS.index(ctx, *_csrs(spx, inst))
    msgs, pm6 = _drive(spx, pk, inst, view, seed, nv, log_v)
    assert (msgs, pm6) == _drive(spx, pk, inst, native, seed, nv, log_v)
    L = nv.to_bytes(8, "little")
    proof = b"".join(msgs[:3]) + L + b"".join(msgs[3:3 + nv]) + b"".join(msgs[3 + nv:5 + nv]) + L + b"".join(msgs[5 + nv:]) + pm6
    assert proof == spx.MLArgumentForR1CS.prove(pk, inst.v_bytes, inst.w_bytes, native, mode="injected", seed=seed)
    wits = [spx.Witness(ctx, inst.v_bytes, inst.w_bytes) for _ in range(3)]
    ctxs = [spx.Context(0) for _ in range(2)]
    assert spx.MLArgumentForR1CS.prove_many(ctxs, pk, wits, view) == spx.MLArgumentForR1CS.prove_many(ctxs, pk, wits, native)


# ------------------------------------------------------------------ wide windows
def test_view_shares_wide_levels():
    """SPX_MSM_WIDE_MIN_LOG=8 in a child process (the setting is read when a parameter is preprocessed):
    levels 0 .. 3 of the nv = 12 parent carry 17-bit windows, so levels 0 and 1 of its nv = 10 view, the
    parent's levels 2 and 3, do; the view reports the parent's plan and proves the native load's bytes"""
    e = dict(os.environ)
    for k in ("SPX_MSM_WIDE_MIN_LOG", "SPX_SORT_FORM", "SPX_MSM_CAP_SCALE"):
        e.pop(k, None)
    e["SPX_MSM_WIDE_MIN_LOG"] = "8"
    r = subprocess.run([sys.executable, "-u", os.path.join(HERE, "pp_view_wide_check.py")], env=e, timeout=120,
                       capture_output=True, text=True)
    print(r.stdout)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "all equal" in r.stdout


def test_wide_check_plan_model():
    assert wc.level_bits(12, 8) == [17, 17, 17, 17, 5, 4, 3, 3, 3, 3, 3, 3]
    assert wc.level_bits(10, 8) == [17, 17, 5, 4, 3, 3, 3, 3, 3, 3]


# ------------------------------------------------------------------ ownership
def test_ownership_and_lifetime(spx, ctx, oc):
    root = spx.MLProofForR1CS.setup(ctx, PARENT_NV, PARENT_SEED + 1)
    own = root.mem_info()
    assert own[0] > 0 and own[1:] == [0, 1]
    view = root.view(8)
    native = spx.PublicParameter.load(ctx, view.serialize_uncompressed())
    assert root.mem_info() == [own[0], 0, 2]
    v = view.mem_info()
    assert v[2] == 2 and v[1] > 0 and 0 < v[0] < native.mem_info()[0]
    assert v[0] + v[1] <= native.mem_info()[0]  # the borrowed G2 tables are no larger than a native load's
    whole = root.view(PARENT_NV)
    assert whole.mem_info()[0] == 0 and whole.mem_info()[1] == own[0] and whole.mem_info()[2] == 3
    inst = oc.Instance(0, 8, 3, 0x0E0E)
    want = _prove(spx, ctx, inst, native)
    assert _prove(spx, ctx, inst, view) == want
    _free(spx, whole)
    _free(spx, root)
    assert view.mem_info() == [v[0], v[1], 1]
    assert _prove(spx, ctx, inst, view) == want
    assert view.serialize_uncompressed() == native.serialize_uncompressed()


# ------------------------------------------------------------------ sharded contexts
def test_view_on_two_virtual_ranks(spx, ctx, oc):
    log_n, G = 8, 2
    inst = oc.Instance(0, log_n, 3, 0x5A4D)
    parent = spx.MLProofForR1CS.setup(ctx, 10, PARENT_SEED + 2)
    ppb = parent.serialize_uncompressed()
    want = _prove(spx, ctx, inst, parent.view(log_n))
    group = spx.CommGroup(G)
    out, errs = [None] * G, []

    def run(r):
        try:
            c = spx.Context(0)
            c.set_comm_group(group, r)
            view = spx.PublicParameter.load(c, ppb).view(log_n)
            out[r] = _prove(spx, c, inst, view)
        except Exception as e:  # surfaced below
            errs.append(repr(e))

    ths = [threading.Thread(target=run, args=(r,)) for r in range(G)]
    for t in ths:
        t.start()
    for t in ths:
        t.join(timeout=300)
    assert not errs, errs
    assert out == [want] * G


# ------------------------------------------------------------------ errors
def test_view_errors(spx, ctx, oc, parent):
    INVALID = 1
    for nv in (0, PARENT_NV + 1, -1):
        with pytest.raises(spx.InvalidArgument, match="nv out of range"):
            parent.view(nv)
    h = ctypes.c_void_p()
    assert spx.lib().spx_pp_view(ctx.h, None, 4, ctypes.byref(h)) == INVALID
    assert spx.lib().spx_pp_view(None, parent.h, 4, ctypes.byref(h)) == INVALID
    out = (ctypes.c_uint64 * 3)()
    assert spx.lib().spx_pp_mem_info(None, out) == INVALID
    inst = oc.Instance(0, 9, 3, 0x0909)
    with pytest.raises(spx.InvalidArgument, match="public parameter nv != log_n"):
        _prove(spx, ctx, inst, parent.view(8))
