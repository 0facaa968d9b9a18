"""The GPU index builder (spx_ctx_set_index_build, index_kernels.hip) against the host builder and against
the Python restatement of the layouts (index_cases.py): every exported device array byte for byte, the
host-side checks and their messages, proofs from a GPU-built index, and the setter."""
import json
import os
import random
import subprocess
import sys
import threading

import pytest

import index_cases as ic

pytestmark = pytest.mark.gpu

R = ic.R
RINV = pow(1 << 256, -1, R)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def bctx(spx):
    """a context of this module's own: the tests switch its builder (and its communicator)"""
    return spx.Context(0)


def _csrs(spx, mats):
    return [spx.Csr(M.n, M.row_ptr, M.col, M.val) for M in mats]


def _index(spx, c, mats, mode):
    c.set_index_build(mode)
    try:
        return spx.MLArgumentForR1CS.index(c, *_csrs(spx, mats))
    finally:
        c.set_index_build(0)


def _from_mont(b):
    return [int.from_bytes(b[i : i + 32], "little") * RINV % R for i in range(0, len(b), 32)]


def _check_layout(spx, c, oc, name, rank, G):
    rows, mats = ic.case(oc, name)
    ref = ic.reference(rows, rank, G)
    host, gpu = _index(spx, c, mats, 0), _index(spx, c, mats, 1)
    for part, pname in enumerate(spx.INDEX_PARTS):
        h, g = host.export(part), gpu.export(part)
        assert h == g, "%s (rank %d of %d): %s differs between the builders" % (name, rank, G, pname)
        want = ref[pname[4:]]
        if pname[4:] in ic.VALUE_PARTS:
            assert len(g) == 32 * len(want) and _from_mont(g) == want, (name, rank, G, pname)
        else:
            assert g == want, (name, rank, G, pname)
    hs, gs = host.stats(), gpu.stats()
    assert hs[0] == 0 and gs[0] == 1
    assert hs[1:6] == gs[1:6] == [ref["_stats"][k] for k in ("sliced", "row_entries", "col_entries", "long_rows", "long_cols")]


@pytest.mark.parametrize("name", list(ic.CASES))
def test_layouts_equal(spx, bctx, oc, name):
    _check_layout(spx, bctx, oc, name, 0, 1)


@pytest.fixture(scope="module")
def sctx(spx):
    return spx.Context(0)


@pytest.mark.parametrize("name,G", ic.SHARDED)
def test_layouts_equal_sharded(spx, sctx, oc, name, G):
    group = spx.CommGroup(G)  # index_build reads only the rank and the size: the ranks build one after another
    for rank in range(G):
        sctx.set_comm_group(group, rank)
        _check_layout(spx, sctx, oc, name, rank, G)


# ---------------------------------------------------------------- errors: the host checks run first
def _error_of(spx, c, csrs, mode):
    c.set_index_build(mode)
    try:
        with pytest.raises(spx.SpartanError) as e:
            spx.MLArgumentForR1CS.index(c, *csrs)
        return type(e.value), str(e.value)
    finally:
        c.set_index_build(0)


def test_errors_equal_the_host_builders(spx, bctx, oc):
    rows, _ = ic.case(oc, "dups6")
    n = len(rows[0])

    def csrs(edit):
        ms = [spx.Csr.from_rows(r) for r in rows]
        edit(ms)
        return ms

    def noncanonical(ms):
        raw = bytearray(ms[1].val.raw)
        raw[32 * 7 : 32 * 8] = (R + 5).to_bytes(32, "little")
        ms[1] = spx.Csr(n, list(ms[1].row_ptr), list(ms[1].col), bytes(raw))

    def column_out_of_range(ms):
        ms[2].col[3] = n

    def decreasing(ms):
        ms[0].row_ptr[10] = ms[0].row_ptr[9] - 1

    def size_mismatch(ms):
        ms[1] = spx.Csr.from_rows(rows[1][: n // 2])

    want = {noncanonical: (spx.SerializationError, "non-canonical field element in matrix"),
            column_out_of_range: (spx.InvalidArgument, "sparse index out of bound"),
            decreasing: (spx.InvalidArgument, "malformed row_ptr"),
            size_mismatch: (spx.InvalidArgument, "matrix size is inconsistent with number of constraints")}
    for edit, (cls, msg) in want.items():
        host, gpu = _error_of(spx, bctx, csrs(edit), 0), _error_of(spx, bctx, csrs(edit), 1)
        assert host == gpu == (cls, msg), edit.__name__


# ---------------------------------------------------------------- end to end
def _instance(oc, kind, log_n):
    inst = oc.Instance(kind, log_n, 3, 8100 + log_n)
    return inst, inst.mats


def _dup_instance(oc):
    inst = oc.Instance(0, 6, 3, 8200)
    rs = random.Random(82)
    mats = []
    for M in inst.mats:
        rws = M.to_rows()
        for x in range(0, len(rws), 3):
            if rws[x]:
                rws[x] = rws[x] + [(rs.randrange(R), rws[x][0][1]), (rs.randrange(R), rws[x][-1][1])]
        mats.append(oc.CsrMatrix.from_rows(rws))
    return inst, mats


@pytest.mark.parametrize("which", ["0-6", "1-10", "0-12", "dups"])
def test_proofs_equal(spx, bctx, oc, which):
    inst, mats = _dup_instance(oc) if which == "dups" else _instance(oc, *map(int, which.split("-")))
    ppc = oc.PP.keygen(inst.log_n, 8300 + inst.log_n)
    pp = spx.PublicParameter.load(bctx, ppc.serialize())
    want = oc.prove(mats, inst.v_bytes, inst.w_bytes, ppc, 0, 0)
    host, gpu = _index(spx, bctx, mats, 0), _index(spx, bctx, mats, 1)
    assert gpu.stats()[0] == 1
    for cached in (False, True):  # cached: the transcript state the builder absorbed beside its kernels
        got = spx.MLArgumentForR1CS.prove(gpu, inst.v_bytes, inst.w_bytes, pp, cached=cached)
        assert got == spx.MLArgumentForR1CS.prove(host, inst.v_bytes, inst.w_bytes, pp, cached=cached)
        assert got == want
    if which == "dups":
        return  # the instance's witness does not satisfy the edited matrices
    vp = pp.derive_vp()
    assert spx.MLArgumentForR1CS.verify(gpu, inst.v_bytes, want, vp) is True
    wit = spx.Witness(bctx, inst.v_bytes, inst.w_bytes)
    assert spx.MLArgumentForR1CS.check_witness(gpu, wit)[0] == 0
    bad = bytearray(want)
    bad[len(bad) // 2] ^= 1
    with pytest.raises(spx.SpartanError):
        spx.MLArgumentForR1CS.verify(gpu, inst.v_bytes, bytes(bad), vp)
    if which == "0-6":
        wits = [spx.Witness(bctx, inst.v_bytes, inst.w_bytes) for _ in range(4)]
        assert spx.MLArgumentForR1CS.prove_many([bctx], gpu, wits, pp) == [want] * 4


def test_sharded_proof_with_mixed_builders(spx, oc):
    inst, mats = _instance(oc, 0, 8)
    ppb = oc.PP.keygen(8, 8400).serialize()
    want = oc.prove(mats, inst.v_bytes, inst.w_bytes, oc.PP.load(ppb), 0, 0)
    group = spx.CommGroup(2)
    out, built, errs = [None, None], [None, None], []

    def run(r):
        try:
            c = spx.Context(0)
            c.set_comm_group(group, r)
            c.set_index_build(1 if r == 0 else 0)
            pp = spx.PublicParameter.load(c, ppb)
            pk = spx.MLArgumentForR1CS.index(c, *_csrs(spx, mats))
            built[r] = pk.stats()[0]
            out[r] = spx.MLArgumentForR1CS.prove(pk, inst.v_bytes, inst.w_bytes, pp)
        except Exception as e:  # surfaced below
            errs.append(repr(e))

    ths = [threading.Thread(target=run, args=(r,)) for r in range(2)]
    for t in ths:
        t.start()
    for t in ths:
        t.join(timeout=300)
    assert not errs, errs
    assert built == [1, 0] and out == [want, want]


# ---------------------------------------------------------------- the setter
def test_setter_and_defaults(spx, oc):
    c = spx.Context(0)
    with pytest.raises(spx.InvalidArgument):
        c.set_index_build(2)
    _, mats = ic.case(oc, "n4")
    assert spx.MLArgumentForR1CS.index(c, *_csrs(spx, mats)).stats()[0] == 0  # no call: the host builder
    c.set_index_build(1)
    assert spx.MLArgumentForR1CS.index(c, *_csrs(spx, mats)).stats()[0] == 1
    c.set_index_build(-1)
    assert spx.MLArgumentForR1CS.index(c, *_csrs(spx, mats)).stats()[0] == (os.environ.get("SPX_INDEX_BUILD") == "gpu")


def test_process_default_from_environment():
    env = dict(os.environ, SPX_INDEX_BUILD="gpu")
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "index_env_child.py")], env=env, capture_output=True,
                       text=True, timeout=120)
    assert p.returncode == 0, p.stderr[-2000:]
    assert json.loads(p.stdout.strip().splitlines()[-1]) == {"default": 1, "host": 0, "default_again": 1}
