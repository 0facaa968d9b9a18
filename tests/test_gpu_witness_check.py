"""The witness check (spx_ctx_set_witness_check, spx_witness_check; csrc/mle_kernels.hip k_r1cs_check,
DESIGN §6b) against the oracle: for every case the reference is oracle_c.sum_over_y on the same three
matrices and z, then Python integers mod r, which gives the set of rows with Az Bz != Cz, its size, its
minimum and the three values there. Each test first asserts that the reference's set is what the case
intends, so no case passes vacuously. Violations are placed at chosen rows by adding 1 to one coefficient
of C in each target row (the matrix is perturbed, not the witness); the reference is computed on the same
perturbed matrices.

Sizes: the check kernel runs one block of 256 lanes up to 2^8 rows, several blocks with one row per lane
up to 2^11, and from 2^12 rows on four rows per lane (the grid-stride loop); 2^2 is less than a wave and
2^6 exactly one.

The reference-shaped generator (kind 1) needs four public inputs and a private variable, so its smallest
instance is 2^3: the kind-1 cases run at 2^3 where the other kinds run at 2^2."""
import json
import os
import subprocess
import sys
import threading

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
R = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001
RAGGED = 3 | (2 << 16)


def _ints(b):
    return [int.from_bytes(b[32 * i : 32 * i + 32], "little") for i in range(len(b) // 32)]


def _log_v(log_n):
    return min(3, log_n - 1)


_INST = {}


def _inst(oc, kind, log_n):
    """one generated instance per (kind, size), shared by the tests and left unchanged"""
    key = (kind, log_n)
    if key not in _INST:
        param = RAGGED if kind == 2 else (0xB0B0 if kind == 3 else 0)
        _INST[key] = oc.Instance(kind, log_n, _log_v(log_n), 0x5EED0000 + log_n, param)
    return _INST[key]


def _reference(oc, mats, z_bytes):
    """(violated rows ascending, Az, Bz, Cz) by the oracle's sum_over_y and Python integers"""
    az, bz, cz = (_ints(oc.sum_over_y(M, z_bytes)) for M in mats)
    return [x for x in range(len(az)) if az[x] * bz[x] % R != cz[x]], az, bz, cz


def _expected(ref):
    bad, az, bz, cz = ref
    if not bad:
        return 0, None, (0, 0, 0)
    x = bad[0]
    return len(bad), x, (az[x], bz[x], cz[x])


def _perturbed(oc, inst, rows):
    """inst's matrices with 1 added to the first coefficient of C in each of `rows`"""
    crows = inst.mats[2].to_rows()
    for x in rows:
        coeff, col = crows[x][0]
        crows[x][0] = ((coeff + 1) % R, col)
    return [inst.mats[0], inst.mats[1], oc.CsrMatrix.from_rows(crows)]


def _index(spx, ctx, mats):
    return spx.MLArgumentForR1CS.index(ctx, *[spx.Csr(M.n, M.row_ptr, M.col, M.val) for M in mats])


def _check(spx, ctx, mats, inst):
    pk = _index(spx, ctx, mats)
    return spx.MLArgumentForR1CS.check_witness(pk, spx.Witness(ctx, inst.v_bytes, inst.w_bytes))


@pytest.fixture(scope="module")
def cctx(spx):
    """a context with the witness check on"""
    c = spx.Context(0)
    c.set_witness_check(1)
    return c


# ---------------------------------------------------------------- stand-alone check
@pytest.mark.parametrize("kind,log_n", [(k, n) for k in (0, 3) for n in (2, 6, 9, 12)] + [(1, n) for n in (3, 6, 9, 12)])
def test_standalone_satisfiable(spx, ctx, oc, kind, log_n):
    inst = _inst(oc, kind, log_n)
    ref = _reference(oc, inst.mats, inst.z_bytes)
    assert ref[0] == [], "the generated instance should be satisfiable"
    before = ctx.witness_check_stats()
    assert _check(spx, ctx, inst.mats, inst) == (0, None, (0, 0, 0))
    after = ctx.witness_check_stats()
    assert [a - b for a, b in zip(after, before)] == [1, 0, 1, 1 << log_n]
    # the C ABI's status: SPX_OK
    pk = _index(spx, ctx, inst.mats)
    wit = spx.Witness(ctx, inst.v_bytes, inst.w_bytes)
    assert spx.lib().spx_witness_check(ctx.h, pk.h, wit.h, None, None, None) == 0


def _row_sets(n):
    return {
        "first": [0],
        "last": [n - 1],
        "two_waves": [63, 64],
        "one_wave": [5, 40],
        "last_block": [n - 100],  # 2^9: the second of two blocks; 2^12: block 3 of 4 (rows 768..1023 mod 1024)
        "every": list(range(n)),
    }


@pytest.mark.parametrize("log_n", [9, 12])
@pytest.mark.parametrize("which", ["first", "last", "two_waves", "one_wave", "last_block", "every"])
def test_standalone_chosen_rows(spx, ctx, oc, log_n, which):
    inst = _inst(oc, 0, log_n)  # single-entry rows (the sliced SpMV), every coefficient's variable non-zero
    rows = _row_sets(1 << log_n)[which]
    mats = _perturbed(oc, inst, rows)
    ref = _reference(oc, mats, inst.z_bytes)
    assert ref[0] == rows, "the perturbation should violate exactly the chosen rows"
    assert _check(spx, ctx, mats, inst) == _expected(ref)


@pytest.mark.parametrize("log_n", [2, 6])
def test_standalone_last_row_small(spx, ctx, oc, log_n):
    """n - 1 violated at n = 4 (less than one wave) and n = 64 (exactly one wave)"""
    inst = _inst(oc, 0, log_n)
    rows = [(1 << log_n) - 1]
    mats = _perturbed(oc, inst, rows)
    ref = _reference(oc, mats, inst.z_bytes)
    assert ref[0] == rows
    assert _check(spx, ctx, mats, inst) == _expected(ref)


@pytest.mark.parametrize("rows", [[0], [63, 64], [5, 40]])
def test_standalone_chosen_rows_csr_form(spx, ctx, oc, rows):
    """the same through the CSR SpMV (kind 1: rows of several entries and a long one)"""
    inst = _inst(oc, 1, 9)
    mats = _perturbed(oc, inst, rows)
    ref = _reference(oc, mats, inst.z_bytes)
    assert ref[0] == rows
    assert _check(spx, ctx, mats, inst) == _expected(ref)


def test_standalone_status_and_stats_on_rejection(spx, ctx, oc):
    inst = _inst(oc, 0, 9)
    mats = _perturbed(oc, inst, [5, 40])
    ref = _reference(oc, mats, inst.z_bytes)
    assert ref[0] == [5, 40]
    pk = _index(spx, ctx, mats)
    wit = spx.Witness(ctx, inst.v_bytes, inst.w_bytes)
    before = ctx.witness_check_stats()
    assert spx.lib().spx_witness_check(ctx.h, pk.h, wit.h, None, None, None) == 3  # SPX_WRONG_WITNESS
    assert b"constraint 5 is not satisfied" in spx.lib().spx_last_error()
    assert b"(2 of 512 constraints fail)" in spx.lib().spx_last_error()
    after = ctx.witness_check_stats()
    assert [a - b for a, b in zip(after, before)] == [1, 1, 1, 512]


def test_ragged_unsatisfiable(spx, ctx, oc):
    """kind 2: random ragged rows, unsatisfiable by construction; count and first row are the reference's"""
    inst = _inst(oc, 2, 8)
    ref = _reference(oc, inst.mats, inst.z_bytes)
    assert ref[0], "a random ragged instance should violate constraints"
    got = _check(spx, ctx, inst.mats, inst)
    assert got == _expected(ref)


@pytest.mark.parametrize("off", [0, 1])
def test_all_zero_rows(spx, ctx, oc, off):
    """make_square's padding rows are all zero (0 * 0 = 0: satisfied); x * x = y with x = r - 1 is
    satisfied by y = 1, and with y off by one exactly that row is reported"""
    cs = spx.ConstraintSystem()
    cs.new_input(7)
    x = cs.new_witness(R - 1)
    y = cs.new_witness(1 + off)
    cs.enforce([(1, x)], [(1, x)], [(1, y)])
    for _ in range(2):
        cs.new_input(0)  # |v| = 4
    for _ in range(2):
        cs.new_witness(0)  # 8 variables
    cs.make_square(8)
    assert cs.is_satisfied() == (off == 0)
    a, b, c, v, w = cs.to_matrices()
    mats = [oc.CsrMatrix(m.n, [m.row_ptr[i] for i in range(m.n + 1)], [m.col[i] for i in range(m.row_ptr[m.n])],
                         m.val.raw[: 32 * m.row_ptr[m.n]]) for m in (a, b, c)]
    ref = _reference(oc, mats, v + w)
    assert ref[0] == ([0] if off else [])
    pk = spx.MLArgumentForR1CS.index(ctx, a, b, c)
    got = spx.MLArgumentForR1CS.check_witness(pk, spx.Witness(ctx, v, w))
    assert got == _expected(ref)
    if off:
        assert got == (1, 0, (R - 1, R - 1, 2))


# ---------------------------------------------------------------- prove with the check on
@pytest.mark.parametrize("log_n", [6, 10])
@pytest.mark.parametrize("mode", ["fs", "injected"])
@pytest.mark.parametrize("stub", [False, True])
def test_prove_checked_satisfiable_same_bytes(spx, ctx, cctx, oc, log_n, mode, stub):
    inst = _inst(oc, 0, log_n)
    assert _reference(oc, inst.mats, inst.z_bytes)[0] == []
    ppc = None if stub else oc.PP.keygen(log_n, 99)
    want = oc.prove(inst.mats, inst.v_bytes, inst.w_bytes, ppc, 1 if mode == "injected" else 0, 5, commitment_stub=stub)
    got = {}
    for name, c in (("off", ctx), ("on", cctx)):
        pp = None if stub else spx.PublicParameter.load(c, ppc.serialize())
        pk = _index(spx, c, inst.mats)
        before = c.witness_check_stats()
        got[name] = spx.MLArgumentForR1CS.prove(pk, inst.v_bytes, inst.w_bytes, pp, mode=mode, seed=5,
                                                commitment_stub=stub)
        moved = [a - b for a, b in zip(c.witness_check_stats(), before)]
        assert moved == ([1, 0, 1, 1 << log_n] if name == "on" else [0, 0, 0, 0])
    assert got["on"] == got["off"] == want


@pytest.mark.parametrize("log_n", [6, 10])
@pytest.mark.parametrize("stub", [False, True])
def test_prove_checked_violated_then_clean(spx, cctx, oc, log_n, stub):
    inst = _inst(oc, 0, log_n)
    rows = [5, 40]
    mats = _perturbed(oc, inst, rows)
    ref = _reference(oc, mats, inst.z_bytes)
    assert ref[0] == rows
    ppc = None if stub else oc.PP.keygen(log_n, 99)
    pp = None if stub else spx.PublicParameter.load(cctx, ppc.serialize())
    pk_bad = _index(spx, cctx, mats)
    pk_good = _index(spx, cctx, inst.mats)
    before = cctx.witness_check_stats()
    with pytest.raises(spx.WrongWitness) as e:
        spx.MLArgumentForR1CS.prove(pk_bad, inst.v_bytes, inst.w_bytes, pp, commitment_stub=stub)
    assert "constraint %d is not satisfied" % ref[0][0] in str(e.value)
    assert "(%d of %d constraints fail)" % (len(ref[0]), 1 << log_n) in str(e.value)
    # the very next prove of a good witness on the same context: the context was left clean
    got = spx.MLArgumentForR1CS.prove(pk_good, inst.v_bytes, inst.w_bytes, pp, commitment_stub=stub)
    assert got == oc.prove(inst.mats, inst.v_bytes, inst.w_bytes, ppc, 0, 0, commitment_stub=stub)
    moved = [a - b for a, b in zip(cctx.witness_check_stats(), before)]
    assert moved == [2, 1, 2, 2 << log_n]


def test_prove_len_untouched_on_rejection(spx, cctx, oc):
    """the C ABI: SPX_WRONG_WITNESS and *len left as it was, for spx_prove and spx_prove_witness"""
    import ctypes

    inst = _inst(oc, 0, 6)
    mats = _perturbed(oc, inst, [0])
    assert _reference(oc, mats, inst.z_bytes)[0] == [0]
    pk = _index(spx, cctx, mats)
    L = spx.lib()
    cap = L.spx_proof_size(6, 0)
    out = ctypes.create_string_buffer(cap)
    o = spx._opts("fs", 0, False, True)
    n = ctypes.c_size_t(12345)
    v, w = inst.v_bytes, inst.w_bytes
    assert L.spx_prove(cctx.h, pk.h, v, len(v) // 32, w, len(w) // 32, None, ctypes.byref(o), out, cap, ctypes.byref(n)) == 3
    assert n.value == 12345
    wit = spx.Witness(cctx, v, w)
    assert L.spx_prove_witness(cctx.h, pk.h, wit.h, None, ctypes.byref(o), out, cap, ctypes.byref(n)) == 3
    assert n.value == 12345


@pytest.mark.parametrize("stub", [False, True])
def test_check_off_proves_violated_witness(spx, ctx, oc, stub):
    """off (the default): a violated witness proves to the oracle's bytes for it, and no check kernel runs"""
    log_n = 6
    inst = _inst(oc, 0, log_n)
    mats = _perturbed(oc, inst, [5, 40])
    assert _reference(oc, mats, inst.z_bytes)[0] == [5, 40]
    ppc = None if stub else oc.PP.keygen(log_n, 99)
    pp = None if stub else spx.PublicParameter.load(ctx, ppc.serialize())
    pk = _index(spx, ctx, mats)
    before = ctx.witness_check_stats()
    got = spx.MLArgumentForR1CS.prove(pk, inst.v_bytes, inst.w_bytes, pp, commitment_stub=stub)
    assert got == oc.prove(mats, inst.v_bytes, inst.w_bytes, ppc, 0, 0, commitment_stub=stub)
    assert ctx.witness_check_stats()[2] == before[2]
    assert ctx.witness_check_stats() == before


def test_mode_setter(spx):
    c = spx.Context(0)
    for bad in (-2, 2):
        with pytest.raises(spx.InvalidArgument):
            c.set_witness_check(bad)
    for ok in (1, 0, -1):
        c.set_witness_check(ok)


@pytest.mark.parametrize("env,default", [("1", "on"), (None, "off"), ("0", "off")])
def test_process_default_in_a_fresh_child(env, default):
    """SPX_WITNESS_CHECK is read once per process: a child per value (tests/witness_check_env_child.py)"""
    e = dict(os.environ)
    e.pop("SPX_WITNESS_CHECK", None)
    if env is not None:
        e["SPX_WITNESS_CHECK"] = env
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "witness_check_env_child.py")], env=e,
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    on, off = ["WrongWitness", [1, 1, 1, 64]], ["ok", [0, 0, 0, 0]]
    assert out["on"] == on and out["off"] == off
    assert out["default"] == out["default_again"] == (on if default == "on" else off)


# ---------------------------------------------------------------- prove_many, one at a time and in lockstep
def _many_case(spx, oc, ctx, log_n, nwit=7, corrupt=(2, 5)):
    """a kind-3 index with nwit witnesses (the helper pattern of tests/test_gpu_group.py), those in
    `corrupt` with one private value changed; the reference's verdict for each"""
    sys.path.insert(0, ROOT)
    import bench

    log_v = 3
    seed = 0x5EED0000 + log_n
    syn, mats, zs, nnz = bench.synth_instance(spx, 3, log_n, log_v, seed, nwit, 0xB0B0)
    pk = spx.IndexPK(ctx, bench.index_from_c(spx, ctx, mats), log_n)
    zs = list(zs)
    for i in corrupt:
        z = bytearray(zs[i])
        at = 32 * ((1 << log_n) - 1)
        z[at : at + 32] = ((int.from_bytes(z[at : at + 32], "little") + 1) % R).to_bytes(32, "little")
        zs[i] = bytes(z)
    omats = oc.Instance(3, log_n, log_v, seed, 0xB0B0).mats
    refs = [_reference(oc, omats, z) for z in zs]
    for i in range(nwit):
        assert bool(refs[i][0]) == (i in corrupt), "witness %d: the reference disagrees with the case" % i
    wits = [spx.Witness(ctx, z[: 32 << log_v], z[32 << log_v :]) for z in zs]
    return syn, pk, wits, refs


def _assert_many(spx, pk, wits, refs, ctxs, corrupt, **kw):
    want = [spx.MLArgumentForR1CS.prove_witness(pk, w, kw.get("pp"), commitment_stub=kw["stub"]) for w in wits]
    before = [c.witness_check_stats() for c in ctxs]
    with pytest.raises(spx.WrongWitness) as e:
        spx.MLArgumentForR1CS.prove_many(ctxs, pk, wits, kw.get("pp"), commitment_stub=kw["stub"])
    proofs = e.value.proofs
    assert [i for i, p in enumerate(proofs) if p is None] == list(corrupt)
    for i, p in enumerate(proofs):
        if i not in corrupt:
            assert p == want[i], "proof %d differs from its one-at-a-time proof" % i
    low = corrupt[0]
    assert "proof %d:" % low in str(e.value)
    assert "constraint %d is not satisfied" % refs[low][0][0] in str(e.value)
    moved = [sum(c.witness_check_stats()[k] for c in ctxs) - sum(b[k] for b in before) for k in range(4)]
    assert moved[0] == len(wits) and moved[1] == len(corrupt)
    return moved


def test_prove_many_rejects_and_goes_on(spx, ctx, oc):
    log_n = 6
    syn, pk, wits, refs = _many_case(spx, oc, ctx, log_n)
    pp = spx.MLProofForR1CS.setup(ctx, log_n, 77)
    ctxs = [spx.Context(0) for _ in range(2)]
    for c in ctxs:
        c.set_witness_check(1)
    moved = _assert_many(spx, pk, wits, refs, ctxs, (2, 5), pp=pp, stub=False)
    assert moved[2] == 7  # one launch per proof


@pytest.mark.parametrize("log_n", [6, 8])
def test_lockstep_group_rejects_and_goes_on(spx, ctx, oc, log_n):
    """stubbed, groups of 4 on two contexts: the blockIdx.y form of the check and the discarded slot"""
    syn, pk, wits, refs = _many_case(spx, oc, ctx, log_n)
    ctxs = [spx.Context(0) for _ in range(2)]
    for c in ctxs:
        c.set_witness_check(1)
        c.set_group(4)
    moved = _assert_many(spx, pk, wits, refs, ctxs, (2, 5), stub=True)
    assert moved[2] == 2  # context 0: proofs 0, 2, 4, 6 in one group; context 1: 1, 3, 5: one launch each
    # and with the check off the same call proves all seven, as before
    for c in ctxs:
        c.set_witness_check(0)
    got = spx.MLArgumentForR1CS.prove_many(ctxs, pk, wits, None, commitment_stub=True)
    assert got == [spx.MLArgumentForR1CS.prove_witness(pk, w, None, commitment_stub=True) for w in wits]


# ---------------------------------------------------------------- round-level session
def test_interactive_session_rejected_then_new_session(spx, oc):
    log_n = 6
    c = spx.Context(0)
    c.set_witness_check(1)
    inst = _inst(oc, 0, log_n)
    mats = _perturbed(oc, inst, [5, 40])
    ref = _reference(oc, mats, inst.z_bytes)
    assert ref[0] == [5, 40]
    ppc = oc.PP.keygen(log_n, 99)
    pp = spx.PublicParameter.load(c, ppc.serialize())
    p = spx.InteractiveProver(_index(spx, c, mats), inst.v_bytes, inst.w_bytes)
    with pytest.raises(spx.WrongWitness) as e:
        p.prover_first_round(pp)
    assert "constraint 5 is not satisfied" in str(e.value)
    p.close()
    # the claim was released and the streams are idle: a new session on the context works
    q = spx.InteractiveProver(_index(spx, c, inst.mats), inst.v_bytes, inst.w_bytes)
    assert len(q.prover_first_round(pp)) == 8 + 48
    q.close()
    assert c.witness_check_stats()[:3] == (2, 1, 2)


# ---------------------------------------------------------------- sharded
def _ranks(spx, G, fn, modes=None):
    """fn(ctx, rank) on G in-process ranks (the thread pattern of tests/test_gpu_sharded.py); every thread
    must end. Returns (results, errors) per rank."""
    group = spx.CommGroup(G)
    out, errs = [None] * G, [None] * G

    def run(r):
        try:
            c = spx.Context(0)
            c.set_comm_group(group, r)
            c.set_witness_check(1 if modes is None else modes[r])
            out[r] = fn(c, r)
        except Exception as e:  # returned to the caller
            errs[r] = e

    ths = [threading.Thread(target=run, args=(r,)) for r in range(G)]
    for t in ths:
        t.start()
    for t in ths:
        t.join(timeout=120)
    for t in ths:
        assert not t.is_alive(), "a rank is still waiting (in an exchange?)"
    return out, errs


@pytest.mark.parametrize("G,log_n", [(2, 6), (4, 8)])
def test_sharded(spx, oc, G, log_n):
    inst = _inst(oc, 0, log_n)
    n = 1 << log_n
    ppb = oc.PP.keygen(log_n, 400 + log_n).serialize()
    want = oc.prove(inst.mats, inst.v_bytes, inst.w_bytes, oc.PP.load(ppb), 0, 0)
    assert _reference(oc, inst.mats, inst.z_bytes)[0] == []
    rows = [n - 3]  # the only violated row lies in the last rank's block
    mats = _perturbed(oc, inst, rows)
    ref = _reference(oc, mats, inst.z_bytes)
    assert ref[0] == rows and rows[0] >= n - n // G

    def good(c, r):
        pp = spx.PublicParameter.load(c, ppb)
        pk = _index(spx, c, inst.mats)
        proof = spx.MLArgumentForR1CS.prove(pk, inst.v_bytes, inst.w_bytes, pp)
        return proof, spx.MLArgumentForR1CS.check_witness(pk, spx.Witness(c, inst.v_bytes, inst.w_bytes))

    out, errs = _ranks(spx, G, good)
    assert errs == [None] * G, errs
    for r in range(G):
        assert out[r][0] == want, "rank %d: the checked proof differs from the single-rank proof" % r
        assert out[r][1] == (0, None, (0, 0, 0))

    def violated(c, r):
        pp = spx.PublicParameter.load(c, ppb)
        pk = _index(spx, c, mats)
        triple = spx.MLArgumentForR1CS.check_witness(pk, spx.Witness(c, inst.v_bytes, inst.w_bytes))
        try:
            spx.MLArgumentForR1CS.prove(pk, inst.v_bytes, inst.w_bytes, pp)
        except spx.WrongWitness as e:
            return triple, str(e)
        return triple, None

    out, errs = _ranks(spx, G, violated)
    assert errs == [None] * G, errs
    for r in range(G):
        assert out[r][0] == _expected(ref), "rank %d" % r
        assert out[r][1] is not None, "rank %d proved a violated witness" % r
        assert "constraint %d is not satisfied" % rows[0] in out[r][1]
        assert "(1 of %d constraints fail)" % n in out[r][1]


def test_sharded_mode_mismatch(spx, oc):
    """the check on for rank 0 and off for rank 1: both fail with InvalidArgument, nobody waits"""
    log_n, G = 6, 2
    inst = _inst(oc, 0, log_n)
    ppb = oc.PP.keygen(log_n, 400 + log_n).serialize()

    def prove(c, r):
        pp = spx.PublicParameter.load(c, ppb)
        return spx.MLArgumentForR1CS.prove(_index(spx, c, inst.mats), inst.v_bytes, inst.w_bytes, pp)

    out, errs = _ranks(spx, G, prove, modes=[1, 0])
    for r in range(G):
        assert isinstance(errs[r], spx.InvalidArgument), (r, errs[r], out[r] is not None)
        assert "witness check mode differs" in str(errs[r])
