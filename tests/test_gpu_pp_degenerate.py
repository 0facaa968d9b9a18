"""The HIP library under the degenerate public parameter of tests/degenerate_pp.py, from spx_pp_load to
a verified proof, byte-equal to the C oracle (which tests/test_pp_degenerate.py pins to the Python
oracle on this very parameter). Trapdoor entries 0, 1 and 1/2 put half-levels at infinity and make the
two points of a pair equal, so loading it takes the branches generic parameters never reach: the
infinity flag of k_points_from_bytes and the fix_inf path of the serializer with finite points around
them, every side of k_precompute's pair sum (first / second / both infinite, and equal points: the
doubling branch of xyzz_madd), k_normalize's batch inversion over chunks of 32 that start with, end
with and have infinities inside them; commitments, openings and proofs then run the MSMs over tables
with sentinel entries, and the verifiers meet an infinite g_mask_random entry."""
import random
import threading

import pytest

import degenerate_pp as dp
import spartan

pytestmark = pytest.mark.gpu

R = spartan.R
LOG_N = dp.NV
SEED = 0x5EED0000 + LOG_N
INJ_SEED = 66


@pytest.fixture(scope="module")
def deg():
    return dp.build()


@pytest.fixture(scope="module")
def ppc(oc, deg):
    return oc.PP.load(deg.bytes)


def _csrs(spx, inst):
    return [spx.Csr(M.n, M.row_ptr, M.col, M.val) for M in inst.mats]


def test_load_serialize_subgroup(spx, ctx, deg):
    pp = spx.PublicParameter.load(ctx, deg.bytes)
    assert pp.serialize_uncompressed() == deg.bytes
    assert pp.check_subgroup() == (0, None)
    assert spx.PublicParameter.load(ctx, deg.bytes, check_subgroup=True).serialize_uncompressed() == deg.bytes


def _tables():
    rs = random.Random(LOG_N)
    n = 1 << LOG_N
    return {"random": [rs.randrange(R) for _ in range(n)], "0/1": [rs.getrandbits(1) for _ in range(n)]}


@pytest.mark.parametrize("table", ["random", "0/1"])
def test_commit_open(spx, ctx, oc, deg, ppc, table):
    pp = spx.PublicParameter.load(ctx, deg.bytes)
    tb = spx.fr_bytes(_tables()[table])
    rs = random.Random(7)
    for point in ([rs.randrange(R) for _ in range(LOG_N)], [rs.randrange(R), 0, 1] + [rs.randrange(R) for _ in range(LOG_N - 3)]):
        pb = spx.fr_bytes(point)
        assert spx.MLPolyCommit.commit(pp, tb) == oc.commit(ppc, tb, LOG_N)
        assert spx.MLPolyCommit.open(pp, tb, pb) == oc.open_(ppc, tb, LOG_N, pb)


def _prove_ranks(spx, G, inst, ppb, mode):
    """G in-process ranks (one thread and context each; G = 1: a plain context without a communicator)"""
    group = spx.CommGroup(G) if G > 1 else None
    out, errs = [None] * G, []

    def run(r):
        try:
            c = spx.Context(0)
            if group is not None:
                c.set_comm_group(group, r)
            pp = spx.PublicParameter.load(c, ppb)
            pk = spx.MLArgumentForR1CS.index(c, *_csrs(spx, inst))
            out[r] = spx.MLArgumentForR1CS.prove(pk, inst.v_bytes, inst.w_bytes, pp, mode=mode, seed=INJ_SEED)
        except Exception as e:  # surfaced below
            errs.append(repr(e))

    ths = [threading.Thread(target=run, args=(r,)) for r in range(G)]
    for t in ths:
        t.start()
    for t in ths:
        t.join(timeout=300)
    assert not errs, errs
    return out


@pytest.mark.parametrize("G", [1, 2, 4])
@pytest.mark.parametrize("mode", ["fs", "injected"])
@pytest.mark.parametrize("kind", [0, 3])
def test_prove_bit_exact(spx, oc, deg, ppc, kind, mode, G):
    inst = oc.Instance(kind, LOG_N, 2, SEED, 7 if kind == 3 else 0)
    want = oc.prove(inst.mats, inst.v_bytes, inst.w_bytes, ppc, 1 if mode == "injected" else 0, INJ_SEED)
    out = _prove_ranks(spx, G, inst, deg.bytes, mode)
    for r in range(G):
        assert out[r] == want, "rank %d of %d: proof differs from the oracle's" % (r, G)


class Case:
    """one index on a context of its own (the subgroup check is switched on it), three proofs that differ
    in |v| (kind 0's matrices do not depend on the split of z), the parameter's own verifier parameter"""

    def __init__(self, spx, oc, deg, ppc):
        self.spx, self.ctx = spx, spx.Context(0)
        self.insts = [oc.Instance(0, LOG_N, lv, SEED) for lv in (1, 2, 3)]
        self.pp = spx.PublicParameter.load(self.ctx, deg.bytes)
        self.pk = spx.MLArgumentForR1CS.index(self.ctx, *_csrs(spx, self.insts[0]))
        self.vp = deg.vp_bytes
        self.vs = [i.v_bytes for i in self.insts]
        self.proofs = [spx.MLArgumentForR1CS.prove(self.pk, i.v_bytes, i.w_bytes, self.pp) for i in self.insts]
        self.want = [oc.prove(i.mats, i.v_bytes, i.w_bytes, ppc, 0, 0) for i in self.insts]

    def single(self, v, proof):
        try:
            return self.spx.MLArgumentForR1CS.verify(self.pk, v, proof, self.vp)
        except self.spx.SpartanError as e:
            return type(e)

    def many(self, vs, proofs):
        return [r if r is True else type(r) for r in self.spx.MLArgumentForR1CS.verify_many(self.pk, vs, proofs, self.vp)]


@pytest.fixture(scope="module")
def case(spx, oc, deg, ppc):
    c = Case(spx, oc, deg, ppc)
    yield c
    c.ctx.set_subgroup_check(0)


def _tampered(proof):
    out = {}
    bad = spartan.Proof.from_bytes(proof)
    bad.pm6 = ((bad.pm6[0] + 1) % R, bad.pm6[1])
    out["pm6 value"] = bad.to_bytes()
    bad = spartan.Proof.from_bytes(proof)
    bad.sc1[2][1] = (bad.sc1[2][1] + 1) % R
    out["sumcheck evaluation"] = bad.to_bytes()
    bad = spartan.Proof.from_bytes(proof)
    z, (h, pts) = bad.pm6
    assert pts[2] != pts[3]
    bad.pm6 = (z, (h, pts[:3] + [pts[2]] + pts[4:]))  # seen by the pairing check alone
    out["second opening point"] = bad.to_bytes()
    return out


@pytest.mark.parametrize("subgroup_check", [0, 1])
def test_verify_and_verify_many(case, deg, subgroup_check):
    c = case
    assert c.proofs == c.want
    assert deg.vp.g_mask_random[1] is None  # g^{t_1}, t_1 = 0: an infinite entry of the verifier parameter
    c.ctx.set_subgroup_check(subgroup_check)
    before = c.ctx.subgroup_stats()
    for v, p in zip(c.vs, c.proofs):
        assert c.single(v, p) is True
    assert c.many(c.vs, c.proofs) == [True, True, True]
    for name, bad in _tampered(c.proofs[1]).items():
        assert bad != c.proofs[1]
        verdict = c.single(c.vs[1], bad)
        assert verdict is not True and issubclass(verdict, c.spx.SpartanError), name
        assert c.many(c.vs, [c.proofs[0], bad, c.proofs[2]]) == [True, verdict, True], name
    after = c.ctx.subgroup_stats()
    if subgroup_check:
        assert after[0] > before[0] and after[1] > before[1] and after[2] == before[2]  # points tested, none rejected
    else:
        assert after == before
