"""Strict verification ("Subgroup membership"): with spx_ctx_set_subgroup_check on, spx_verify and
spx_verify_many reject a proof whose point lies on the curve but outside its prime-order subgroup, with
SPX_SERIALIZATION and a message naming the field, as the reference's checked deserialization does; valid
proofs stay on the batch's fast path; with the check off nothing changes."""
import json
import os
import subprocess
import sys

import pytest

import spartan
import subgroup_cases as sc
from bls12_381 import G1, G2

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LOG_NS = [4, 6]
SEED = 8300
NEW = " is not in the prime-order subgroup"

# What spx_verify answers with the check off for each tampered proof below: recorded from the build before
# the subgroup check existed (same seeds), as (exception class, message). The torsion component is
# invisible to the pairings, but the point's bytes feed the Fiat-Shamir transcript.
RECORDED = {
    (log_n, name): verdict
    for log_n in LOG_NS
    for name, verdict in (
        ("commitment", ("InvalidArgument", "public witness failed in commitment check")),
        ("opening 1 point", ("InvalidArgument", "public witness failed in commitment check")),
        ("opening 2 last point", ("WrongWitness", "Cannot verify z_ry")),
    )
}


def _torsion(cid):
    pt = next(c[1] for c in sc.cases(cid) if c[0] == "c torsion")
    from bls12_381 import g1_from_uncompressed, g2_from_uncompressed

    return (g1_from_uncompressed if cid == 1 else g2_from_uncompressed)(pt)


def _plus(curve, A, T):
    return curve.to_affine(curve.add(curve.from_affine(A), curve.from_affine(T)))


def tampers(log_n):
    """{name: (field named by the strict error, function proof bytes -> tampered bytes)}: one point
    replaced by point + torsion, which stays on the curve and decompresses"""
    t1, t2 = _torsion(1), _torsion(2)

    def commitment(b):
        p = spartan.Proof.from_bytes(b)
        p.pm1 = (p.pm1[0], _plus(G1, p.pm1[1], t1))
        return p.to_bytes()

    def opening1(b):
        p = spartan.Proof.from_bytes(b)
        z, (h, pts) = p.pm2
        p.pm2 = (z, (h, [pts[0], _plus(G2, pts[1], t2)] + pts[2:]))
        return p.to_bytes()

    def opening2_last(b):
        p = spartan.Proof.from_bytes(b)
        z, (h, pts) = p.pm6
        p.pm6 = (z, (h, pts[:-1] + [_plus(G2, pts[-1], t2)]))
        return p.to_bytes()

    return {
        "commitment": ("commitment", commitment),
        "opening 1 point": ("opening 1 proof point 1", opening1),
        "opening 2 last point": ("opening 2 proof point %d" % (log_n - 1), opening2_last),
    }


class Case:
    """an index on a context of its own (the shared one keeps its default), keys and five proofs"""

    def __init__(self, spx, oc, log_n):
        self.spx, self.L = spx, log_n
        self.ctx = spx.Context(0)
        self.log_vs = [1, 2, 3, 2, 1]
        self.insts = [oc.Instance(0, log_n, lv, SEED + log_n) for lv in self.log_vs]
        self.pp = spx.MLProofForR1CS.setup(self.ctx, log_n, 909)
        self.pk = spx.MLArgumentForR1CS.index(self.ctx, *[spx.Csr(M.n, M.row_ptr, M.col, M.val) for M in self.insts[0].mats])
        self.vp = spx.verifier_parameter(self.pp)
        self.vs = [i.v_bytes for i in self.insts]
        done = {}
        for i in self.insts:
            if i.v_bytes not in done:
                done[i.v_bytes] = spx.MLArgumentForR1CS.prove(self.pk, i.v_bytes, i.w_bytes, self.pp)
        self.proofs = [done[i.v_bytes] for i in self.insts]
        self.tampered = {name: (field, fn(self.proofs[0])) for name, (field, fn) in tampers(log_n).items()}

    def single(self, v, proof):
        """spx_verify's verdict: ("ok", "") or (exception class name, message)"""
        try:
            self.spx.MLArgumentForR1CS.verify(self.pk, v, proof, self.vp)
            return ("ok", "")
        except self.spx.SpartanError as e:
            return (type(e).__name__, str(e))

    def many(self, vs, proofs):
        res = self.spx.MLArgumentForR1CS.verify_many(self.pk, vs, proofs, self.vp)
        return [("ok", "") if r is True else (type(r).__name__, str(r)) for r in res]


_cases = {}


@pytest.fixture
def case(spx, oc):
    made = []

    def get(log_n):
        if log_n not in _cases:
            _cases[log_n] = Case(spx, oc, log_n)
        made.append(_cases[log_n])
        return _cases[log_n]

    yield get
    for c in made:
        c.ctx.set_subgroup_check(0)


@pytest.mark.parametrize("log_n", LOG_NS)
def test_valid_proofs_with_the_check_on(case, log_n):
    c = case(log_n)
    c.ctx.set_subgroup_check(1)
    L = c.L
    before = c.ctx.subgroup_stats()
    for v, p in zip(c.vs, c.proofs):
        assert c.single(v, p) == ("ok", "")
    after = c.ctx.subgroup_stats()
    # spx_verify tests the commitment and both openings' h and L quotient points on the host
    assert tuple(a - b for a, b in zip(after, before)) == (0, 5 * (1 + 2 * (L + 1)), 0)
    for k in (1, 3, 5):
        sg0, vs0 = c.ctx.subgroup_stats(), c.spx.verify_stats(c.ctx)
        assert c.many(c.vs[:k], c.proofs[:k]) == [("ok", "")] * k
        sg1, vs1 = c.ctx.subgroup_stats(), c.spx.verify_stats(c.ctx)
        npts = k + 2 * k * (L + 1)
        # one batch, no proof on the single-proof path, every point tested on the GPU and none on the host
        assert tuple(a - b for a, b in zip(vs1, vs0)) == (1, L + 2, 0, npts)
        assert tuple(a - b for a, b in zip(sg1, sg0)) == (npts, 0, 0)


@pytest.mark.parametrize("name", ["commitment", "opening 1 point", "opening 2 last point"])
@pytest.mark.parametrize("log_n", LOG_NS)
def test_check_off_is_unchanged(case, log_n, name):
    c = case(log_n)
    field, bad = c.tampered[name]
    assert bad != c.proofs[0] and len(bad) == len(c.proofs[0])
    for mode in (0, -1):  # off, and the process default with nothing set
        c.ctx.set_subgroup_check(mode)
        got = c.single(c.vs[0], bad)
        assert got == RECORDED[(log_n, name)]
        assert NEW not in got[1]
        before = c.ctx.subgroup_stats()
        assert c.many(c.vs[:3], [bad] + c.proofs[1:3]) == [got, ("ok", ""), ("ok", "")]
        assert c.ctx.subgroup_stats() == before  # no membership check ran


@pytest.mark.parametrize("name", ["commitment", "opening 1 point", "opening 2 last point"])
@pytest.mark.parametrize("log_n", LOG_NS)
def test_check_on_rejects_with_the_field_named(case, log_n, name):
    c = case(log_n)
    field, bad = c.tampered[name]
    c.ctx.set_subgroup_check(1)
    want = ("SerializationError", field + NEW)
    before = c.ctx.subgroup_stats()
    assert c.single(c.vs[0], bad) == want
    after = c.ctx.subgroup_stats()
    assert after[2] - before[2] == 1 and after[0] == before[0]
    for k, j in ((1, 0), (3, 1), (5, 4), (5, 0)):  # the tampered proof at position j of a batch of k
        vs, proofs = list(c.vs[:k]), list(c.proofs[:k])
        vs[j], proofs[j] = c.vs[0], bad
        vs0 = c.spx.verify_stats(c.ctx)
        got = c.many(vs, proofs)
        vs1 = c.spx.verify_stats(c.ctx)
        assert got == [want if i == j else ("ok", "") for i in range(k)]
        # only the rejected proof left the fast path; the others (if any) shared one combined check
        assert vs1[2] - vs0[2] == 1 and vs1[0] - vs0[0] == (1 if k > 1 else 0)


@pytest.mark.parametrize("log_n", LOG_NS)
def test_return_value_is_the_lowest_rejected_index(case, log_n):
    import ctypes

    c = case(log_n)
    c.ctx.set_subgroup_check(1)
    f_com, bad_com = c.tampered["commitment"]
    f_op, bad_op = c.tampered["opening 2 last point"]
    vs = [c.vs[1], c.vs[0], c.vs[2], c.vs[0], c.vs[4]]
    proofs = [c.proofs[1], bad_op, c.proofs[2], bad_com, c.proofs[4]]
    assert c.many(vs, proofs)[1] == ("SerializationError", f_op + NEW)
    L, spx = c.spx.lib(), c.spx
    va, na, pa, la, k = spx._many_args(vs, proofs)
    st = (ctypes.c_int * k)(*([-1] * k))
    rc = L.spx_verify_many(c.ctx.h, c.pk.h, va, na, pa, la, k, c.vp, len(c.vp), None, None, st)
    assert rc == 4 and list(st) == [0, 4, 0, 4, 0]
    assert L.spx_last_error().decode() == f_op + NEW


def test_setter_conventions(case):
    c = case(4)
    for bad in (-2, 2):
        with pytest.raises(c.spx.InvalidArgument):
            c.ctx.set_subgroup_check(bad)
    # a context claimed by a round-level session refuses the setter, as spx_ctx_set_msm_hot does
    i = c.insts[0]
    s = c.spx.InteractiveProver(c.pk, i.v_bytes, i.w_bytes)
    try:
        with pytest.raises(c.spx.InvalidArgument):
            c.ctx.set_subgroup_check(1)
    finally:
        s.close()
    c.ctx.set_subgroup_check(1)


@pytest.mark.parametrize("env,default", [("1", "on"), (None, "off"), ("0", "off")])
def test_process_default_in_a_fresh_child(case, tmp_path, env, default):
    c = case(4)
    field, bad = c.tampered["commitment"]
    job = tmp_path / "job.json"
    job.write_text(json.dumps({"log_n": 4, "log_v": c.log_vs[0], "seed": SEED + 4, "v": c.vs[0].hex(), "vp": c.vp.hex(),
                               "proof": bad.hex()}))
    e = dict(os.environ)
    e.pop("SPX_SUBGROUP_CHECK", None)
    if env is not None:
        e["SPX_SUBGROUP_CHECK"] = env
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "subgroup_env_child.py"), str(job)], env=e,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    on, off = ["SerializationError", field + NEW], list(RECORDED[(4, "commitment")])
    assert out["on"] == on and out["off"] == off
    assert out["default"] == out["default_again"] == (on if default == "on" else off)
