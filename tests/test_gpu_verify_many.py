"""spx_verify_many: status[j] always equals what spx_verify gives for proof j alone. A valid
batch stays on the fast path (one Miller loop of L + 2 pairs, no proof on the single-proof path: the
structural guarantee, read from spx_verify_stats); a tampered proof gets the single path's error kind
while its neighbours stay accepted."""
import pytest

import spartan
from bls12_381 import FLAG_POS_Y, R, g2_decompress, ser_fq2

pytestmark = pytest.mark.gpu


class Case:
    """one index with its keys and up to five proofs per mode. Kind 0's matrices do not depend on how z is
    split into v and w, so its proofs differ in |v|; kind 1 repeats its one instance."""

    def __init__(self, spx, ctx, oc, kind, log_n):
        self.spx, self.ctx, self.L = spx, ctx, log_n
        log_vs = [v for v in (1, 2, 3, 2, 1)] if kind == 0 else [2] * 5
        self.insts = [oc.Instance(kind, log_n, lv, 7100 + log_n) for lv in log_vs]
        self.pp = spx.MLProofForR1CS.setup(ctx, log_n, 707)
        self.pk = spx.MLArgumentForR1CS.index(ctx, *[spx.Csr(M.n, M.row_ptr, M.col, M.val) for M in self.insts[0].mats])
        self.vp = spx.verifier_parameter(self.pp)
        self.vs = [i.v_bytes for i in self.insts]
        self._proofs = {}

    def proofs(self, mode="fs"):
        if mode not in self._proofs:
            done = {}
            for i in self.insts:  # equal instances share one prove
                if i.v_bytes not in done:
                    done[i.v_bytes] = self.spx.MLArgumentForR1CS.prove(self.pk, i.v_bytes, i.w_bytes, self.pp, mode=mode, seed=9)
            self._proofs[mode] = [done[i.v_bytes] for i in self.insts]
        return self._proofs[mode]

    def single(self, v, proof, **kw):
        """spx_verify's verdict: True or the exception class"""
        try:
            return self.spx.MLArgumentForR1CS.verify(self.pk, v, proof, self.vp, **kw)
        except self.spx.SpartanError as e:
            return type(e)

    def many(self, vs, proofs, **kw):
        """(verdicts as True / exception class, stats delta)"""
        before = self.spx.verify_stats(self.ctx)
        res = self.spx.MLArgumentForR1CS.verify_many(self.pk, vs, proofs, self.vp, **kw)
        after = self.spx.verify_stats(self.ctx)
        return [r if r is True else type(r) for r in res], tuple(a - b for a, b in zip(after, before))


_cases = {}


@pytest.fixture
def case(spx, ctx, oc):
    def get(kind, log_n):
        if (kind, log_n) not in _cases:
            _cases[(kind, log_n)] = Case(spx, ctx, oc, kind, log_n)
        return _cases[(kind, log_n)]

    return get


@pytest.mark.parametrize("kind", [0, 1])
@pytest.mark.parametrize("log_n", [4, 6, 8])
def test_all_valid_stays_on_the_fast_path(case, kind, log_n):
    c = case(kind, log_n)
    for mode in ("fs", "injected"):
        proofs = c.proofs(mode)
        for k in (1, 2, 5):
            for cached in (False, True):
                got, st = c.many(c.vs[:k], proofs[:k], mode=mode, seed=9, cached=cached)
                assert got == [True] * k, (mode, k, cached)
                # one batch, one Miller loop of L + 2 pairs, nothing on the single-proof path, and every
                # point of the batch (k commitments, 2 k (L + 1) opening points) decompressed on the GPU
                assert st == (1, c.L + 2, 0, k + 2 * k * (c.L + 1)), (mode, k, cached)


def _nonresidue_g2():
    k = 1
    while True:  # the first x = k + u with no point on the curve
        b = ser_fq2((k, 1), FLAG_POS_Y)
        try:
            g2_decompress(b)
        except ValueError:
            return b
        k += 1


def _tampered(c):
    """{name: (v, proof)} : proof 2 of the case tampered in each way test_verify_rejects_tampering uses, and
    with a G2 point that is on no curve"""
    v, proof = c.vs[2], c.proofs()[2]
    pf = spartan.Proof.from_bytes(proof)
    out = {}
    bad = spartan.Proof.from_bytes(proof)
    bad.sc1[2][1] = (bad.sc1[2][1] + 1) % R
    out["sumcheck evaluation"] = (v, bad.to_bytes())
    bad = spartan.Proof.from_bytes(proof)
    bad.pm4 = ((pf.pm4[0] + 1) % R, pf.pm4[1], pf.pm4[2])
    out["pm4"] = (v, bad.to_bytes())
    bad = spartan.Proof.from_bytes(proof)
    bad.pm6 = ((pf.pm6[0] + 1) % R, pf.pm6[1])
    out["pm6 value"] = (v, bad.to_bytes())
    bad = spartan.Proof.from_bytes(proof)
    z, (h, pts) = pf.pm2
    bad.pm2 = (z, (h, [pts[1]] + pts[1:]))
    out["opening point"] = (v, bad.to_bytes())
    bad = spartan.Proof.from_bytes(proof)
    z, (h, pts) = pf.pm6
    bad.pm6 = (z, (h, pts[:3] + [pts[2]] + pts[4:]))
    out["second opening point"] = (v, bad.to_bytes())
    v2 = bytearray(v)
    v2[32] ^= 1
    out["public input"] = (bytes(v2), proof)
    out["truncation"] = (v, proof[:-5])
    at = 56 + 32 + 96 + 8  # the first quotient point of the first opening
    out["non-residue G2 x"] = (v, proof[:at] + _nonresidue_g2() + proof[at + 96 :])
    # the same in the last message, which no challenge depends on: only the decompression can object
    out["non-residue G2 x, last point"] = (v, proof[:-96] + _nonresidue_g2())
    return out


@pytest.fixture(scope="module")
def tampered(spx, ctx, oc):
    c = _cases.get((0, 8)) or _cases.setdefault((0, 8), Case(spx, ctx, oc, 0, 8))
    t = _tampered(c)
    verdicts = {name: c.single(v, p) for name, (v, p) in t.items()}
    return c, t, verdicts


@pytest.mark.parametrize("name", ["sumcheck evaluation", "pm4", "pm6 value", "opening point", "second opening point",
                                  "public input", "truncation", "non-residue G2 x", "non-residue G2 x, last point"])
def test_one_tampered_proof(tampered, name):
    c, t, verdicts = tampered
    assert verdicts[name] is not True and issubclass(verdicts[name], c.spx.SpartanError)
    vs, proofs = list(c.vs), list(c.proofs())
    vs[2], proofs[2] = t[name]
    got, st = c.many(vs, proofs)
    assert got == [True, True, verdicts[name], True, True]
    assert st[2] >= 1  # the tampered proof was settled by the single-proof path
    if name == "second opening point":
        # no challenge depends on the last message, so only the combined pairing check can see a point
        # swapped there: the whole batch went to the single-proof path
        assert st[:3] == (1, c.L + 2, 5)
    else:
        assert st[:3] == (1, c.L + 2, 1)  # the four others stayed on the fast path


def test_two_tampered_proofs(tampered):
    c, t, verdicts = tampered
    vs, proofs = list(c.vs), list(c.proofs())
    bad = spartan.Proof.from_bytes(c.proofs()[0])
    bad.pm6 = ((bad.pm6[0] + 1) % R, bad.pm6[1])
    proofs[0] = bad.to_bytes()
    vs[3], proofs[3] = c.vs[3], c.proofs()[3][:-5]
    got, _ = c.many(vs, proofs)
    assert got == [c.single(vs[0], proofs[0]), True, True, c.spx.SerializationError, True]
    assert got[0] is not True
    # the ABI's return value is the lowest-index rejected proof's status, with its message
    res = c.spx.MLArgumentForR1CS.verify_many(c.pk, vs, proofs, c.vp)
    with pytest.raises(got[0]) as e:
        c.spx.MLArgumentForR1CS.verify(c.pk, vs[0], proofs[0], c.vp)
    assert str(res[0]) == str(e.value)


def test_entropy_does_not_change_verdicts(tampered):
    c, t, verdicts = tampered
    vs, proofs = list(c.vs), list(c.proofs())
    vs[2], proofs[2] = t["second opening point"]  # seen by the combined pairing check alone
    for entropy in (None, bytes(32), bytes(range(32)), b"\xff" * 32):
        assert c.many(c.vs, c.proofs(), entropy=entropy)[0] == [True] * 5
        assert c.many(vs, proofs, entropy=entropy)[0] == [True, True, verdicts["second opening point"], True, True]
    assert c.spx.verify_many_coeffs(c.vs, c.proofs(), c.vp, bytes(range(32))) != c.spx.verify_many_coeffs(c.vs, c.proofs(), c.vp)


def test_oracle_proof_among_gpu_proofs(case, oc):
    c = case(1, 6)
    ppc = oc.PP.load(c.pp.serialize_uncompressed())
    i = c.insts[0]
    op = oc.prove(i.mats, i.v_bytes, i.w_bytes, ppc, 0, 0)
    proofs = c.proofs()
    got, st = c.many(c.vs[:3], [proofs[0], op, proofs[2]])
    assert got == [True, True, True] and st[:3] == (1, c.L + 2, 0)


def test_different_public_input_sizes(case):
    c = case(0, 6)
    assert sorted({len(v) // 32 for v in c.vs}) == [2, 4, 8]
    got, st = c.many(c.vs, c.proofs())
    assert got == [True] * 5 and st[:3] == (1, c.L + 2, 0)
    # a proof under another proof's public input is rejected alone
    vs = list(c.vs)
    vs[1] = c.vs[0]
    got, st = c.many(vs, c.proofs())
    assert got == [True, c.single(vs[1], c.proofs()[1]), True, True, True] and got[1] is not True


def test_infinite_quotient_points(spx, ctx):
    """a witness table constant in its two lowest variables: the first two quotients of both openings are
    zero polynomials, so their proof points are infinity, and the batch accepts them (such terms drop
    out of the combinations)"""
    log_n = 4
    n = 1 << log_n
    # z_x z_0 = z_x: satisfied by every z with z_0 = 1
    A = [[(1, x)] for x in range(n)]
    B = [[(1, 0)] for _ in range(n)]
    pk = spx.MLArgumentForR1CS.index(ctx, A, B, A)
    pp = spx.MLProofForR1CS.setup(ctx, log_n, 808)
    vp = spx.verifier_parameter(pp)
    vs, proofs = [], []
    for seed in (1, 2):
        z = [1 if x < 4 else 1000 * seed + (x >> 2) for x in range(n)]
        v = spx.fr_bytes(z[:4])
        proof = spx.MLArgumentForR1CS.prove(pk, v, spx.fr_bytes(z[4:]), pp)
        pf = spartan.Proof.from_bytes(proof)
        for _z, (_h, pts) in (pf.pm2, pf.pm6):
            assert pts[0] is None and pts[1] is None and pts[3] is not None
        assert spx.MLArgumentForR1CS.verify(pk, v, proof, vp)
        vs.append(v)
        proofs.append(proof)
    before = spx.verify_stats(ctx)
    assert spx.MLArgumentForR1CS.verify_many(pk, vs, proofs, vp) == [True, True]
    after = spx.verify_stats(ctx)
    assert (after[0] - before[0], after[1] - before[1], after[2] - before[2]) == (1, log_n + 2, 0)
    # the all-zero witness: every point of the proof is infinity
    v0, w0 = spx.fr_bytes([0] * 4), spx.fr_bytes([0] * (n - 4))
    p0 = spx.MLArgumentForR1CS.prove(pk, v0, w0, pp)
    assert spx.MLArgumentForR1CS.verify(pk, v0, p0, vp)
    assert spx.MLArgumentForR1CS.verify_many(pk, vs + [v0], proofs + [p0], vp) == [True, True, True]


def test_call_errors_leave_status_alone(case):
    c = case(0, 4)
    with pytest.raises(c.spx.SerializationError):
        c.spx.MLArgumentForR1CS.verify_many(c.pk, c.vs[:2], c.proofs()[:2], c.vp[:-1])  # a bad vp
    with pytest.raises(c.spx.InvalidArgument):
        c.spx.MLArgumentForR1CS.verify_many(c.pk, [], [], c.vp)  # nproofs < 1
