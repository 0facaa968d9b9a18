"""CPU side of the public-parameter structure work ("Public-parameter structure and views"):
the identities the library relies on, asserted on the Python oracle's points, and spx_pc_verify
(MLPolyCommit::verify on the host pairing, no GPU) against the oracle's opening and its mkzg_verify.

With bit 0 of x paired with t_i:
  fold    powers[i][2b] + powers[i][2b+1] = powers[i+1][b]   (the last level's pair sums to g / h)
  mask    sum_b powers_of_g[i][2b+1] = g^{t_i} = vp.g_mask_random[i]
  suffix  keygen(nv - k, gs, hs, t[k:]) = {powers_of_g[k:], powers_of_h[k:], g, h}, g_mask[k:]"""
import ctypes
import random

import pytest

import pp_structure_cases as cases
import spartan

R = spartan.R


@pytest.fixture(scope="module", params=["random", "degenerate"])
def fx(request):
    return cases.random_pp() if request.param == "random" else cases.degenerate()


def test_fold_identity(fx):
    assert cases.fold_failures(fx.pp) == []


def test_fold_identity_sees_a_replaced_point():
    fx = cases.random_pp()
    pg = [list(lvl) for lvl in fx.pp.powers_of_g]
    pg[1][5] = pg[1][2]
    bad = spartan.PublicParameter(fx.nv, pg, fx.pp.powers_of_h, fx.pp.g, fx.pp.h)
    assert cases.fold_failures(bad) == cases.expected_failures(fx.nv, 1, 1, 5) == [(1, 0, 5), (1, 1, 2)]


def test_mask_identity(fx):
    assert cases.odd_sums(fx.pp) == list(fx.vp.g_mask_random)


def test_suffix_identity(fx):
    for k in ((1, 2, 3) if fx.nv == cases.RANDOM_NV else (2, 5)):
        pp, vp, _ = spartan.keygen_from_scalars(fx.nv - k, fx.gs, fx.hs, fx.t[k:])
        want_pp, want_vp = cases.sliced(fx.pp, fx.vp, k)
        assert pp.serialize_uncompressed() == want_pp.serialize_uncompressed(), k
        assert vp.serialize_uncompressed() == want_vp.serialize_uncompressed(), k


def test_byte_helpers_address_the_points():
    fx = cases.random_pp()
    nv, b = fx.nv, fx.bytes
    from bls12_381 import g1_uncompressed, g2_uncompressed

    assert cases.get_point(b, nv, 1, 0, 0) == g1_uncompressed(fx.pp.powers_of_g[0][0])
    assert cases.get_point(b, nv, 1, 2, 3) == g1_uncompressed(fx.pp.powers_of_g[2][3])
    assert cases.get_point(b, nv, 2, 3, 1) == g2_uncompressed(fx.pp.powers_of_h[3][1])
    assert b[cases.g_offset(nv):cases.g_offset(nv) + 96] == g1_uncompressed(fx.pp.g)
    assert len(b) == cases.g_offset(nv) + 96 + 192
    swapped = cases.swap_points(b, nv, 1, 0, 0, 1)
    got = spartan.PublicParameter.deserialize_uncompressed(swapped)
    assert got.powers_of_g[0][:2] == fx.pp.powers_of_g[0][1::-1] and got.powers_of_g[0][2:] == fx.pp.powers_of_g[0][2:]


# ------------------------------------------------------------------ spx_pc_verify (host only)
class Opening:
    def __init__(self):
        fx = cases.random_pp()
        rs = random.Random(0x0FE1)
        self.fx, self.nv = fx, fx.nv
        self.table = [rs.randrange(R) for _ in range(1 << fx.nv)]
        self.point = [rs.randrange(R) for _ in range(fx.nv)]
        self.com = spartan.commit(fx.pp, self.table)
        self.value, self.proof, _ = spartan.open_(fx.pp, self.table, self.point)
        self.com_b = spartan.commitment_bytes(self.com)
        self.proof_b = spartan.open_proof_bytes(self.proof)


@pytest.fixture(scope="module")
def opening():
    return Opening()


def _pc_verify(spx, vp, com, point, value, proof):
    """(status, accepted) of the raw entry point"""
    ok = ctypes.c_int(-1)
    pb = spx.fr_bytes(point)
    rc = spx.lib().spx_pc_verify(vp, len(vp), com, pb, len(point), spx.fr_bytes([value]), proof, len(proof), ctypes.byref(ok))
    return rc, ok.value


def test_pc_verify_accepts_the_oracle_opening(spx, opening):
    o = opening
    assert len(o.proof_b) == 96 + 8 + 96 * o.nv and len(o.com_b) == 56
    assert spartan.mkzg_verify(o.fx.vp, o.com, o.point, o.value, o.proof) is True
    assert _pc_verify(spx, o.fx.vp_bytes, o.com_b, o.point, o.value, o.proof_b) == (0, 1)
    assert spx.MLPolyCommit.verify(o.fx.vp_bytes, o.com_b, o.point, spx.fr_bytes([o.value]), o.proof_b) is True


def test_pc_verify_rejects_what_the_oracle_rejects(spx, opening):
    o = opening
    vpb = o.fx.vp_bytes
    # a changed value: the oracle's verdict, and the library's equal to it
    assert spartan.mkzg_verify(o.fx.vp, o.com, o.point, (o.value + 1) % R, o.proof) is False
    assert _pc_verify(spx, vpb, o.com_b, o.point, (o.value + 1) % R, o.proof_b) == (0, 0)
    # a changed point coordinate
    point = list(o.point)
    point[2] = (point[2] + 1) % R
    assert _pc_verify(spx, vpb, o.com_b, point, o.value, o.proof_b) == (0, 0)
    # another commitment (the oracle's commitment to another table)
    other = spartan.commitment_bytes(spartan.commit(o.fx.pp, [x ^ 1 for x in o.table]))
    assert other != o.com_b
    assert _pc_verify(spx, vpb, other, o.point, o.value, o.proof_b) == (0, 0)
    # another proof point (proof point 1 in the place of proof point 3)
    h, pts = o.proof
    assert pts[1] != pts[3]
    bad = spartan.open_proof_bytes((h, pts[:3] + [pts[1]]))
    assert _pc_verify(spx, vpb, o.com_b, o.point, o.value, bad) == (0, 0)
    # the proof's own h is not read (verify.rs:15)
    free_h = spartan.open_proof_bytes((pts[0], pts))
    assert _pc_verify(spx, vpb, o.com_b, o.point, o.value, free_h) == (0, 1)


def test_pc_verify_errors(spx, opening):
    o = opening
    vpb = o.fx.vp_bytes
    INVALID, SERIALIZATION = 1, 4
    assert issubclass(spx._ERRORS[INVALID], spx.InvalidArgument) and issubclass(spx._ERRORS[SERIALIZATION], spx.SerializationError)
    # a wrong proof length, a point of another length than vp.nv
    assert _pc_verify(spx, vpb, o.com_b, o.point, o.value, o.proof_b[:-96])[0] == INVALID
    assert _pc_verify(spx, vpb, o.com_b, o.point, o.value, o.proof_b + bytes(96))[0] == INVALID
    assert _pc_verify(spx, vpb, o.com_b, o.point[:-1], o.value, o.proof_b[:-96])[0] == INVALID
    # a non-canonical proof point: the 48 bytes of x.c0 all ones, 2^384 - 1 > q
    at = 96 + 8 + 96 * 2
    noncanon = bytearray(o.proof_b)
    noncanon[at:at + 48] = b"\xff" * 48
    assert _pc_verify(spx, vpb, o.com_b, o.point, o.value, bytes(noncanon))[0] == SERIALIZATION
    assert "G2" in spx.lib().spx_last_error().decode()
    # a non-canonical value
    ok = ctypes.c_int(-1)
    rc = spx.lib().spx_pc_verify(vpb, len(vpb), o.com_b, spx.fr_bytes(o.point), o.nv, b"\xff" * 32, o.proof_b,
                                 len(o.proof_b), ctypes.byref(ok))
    assert rc == SERIALIZATION
    with pytest.raises(spx.InvalidArgument):
        spx.MLPolyCommit.verify(vpb, o.com_b, o.point, spx.fr_bytes([o.value]), o.proof_b[:-1])
