"""spx_verify_many's host side, no GPU needed: the coefficient derivation (spx_verify_many_coeffs against
hashlib.blake2s), the argument checks of the call, and the batched identity itself,

    C = sum_o rho_o com_o - (sum_o rho_o v_o) g,  A_i = sum_o rho_o pi_{o,i},  B = sum_o sum_i (rho_o z_{o,i}) pi_{o,i},
    e(C, h) e(g, B) prod_i e(-g_mask_i, A_i) = 1,

evaluated with the oracle's curve arithmetic on oracle proofs and checked by the product's host pairing."""
import ctypes
import hashlib

import pytest

import spartan
from bls12_381 import G1, G2, R, g1_uncompressed, g2_uncompressed, msm_naive

TAG = b"spx-verify-many-v1"


def _coeffs_ref(vs, proofs, vp, entropy):
    h = hashlib.blake2s(TAG + vp + (entropy if entropy is not None else bytes(32)))
    for v, p in zip(vs, proofs):
        h.update((len(v) // 32).to_bytes(8, "little") + v + len(p).to_bytes(8, "little") + p)
    seed = h.digest()
    out = []
    for i in range(2 * len(proofs)):
        rho = int.from_bytes(hashlib.blake2s(seed + i.to_bytes(8, "little")).digest()[:16], "little")
        out.append(rho or 1)
    return out


@pytest.fixture(scope="module")
def batch(oc):
    """three oracle proofs at log_n = 3 under one keygen (public inputs of 2, 2 and 4 elements)"""
    log_n = 3
    ppc = oc.PP.keygen(log_n, 77)
    pp = spartan.PublicParameter.deserialize_uncompressed(ppc.serialize())
    # the verifier parameter from the keygen's trapdoor (setup.rs:91-101): g_mask_random[i] = g^{t_i}
    vp = spartan.VerifierParameter(log_n, pp.g, pp.h, [G1.mul_affine(pp.g, t) for t in ppc.trapdoor(log_n)])
    items = []
    for j, log_v in enumerate((1, 1, 2)):
        inst = oc.Instance(0, log_n, log_v, 500 + j)
        items.append((inst, oc.prove(inst.mats, inst.v_bytes, inst.w_bytes, ppc, 0, 0)))
    return vp, items


@pytest.mark.parametrize("k", [1, 3])
@pytest.mark.parametrize("entropy", [None, bytes(range(32))])
def test_coeffs_match_blake2s(spx, batch, k, entropy):
    vp, items = batch
    vpb = vp.serialize_uncompressed()
    vs = [it[0].v_bytes for it in items[:k]]
    proofs = [it[1] for it in items[:k]]
    got = spx.verify_many_coeffs(vs, proofs, vpb, entropy)
    assert got == _coeffs_ref(vs, proofs, vpb, entropy)
    assert len(got) == 2 * k and all(0 < c < 1 << 128 for c in got)
    # one changed proof byte changes every coefficient
    bad = bytearray(proofs[-1])
    bad[len(bad) // 2] ^= 1
    other = spx.verify_many_coeffs(vs, proofs[:-1] + [bytes(bad)], vpb, entropy)
    assert other == _coeffs_ref(vs, proofs[:-1] + [bytes(bad)], vpb, entropy)
    assert all(a != b for a, b in zip(got, other))


def test_entropy_changes_coeffs(spx, batch):
    vp, items = batch
    vpb = vp.serialize_uncompressed()
    vs, proofs = [items[0][0].v_bytes], [items[0][1]]
    a = spx.verify_many_coeffs(vs, proofs, vpb)
    assert a == spx.verify_many_coeffs(vs, proofs, vpb, bytes(32))  # no entropy = 32 zero bytes
    assert a != spx.verify_many_coeffs(vs, proofs, vpb, b"\x01" + bytes(31))
    with pytest.raises(spx.InvalidArgument):
        spx.verify_many_coeffs(vs, proofs, vpb, b"short")


def test_verify_many_fails_loudly(spx, batch):
    """NULL arguments and a missing context give the error kind spx_verify gives; status[] stays untouched"""
    vp, items = batch
    vpb = vp.serialize_uncompressed()
    L = spx.lib()
    v, proof = items[0][0].v_bytes, items[0][1]
    o = spx._Opts(0, 0, 0, 0)
    single = L.spx_verify(None, None, v, len(v) // 32, proof, len(proof), vpb, len(vpb), ctypes.byref(o))
    assert single != 0
    va = (ctypes.c_char_p * 1)(v)
    pa = (ctypes.c_char_p * 1)(proof)
    na = (ctypes.c_size_t * 1)(len(v) // 32)
    la = (ctypes.c_size_t * 1)(len(proof))
    st = (ctypes.c_int * 1)(-7)
    assert L.spx_verify_many(None, None, va, na, pa, la, 1, vpb, len(vpb), ctypes.byref(o), None, st) == single
    assert L.spx_last_error()
    assert st[0] == -7
    assert L.spx_verify_many(None, None, None, na, pa, la, 1, vpb, len(vpb), ctypes.byref(o), None, st) == single
    assert L.spx_verify_many(None, None, va, na, pa, la, 1, vpb, len(vpb), ctypes.byref(o), None, None) == single
    out = ctypes.create_string_buffer(64)
    assert L.spx_verify_many_coeffs(va, na, pa, la, 0, vpb, len(vpb), None, out) == single  # nproofs < 1
    assert L.spx_verify_many_coeffs(va, na, pa, la, 1, vpb, len(vpb), None, None) == single
    stats = (ctypes.c_uint64 * 4)()
    assert L.spx_verify_stats(None, stats) == single


def _rows(M):
    rp = list(M.row_ptr)
    return [[(int.from_bytes(M.val.raw[32 * k : 32 * k + 32], "little"), M.col[k]) for k in range(rp[x], rp[x + 1])]
            for x in range(M.n)]


def _openings(vp, items):
    """(commitment, point, value, quotient points) of both openings of every proof, in coefficient order"""
    out = []
    for inst, pb in items:
        vk = spartan.index(*[_rows(M) for M in inst.mats])
        v = [int.from_bytes(inst.v_bytes[32 * i : 32 * i + 32], "little") for i in range(len(inst.v_bytes) // 32)]
        proof = spartan.Proof.from_bytes(pb)
        pts = {}
        assert spartan.verify(vk, v, proof, vp, out=pts)  # each proof is valid alone (pairings included)
        com = proof.pm1[1]
        out.append((com, pts["r_v0"], proof.pm2[0], proof.pm2[1][1]))
        out.append((com, pts["r_y"], proof.pm6[0], proof.pm6[1][1]))
    return out


def _identity_pairs(vp, ops, rho):
    nv = vp.nv
    vsum = sum(r * o[2] for r, o in zip(rho, ops)) % R
    C = msm_naive(G1, [o[0] for o in ops] + [vp.g], list(rho) + [(R - vsum) % R])
    g1 = [g1_uncompressed(G1.to_affine(C)), g1_uncompressed(vp.g)]
    B = msm_naive(G2, [o[3][i] for o in ops for i in range(nv)], [r * o[1][i] % R for r, o in zip(rho, ops) for i in range(nv)])
    g2 = [g2_uncompressed(vp.h), g2_uncompressed(G2.to_affine(B))]
    for i in range(nv):
        g1.append(g1_uncompressed(G1.neg_affine(vp.g_mask_random[i])))
        g2.append(g2_uncompressed(G2.to_affine(msm_naive(G2, [o[3][i] for o in ops], rho))))
    return g1, g2


def test_batched_identity_on_oracle_proofs(spx, batch):
    vp, items = batch
    vpb = vp.serialize_uncompressed()
    rho = spx.verify_many_coeffs([it[0].v_bytes for it in items], [it[1] for it in items], vpb)
    ops = _openings(vp, items)
    assert len(rho) == len(ops) == 6
    g1, g2 = _identity_pairs(vp, ops, rho)
    assert len(g1) == vp.nv + 2  # L + 2 pairs for the whole batch
    assert spx.pairing_product_is_one(g1, g2)
    # a value shifted by 1 is rejected
    bad = list(ops)
    bad[3] = (ops[3][0], ops[3][1], (ops[3][2] + 1) % R, ops[3][3])
    assert not spx.pairing_product_is_one(*_identity_pairs(vp, bad, rho))
    # and so is a quotient point swapped for another valid one
    bad = list(ops)
    q = list(ops[2][3])
    q[0] = q[1]
    bad[2] = (ops[2][0], ops[2][1], ops[2][2], q)
    assert not spx.pairing_product_is_one(*_identity_pairs(vp, bad, rho))
