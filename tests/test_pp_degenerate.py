"""The oracles on the degenerate public parameter of tests/degenerate_pp.py (trapdoor entries 0, 1 and
1/2: infinite points, equal pairs): the C oracle, which tests/test_gpu_pp_degenerate.py compares the
HIP library with, loads it and proves under it exactly as the Python oracle does, and the Python
verifier accepts what they produce. No GPU."""
import pytest

import degenerate_pp as dp
import spartan
from bls12_381 import R
from gen import circuit_3n, uniform_3n
from transcript import InjectedChallenges

LOG_N, LOG_V = dp.NV, 2
INJ_SEED = 66


@pytest.fixture(scope="module")
def deg():
    return dp.build()


def test_parameter_holds_every_class(deg):
    """the assertions of degenerate_pp.build(), and the figures they rest on"""
    assert {c for lvl in deg.classes for c in lvl} == set(dp.PAIR_CLASSES)
    assert deg.equal_pairs[0] > 0 and deg.equal_pairs[-1] == 1  # t_0 = t_5 = 1/2
    assert deg.inf_g2[0] > 0 and deg.inf_g2[-1] == 0 and deg.inf_g1 == sum(deg.inf_g2)
    assert deg.classes[1].count("finite + infinite") > 0 and deg.classes[3].count("infinite + finite") > 0
    assert deg.vp.g_mask_random[1] is None  # g^{t_1}, t_1 = 0
    print("equal pairs per level", deg.equal_pairs, "infinite G2 points per level", deg.inf_g2, "infinite G1 points", deg.inf_g1)


def test_oracles_roundtrip_the_bytes(oc, deg):
    assert oc.PP.load(deg.bytes).serialize() == deg.bytes
    assert spartan.PublicParameter.deserialize_uncompressed(deg.bytes).serialize_uncompressed() == deg.bytes


@pytest.mark.parametrize("kind", [0, 3])
def test_c_oracle_proves_as_the_python_oracle_and_verifier_accepts(oc, deg, kind):
    """both transcript modes at log_n = 6; the Python verifier (pairing checks under the parameter's own
    verifier parameter, whose g_mask_random has an infinite entry) accepts the proof, its mKZG check
    accepts the last opening and rejects a changed value"""
    seed = 0x5EED0000 + LOG_N
    if kind == 0:
        A, B, C, v, w = uniform_3n(LOG_N, LOG_V, seed=seed)
        inst = oc.Instance(0, LOG_N, LOG_V, seed)
    else:
        A, B, C, v, w = circuit_3n(LOG_N, LOG_V, seed=seed, wseed=7)
        inst = oc.Instance(3, LOG_N, LOG_V, seed, 7)
    assert [M.to_rows() for M in inst.mats] == [A, B, C]
    ppc = oc.PP.load(deg.bytes)
    pk = spartan.index(A, B, C)
    trace = {}
    fs = spartan.prove(pk, v, w, deg.pp, trace=trace)
    assert oc.prove(inst.mats, inst.v_bytes, inst.w_bytes, ppc, 0, 0) == fs.to_bytes()
    inj = spartan.prove(pk, v, w, deg.pp, fs=InjectedChallenges(INJ_SEED))
    assert oc.prove(inst.mats, inst.v_bytes, inst.w_bytes, ppc, 1, INJ_SEED) == inj.to_bytes()
    if kind == 0:
        assert spartan.verify(pk, v, fs, deg.vp)
        z_ry, opening = fs.pm6
        assert spartan.mkzg_verify(deg.vp, fs.pm1, trace["r_y"], z_ry, opening)
        assert not spartan.mkzg_verify(deg.vp, fs.pm1, trace["r_y"], (z_ry + 1) % R, opening)
