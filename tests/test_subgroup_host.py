"""Subgroup membership on the host ("Subgroup membership"): spx_point_in_subgroup_host against
the oracle's definition [r] P = O on every class of subgroup_cases.py, and the generated constants."""
import importlib.util
import os

import pytest

import subgroup_cases as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("cid", [1, 2])
def test_host_function_equals_the_oracle(spx, cid):
    cs = sc.cases(cid)
    names = {c[0][0] for c in cs}
    assert names == set("abcdefg")
    # the small-order class holds every prime below 2^16 that divides the cofactor
    assert [c[0] for c in cs if c[0].startswith("e ")] == ["e order %d" % l for l in sc.small_primes(sc.CURVES[cid][1])]
    for name, pt, want in cs:
        assert spx.point_in_subgroup_host(cid, pt) == want, name


def test_small_primes_of_the_cofactors():
    assert sc.small_primes(sc.H1) == [3, 11, 10177]
    assert sc.small_primes(sc.H2) == [13, 23, 2713, 11953]


def test_host_function_argument_errors(spx):
    L = spx.lib()
    import ctypes

    ok = ctypes.c_int(7)
    assert L.spx_point_in_subgroup_host(3, bytes(192), ctypes.byref(ok)) == 1  # SPX_INVALID_ARGUMENT
    assert L.spx_point_in_subgroup_host(1, None, ctypes.byref(ok)) == 1
    assert L.spx_point_in_subgroup_host(1, bytes(96), None) == 1
    with pytest.raises(spx.InvalidArgument):
        spx.point_in_subgroup_host(2, bytes(96))


def test_generator_reproduces_the_committed_constants():
    spec = importlib.util.spec_from_file_location("gen_subgroup_consts", os.path.join(ROOT, "tools", "gen_subgroup_consts.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    with open(os.path.join(ROOT, "r1cs-spartan_amd", "csrc", "subgroup_consts.hpp")) as f:
        assert f.read() == gen.render()
    beta, c_x, c_y = gen.constants()
    assert hex(beta).startswith("0x5f19672fdf")
    # the other cube root of unity would test [z^2 - 1] P instead
    assert beta != 1 and pow(beta, 3, gen.Q) == 1 and beta != pow(beta, 2, gen.Q)
