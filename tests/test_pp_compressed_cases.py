"""The compressed wire form without a GPU: tests/pp_compressed_cases.py is pinned to the oracle (every point
of its images decompresses to the oracle's point, the lengths follow the framing), spx_pp_serialized_size
gives the lengths of the oracle's images in both forms, and spx_vp_convert takes the oracle's verifier
parameters from one form to the other byte for byte and rejects malformed input."""
import ctypes

import pytest

import pp_compressed_cases as cc
from bls12_381 import FLAG_INF, FLAG_POS_Y, Q, g1_decompress, g2_decompress, ser_fq

SERIALIZATION = 4


def _fixtures():
    return [cc.random_pp(nv) for nv in cc.NVS] + [cc.degenerate()]


@pytest.mark.parametrize("which", [1, 2, 5, "degenerate"])
def test_image_decompresses_to_the_oracle_points(which):
    fx = cc.degenerate() if which == "degenerate" else cc.random_pp(which)
    assert fx.nv == (6 if which == "degenerate" else which)
    assert len(fx.image) == cc.image_length(fx.nv)
    assert len(fx.bytes) == cc.uncompressed_length(fx.nv)
    nv, g1, g2, g, h = cc.parse_image(fx.image)
    assert nv == fx.nv
    assert [[g1_decompress(c) for c in lvl] for lvl in g1] == fx.pp.powers_of_g
    assert [[g2_decompress(c) for c in lvl] for lvl in g2] == fx.pp.powers_of_h
    assert g1_decompress(g) == fx.pp.g and g2_decompress(h) == fx.pp.h
    assert [len(lvl) for lvl in g1] == [1 << (nv - i) for i in range(nv)] == [len(lvl) for lvl in g2]
    # the offsets the rejection tests plant at
    assert fx.image[cc.point_offset(nv, 1, nv - 1, 1):][:48] == g1[nv - 1][1]
    assert fx.image[cc.point_offset(nv, 2, 0, 1):][:96] == g2[0][1]
    assert fx.image[cc.g_offset(nv):][:48] == g and fx.image[cc.h_offset(nv):] == h
    if which == "degenerate":  # half-levels at infinity reach the image as flagged zeros
        inf = sum(c[47] & FLAG_INF != 0 for lvl in g1 for c in lvl)
        assert inf == cc.degenerate_pp.build().inf_g1 > 0


def test_sub_image_is_the_sliced_parameter():
    fx = cc.random_pp(5)
    nv, g1, g2, g, h = cc.parse_image(cc.pp_image(fx.pp, 1))
    assert nv == 4 and [[g1_decompress(c) for c in lvl] for lvl in g1] == fx.pp.powers_of_g[1:]
    assert [[g2_decompress(c) for c in lvl] for lvl in g2] == fx.pp.powers_of_h[1:]


def test_batches_place_every_special_case():
    for cid in (1, 2):
        assert [c[2] for c in cc.pool(cid)] == [True] * 41 + [False] * 3
        for n in (63, 64, 65, 127, 128, 129, 255, 256, 257, 513):
            picks, placed = cc.batch(cid, n)
            assert len(picks) == n and all(v == {"even", "odd"} for v in placed.values())
            for s in cc.SPECIALS:
                at = [i for i, c in enumerate(picks) if c is cc.pool(cid)[s]]
                assert {i % 2 for i in at} == {0, 1}
            lasts = cc.last_batches(cid, n)
            assert [b[-1] for b in lasts] == [cc.pool(cid)[s] for s in cc.SPECIALS]
        assert [b[0] for b in cc.last_batches(cid, 1)] == [cc.pool(cid)[s] for s in cc.SPECIALS]


def test_points_of_the_other_square_root_branch():
    pts = cc.fq_rhs_points()
    assert len(pts) == 6 and len({c[0] for c in pts}) == 6
    for comp, unc, ok in pts:
        assert ok and unc[96:144] == bytes(48)  # y = c u
        assert g2_decompress(comp) is not None
    assert {c[0][95] & FLAG_POS_Y for c in pts} == {0, FLAG_POS_Y}


def test_serialized_size(spx):
    for fx in _fixtures():
        assert spx.serialized_size(fx.nv, True) == len(fx.image)
        assert spx.serialized_size(fx.nv, False) == len(fx.bytes)
    for nv in range(1, 9):
        assert spx.serialized_size(nv, True) == cc.image_length(nv)
        assert spx.serialized_size(nv, False) == cc.uncompressed_length(nv)
    n = ctypes.c_size_t(0)
    for nv in (0, -1, 27, 64):
        assert spx.lib().spx_pp_serialized_size(nv, 1, ctypes.byref(n)) != 0
        with pytest.raises(spx.InvalidArgument):
            spx.serialized_size(nv, False)
    assert spx.lib().spx_pp_serialized_size(26, 0, ctypes.byref(n)) == 0 and n.value == cc.uncompressed_length(26)


def test_vp_convert_matches_the_oracle(spx):
    for fx in _fixtures():
        assert spx.vp_convert(fx.vp_bytes, True) == fx.vp_image
        assert spx.vp_convert(fx.vp_image, False) == fx.vp_bytes
    deg = cc.degenerate()
    assert deg.vp.g_mask_random[1] is None  # an infinite entry, both ways above
    assert deg.vp_image[8 + 48 + 96 + 8 + 48:][:48] == ser_fq(0, FLAG_INF)


def test_vp_convert_rejects_malformed_input(spx):
    fx = cc.random_pp(2)
    for data, to in ((fx.vp_image, False), (fx.vp_bytes, True)):
        for cut in (4, 8 + 20, len(data) - 1):
            with pytest.raises(spx.SerializationError, match="truncated"):
                spx.vp_convert(data[:cut], to)
        with pytest.raises(spx.SerializationError, match="trailing"):
            spx.vp_convert(data + b"\0", to)
    img = fx.vp_image
    mask1 = 8 + 48 + 96 + 8 + 48  # g_mask_random[1]
    bad = img[:mask1] + cc.raw_fq(Q + 1, FLAG_POS_Y) + img[mask1 + 48:]
    with pytest.raises(spx.SerializationError, match="g_mask_random point: x is not canonical"):
        spx.vp_convert(bad, False)
    nopoint = cc.pool(1)[41][0]
    bad = img[:8] + nopoint + img[8 + 48:]
    with pytest.raises(spx.SerializationError, match="g: no point on the curve with this x"):
        spx.vp_convert(bad, False)
    bad = img[:8 + 48] + cc.pool(2)[41][0] + img[8 + 48 + 96:]
    with pytest.raises(spx.SerializationError, match="h: no point on the curve with this x"):
        spx.vp_convert(bad, False)
    n = ctypes.c_size_t(0)
    out = ctypes.create_string_buffer(16)
    assert spx.lib().spx_vp_convert(img[:30], 30, 0, out, 16, ctypes.byref(n)) == SERIALIZATION
    assert spx.lib().spx_vp_convert(img, len(img), 0, out, 16, ctypes.byref(n)) == 1  # buffer too small
    assert n.value == len(fx.vp_bytes)
