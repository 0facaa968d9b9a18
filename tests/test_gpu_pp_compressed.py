"""The compressed public-parameter form on the GPU ("Compressed public parameters"): the bulk
decompression and compression kernels against the oracle byte for byte (and against the batch verifier's
kernel), spx_pp_load_compressed / spx_pp_serialize_compressed against the images of
tests/pp_compressed_cases.py, proofs under a compressed-loaded parameter, staging chunks that straddle level
and curve boundaries, rejections that name the lowest offender, and views of a compressed-loaded parent."""
import ctypes

import pytest

import pp_compressed_cases as cc
import subgroup_cases as sc
from bls12_381 import FLAG_POS_Y, Q, g1_compress, g1_from_uncompressed, g2_compress, g2_from_uncompressed

pytestmark = pytest.mark.gpu

SERIALIZATION = 4
SIZES = [1, 2, 3, 63, 64, 65, 127, 128, 129, 255, 256, 257, 513]


def _csrs(spx, inst):
    return [spx.Csr(M.n, M.row_ptr, M.col, M.val) for M in inst.mats]


def _fixture(which):
    return cc.degenerate() if which == "degenerate" else cc.random_pp(which)


# ------------------------------------------------------------------ kernels
def _expect(spx_fn, ctx, picks, size):
    out, ok = spx_fn(ctx, b"".join(c[0] for c in picks))
    assert ok == [c[2] for c in picks]
    for i, c in enumerate(picks):
        assert out[size * i:size * (i + 1)] == c[1], i
    return out, ok


@pytest.mark.parametrize("cid", [1, 2])
@pytest.mark.parametrize("n", SIZES)
def test_bulk_decompress_matches_oracle_and_verifier_kernel(spx, ctx, cid, n):
    bulk, parent = (spx.g1_decompress_bulk, spx.g1_decompress) if cid == 1 else (spx.g2_decompress_bulk, spx.g2_decompress)
    size = 96 * cid
    picks, _ = cc.batch(cid, n)
    got = _expect(bulk, ctx, picks, size)
    assert got == parent(ctx, b"".join(c[0] for c in picks))
    for picks in cc.last_batches(cid, n):  # every special case as the last point
        _expect(bulk, ctx, picks, size)


def test_g2_points_whose_curve_equation_lies_in_fq(spx, ctx):
    """x^3 + b in Fq and no square there: the alpha = -1 branch of the Fq2 root, beside ordinary and rejected
    points in one batch"""
    special = list(cc.fq_rhs_points())
    pool = cc.pool(2)
    picks = [pool[0], special[0], special[1], pool[41], special[2], pool[1], special[3], pool[42], special[4], special[5]]
    got = _expect(spx.g2_decompress_bulk, ctx, picks, 192)
    assert got == spx.g2_decompress(ctx, b"".join(c[0] for c in picks))
    assert spx.g2_compress(ctx, b"".join(c[1] for c in special)) == b"".join(c[0] for c in special)


@pytest.mark.parametrize("cid", [1, 2])
@pytest.mark.parametrize("n", SIZES)
def test_compress_matches_oracle(spx, ctx, cid, n):
    fn = spx.g1_compress if cid == 1 else spx.g2_compress
    valid = [c for c in cc.pool(cid) if c[2]]  # 40 points and infinity
    picks = [valid[(37 + i) % len(valid)] for i in range(n)]  # infinity at 3, 44, ...: both parities
    assert fn(ctx, b"".join(c[1] for c in picks)) == b"".join(c[0] for c in picks)
    picks[-1] = valid[40]  # infinity last
    assert fn(ctx, b"".join(c[1] for c in picks)) == b"".join(c[0] for c in picks)


# ------------------------------------------------------------------ load and serialize
@pytest.mark.parametrize("which", [1, 2, 5, "degenerate"])
def test_load_and_serialize_both_forms(spx, ctx, which):
    fx = _fixture(which)
    a = spx.PublicParameter.load_compressed(ctx, fx.image)
    assert a.nv == fx.nv
    assert a.serialize_uncompressed() == fx.bytes
    assert a.serialize_compressed() == fx.image
    b = spx.PublicParameter.load(ctx, fx.bytes)
    assert b.serialize_compressed() == fx.image
    # the two handles cannot be told apart
    assert [a.window_plan(i) for i in range(-1, fx.nv)] == [b.window_plan(i) for i in range(-1, fx.nv)]
    assert a.derive_vp() == b.derive_vp() == fx.vp_bytes
    assert a.mem_info() == b.mem_info()
    assert a.check_subgroup() == (0, None) and a.check_structure() == (0, None, 1)
    if fx.nv > 1:
        view = a.view(fx.nv - 1)
        assert view.serialize_compressed() == cc.pp_image(fx.pp, 1)
    n = ctypes.c_size_t(0)
    assert spx.lib().spx_pp_serialize_compressed(a.h, None, 0, ctypes.byref(n)) == 0 and n.value == len(fx.image)
    small = ctypes.create_string_buffer(16)
    assert spx.lib().spx_pp_serialize_compressed(a.h, small, 16, ctypes.byref(n)) == 1  # SPX_INVALID_ARGUMENT


def test_generated_parameter_round_trips(spx, ctx):
    pp = spx.MLProofForR1CS.setup(ctx, 7, 0xC0DE)
    img = pp.serialize_compressed()
    assert len(img) == spx.serialized_size(7, True)
    again = spx.PublicParameter.load_compressed(ctx, img, check_subgroup=True, check_structure=True)
    assert again.serialize_uncompressed() == pp.serialize_uncompressed()
    assert spx.vp_convert(spx.verifier_parameter(pp), True) == spx.vp_convert(again.derive_vp(), True)


# ------------------------------------------------------------------ proofs
@pytest.mark.parametrize("which", [5, "degenerate"])
def test_proofs_equal_under_both_loads(spx, ctx, oc, which):
    fx = _fixture(which)
    log_n = fx.nv
    inst = oc.Instance(0, log_n, 2, 0x5EED0000 + log_n)
    want = oc.prove(inst.mats, inst.v_bytes, inst.w_bytes, oc.PP.load(fx.bytes), 0, 0)
    pk = spx.MLArgumentForR1CS.index(ctx, *_csrs(spx, inst))
    pc = spx.PublicParameter.load_compressed(ctx, fx.image)
    pu = spx.PublicParameter.load(ctx, fx.bytes)
    got = spx.MLArgumentForR1CS.prove(pk, inst.v_bytes, inst.w_bytes, pc)
    assert got == spx.MLArgumentForR1CS.prove(pk, inst.v_bytes, inst.w_bytes, pu)
    assert got == want
    vp = spx.vp_convert(spx.vp_convert(fx.vp_bytes, True), False)
    assert vp == fx.vp_bytes
    assert spx.MLArgumentForR1CS.verify(pk, inst.v_bytes, got, vp) is True


# ------------------------------------------------------------------ staging chunks
def test_small_staging_chunks_straddle_levels_and_curves(spx, ctx, monkeypatch):
    """nv = 5: levels of 32, 16, 8, 4 and 2 points, 62 per curve, G1 first. Of the chunks of 8 points, [0, 8)
    .. [24, 32) lie inside G1 level 0, [56, 64) holds G1 levels 3 and 4 and the first two points of G2 level 0,
    and [88, 96) the last six points of G2 level 0 and the first two of level 1."""
    fx = cc.random_pp(5)
    want = spx.PublicParameter.load_compressed(ctx, fx.image)
    monkeypatch.setenv("SPX_PP_STAGE_LOG", "3")
    pp = spx.PublicParameter.load_compressed(ctx, fx.image)
    assert pp.serialize_compressed() == fx.image  # serialized in chunks of 8 too
    assert spx.PublicParameter.load(ctx, fx.bytes).serialize_compressed() == fx.image
    monkeypatch.delenv("SPX_PP_STAGE_LOG")
    assert pp.serialize_uncompressed() == fx.bytes == want.serialize_uncompressed()
    assert pp.serialize_compressed() == fx.image
    deg = cc.degenerate()
    monkeypatch.setenv("SPX_PP_STAGE_LOG", "0")  # one point per chunk
    assert spx.PublicParameter.load_compressed(ctx, deg.image).serialize_uncompressed() == deg.bytes


# ------------------------------------------------------------------ rejections
def _load_fails(spx, ctx, data):
    h = ctypes.c_void_p()
    rc = spx.lib().spx_pp_load_compressed(ctx.h, bytes(data), len(data), ctypes.byref(h))
    assert not h.value  # no handle
    return rc, spx.lib().spx_last_error().decode()


def _plant(img, at, point):
    return img[:at] + point + img[at + len(point):]


def test_framing_errors(spx, ctx):
    fx = cc.random_pp(5)
    img, nv = fx.image, fx.nv
    for cut in (12, cc.point_offset(nv, 1, 1, 3) + 7, cc.h_offset(nv) - 1, len(img) - 1):
        assert _load_fails(spx, ctx, img[:cut]) == (SERIALIZATION, "truncated public parameter bytes")
    at = cc.point_offset(nv, 1, 2, 0) - 8  # the length word of G1 level 2
    assert _load_fails(spx, ctx, _plant(img, at, (9).to_bytes(8, "little"))) == (SERIALIZATION, "powers_of_g level size")
    at = cc.point_offset(nv, 2, 0, 0) - 8
    assert _load_fails(spx, ctx, _plant(img, at, (16).to_bytes(8, "little"))) == (SERIALIZATION, "powers_of_h level size")
    assert _load_fails(spx, ctx, _plant(img, 8, (4).to_bytes(8, "little")))[1] == "powers_of_g length != nv"
    assert _load_fails(spx, ctx, _plant(img, 0, (27).to_bytes(8, "little")))[0] == SERIALIZATION


@pytest.mark.parametrize("stage_log", [None, "3"])
def test_rejected_points_name_the_lowest_offender(spx, ctx, monkeypatch, stage_log):
    if stage_log is not None:
        monkeypatch.setenv("SPX_PP_STAGE_LOG", stage_log)
    fx = cc.random_pp(5)
    img, nv = fx.image, fx.nv
    noncanon = cc.raw_fq(Q + 3, FLAG_POS_Y)
    nopoint2 = cc.pool(2)[41][0]
    g1_at, g2_at, h_at = cc.point_offset(nv, 1, 1, 3), cc.point_offset(nv, 2, 0, 7), cc.h_offset(nv)
    bad_h = cc.raw_fq(Q + 1) + img[h_at + 48:]
    alone_g1 = _plant(img, g1_at, noncanon)
    alone_g2 = _plant(img, g2_at, nopoint2)
    alone_h = _plant(img, h_at, bad_h)
    all3 = _plant(_plant(alone_g1, g2_at, nopoint2), h_at, bad_h)
    assert _load_fails(spx, ctx, all3) == (SERIALIZATION, "powers_of_g level 1 point 3: x is not canonical")
    assert _load_fails(spx, ctx, alone_g1) == (SERIALIZATION, "powers_of_g level 1 point 3: x is not canonical")
    assert _load_fails(spx, ctx, alone_g2) == (SERIALIZATION, "powers_of_h level 0 point 7: no point on the curve with this x")
    assert _load_fails(spx, ctx, alone_h) == (SERIALIZATION, "h: x is not canonical")
    g2_and_h = _plant(alone_g2, h_at, bad_h)
    assert _load_fails(spx, ctx, g2_and_h)[1] == "powers_of_h level 0 point 7: no point on the curve with this x"
    # within a curve the lower level wins, then the lower index; g comes after every level
    two = _plant(_plant(img, cc.point_offset(nv, 2, 2, 5), noncanon + noncanon), cc.point_offset(nv, 2, 4, 1), nopoint2)
    assert _load_fails(spx, ctx, two)[1] == "powers_of_h level 2 point 5: x is not canonical"
    bad_g = _plant(img, cc.g_offset(nv), cc.pool(1)[41][0])
    assert _load_fails(spx, ctx, bad_g)[1] == "g: no point on the curve with this x"
    assert _load_fails(spx, ctx, _plant(bad_g, h_at, bad_h))[1] == "g: no point on the curve with this x"
    with pytest.raises(spx.SerializationError, match="powers_of_g level 1 point 3"):
        spx.PublicParameter.load_compressed(ctx, all3)


def test_checked_load_rejects_a_point_outside_the_subgroup(spx, ctx):
    fx = cc.random_pp(5)
    nv = fx.nv
    out1 = next(c[1] for c in sc.cases(1) if c[0] == "d multiple + torsion")
    out2 = next(c[1] for c in sc.cases(2) if c[0] == "b random")
    for cid, lvl, idx, pt in ((1, 0, 5, g1_compress(g1_from_uncompressed(out1))), (2, 1, 2, g2_compress(g2_from_uncompressed(out2)))):
        img = _plant(fx.image, cc.point_offset(nv, cid, lvl, idx), pt)
        pp = spx.PublicParameter.load_compressed(ctx, img)  # on the curve: the unchecked load takes it
        assert pp.serialize_compressed() == img
        want = spx.PublicParameter.load(ctx, pp.serialize_uncompressed()).check_subgroup(strict=False)
        assert pp.check_subgroup(strict=False) == want == (1, (cid, lvl, idx))
        name = "powers_of_%s level %d index %d" % ("g" if cid == 1 else "h", lvl, idx)
        with pytest.raises(spx.SerializationError, match="outside the prime-order subgroup: " + name):
            spx.PublicParameter.load_compressed(ctx, img, check_subgroup=True)


# ------------------------------------------------------------------ views and ownership
def test_view_outlives_its_compressed_loaded_parent(spx, ctx, oc):
    fx = cc.random_pp(5)
    parent = spx.PublicParameter.load_compressed(ctx, fx.image)
    view = parent.view(4)
    assert view.mem_info()[2] == 2
    assert spx.lib().spx_pp_free(parent.h) == 0
    parent.h = None
    assert view.mem_info()[2] == 1
    want_img = cc.pp_image(fx.pp, 1)
    assert view.serialize_compressed() == want_img
    sliced = spx.PublicParameter.load_compressed(ctx, want_img)
    assert view.serialize_uncompressed() == sliced.serialize_uncompressed()
    inst = oc.Instance(0, 4, 1, 0x5EED0004)
    pk = spx.MLArgumentForR1CS.index(ctx, *_csrs(spx, inst))
    want = oc.prove(inst.mats, inst.v_bytes, inst.w_bytes, oc.PP.load(sliced.serialize_uncompressed()), 0, 0)
    assert spx.MLArgumentForR1CS.prove(pk, inst.v_bytes, inst.w_bytes, view) == want
    assert spx.MLArgumentForR1CS.prove(pk, inst.v_bytes, inst.w_bytes, sliced) == want
