"""The compressed public-parameter interface without a GPU: include/spartan_hip.h declares the new functions,
the package's symbol list names them, the library exports them, the Python classes carry the methods, and the
functions refuse null handles (the pattern of tests/test_abi_witness_check.py)."""
import ctypes

from test_abi import declared_functions

NEW = ["spx_pp_load_compressed", "spx_pp_serialize_compressed", "spx_pp_serialized_size", "spx_vp_convert",
       "spx_g1_decompress_bulk", "spx_g2_decompress_bulk", "spx_g1_compress", "spx_g2_compress"]
INVALID = 1


def test_header_declares_and_package_lists_them(spx):
    names = declared_functions()
    for n in NEW:
        assert n in names, n
        assert n in spx.EXPORTED, n
        assert hasattr(spx.lib(), n), n


def test_python_carries_the_methods(spx):
    assert hasattr(spx.PublicParameter, "load_compressed") and hasattr(spx.PublicParameter, "serialize_compressed")
    for n in ("serialized_size", "vp_convert", "g1_decompress_bulk", "g2_decompress_bulk", "g1_compress", "g2_compress"):
        assert callable(getattr(spx, n)), n


def test_null_handles_are_refused(spx):
    L = spx.lib()
    h = ctypes.c_void_p()
    n = ctypes.c_size_t(0)
    buf = ctypes.create_string_buffer(192)
    assert L.spx_pp_load_compressed(None, bytes(312), 312, ctypes.byref(h)) == INVALID and not h.value
    assert L.spx_pp_serialize_compressed(None, buf, 192, ctypes.byref(n)) == INVALID
    assert L.spx_pp_serialized_size(3, 1, None) == INVALID
    assert L.spx_vp_convert(None, 0, 1, buf, 192, ctypes.byref(n)) == INVALID
    assert L.spx_g1_decompress_bulk(None, bytes(48), 1, buf, buf) == INVALID
    assert L.spx_g2_decompress_bulk(None, bytes(96), 1, buf, buf) == INVALID
    assert L.spx_g1_compress(None, bytes(96), 1, buf) == INVALID
    assert L.spx_g2_compress(None, bytes(192), 1, buf) == INVALID
