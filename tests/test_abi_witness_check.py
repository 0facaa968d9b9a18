"""The witness check's interface without a GPU: include/spartan_hip.h declares spx_ctx_set_witness_check,
spx_witness_check and spx_witness_check_stats, the package's symbol list names them, the library exports
them, the Python classes carry the new methods, and each function refuses a null context (the pattern of
tests/test_abi_msm_skew.py)."""
import ctypes

from test_abi import declared_functions

NEW = ["spx_ctx_set_witness_check", "spx_witness_check", "spx_witness_check_stats"]


def test_header_declares_and_package_lists_them(spx):
    names = declared_functions()
    for n in NEW:
        assert n in names, n
        assert n in spx.EXPORTED, n
        assert hasattr(spx.lib(), n), n


def test_python_classes_have_the_methods(spx):
    assert hasattr(spx.Context, "set_witness_check") and hasattr(spx.Context, "witness_check_stats")
    assert hasattr(spx.MLArgumentForR1CS, "check_witness")


def test_null_context_is_refused(spx):
    L = spx.lib()
    out = (ctypes.c_uint64 * 4)()
    bad, first = ctypes.c_uint64(), ctypes.c_uint64()
    assert L.spx_ctx_set_witness_check(None, 1) != 0
    assert L.spx_witness_check(None, None, None, ctypes.byref(bad), ctypes.byref(first), None) != 0
    assert L.spx_witness_check_stats(None, out) != 0
