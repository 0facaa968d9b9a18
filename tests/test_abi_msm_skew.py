"""The hot-bucket interface without a GPU: include/spartan_hip.h declares spx_ctx_set_msm_hot and
spx_msm_skew_stats, the package's symbol list names them, the library exports them, and both refuse a
null context (the pattern of tests/test_abi.py)."""
import ctypes

from test_abi import declared_functions

NEW = ["spx_ctx_set_msm_hot", "spx_msm_skew_stats"]


def test_header_declares_and_package_lists_them(spx):
    names = declared_functions()
    for n in NEW:
        assert n in names, n
        assert n in spx.EXPORTED, n
        assert hasattr(spx.lib(), n), n
    assert hasattr(spx.Context, "set_msm_hot") and hasattr(spx.Context, "msm_skew_stats")


def test_null_context_is_refused(spx):
    L = spx.lib()
    out = (ctypes.c_uint64 * 4)()
    assert L.spx_ctx_set_msm_hot(None, 1) != 0
    assert L.spx_msm_skew_stats(None, out) != 0
