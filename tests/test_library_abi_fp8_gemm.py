"""The exported, declared and bound function sets still agree with the e4m3 many-query entry points added (CPU only)."""
import ctypes

from evi_rag_amd import _lib

NEW = ("evi_cosine_topk_gemm_fp8", "evi_cosine_topk_gemm_fp8_selection")


def test_fp8_gemm_symbols_are_declared_exported_and_bound():
    lib = ctypes.CDLL(_lib.LIB_PATH)
    declared = set(_lib.header_symbols())
    bound = set(_lib.bound_symbols())
    assert bound == declared, f"binding/header mismatch: {bound ^ declared}"
    for name in declared:
        assert hasattr(lib, name), f"{name} declared in include/evi_hip.h but not exported"
    for name in NEW:
        assert name in declared and name in bound and hasattr(lib, name)


def test_fp8_gemm_validates_on_the_host():
    """Both refusals happen before any device work, so they are safe without a GPU."""
    lib = _lib.load()
    dummy = ctypes.create_string_buffer(64)
    p = ctypes.addressof(dummy)
    rc = lib.evi_cosine_topk_gemm_fp8(p, 4, p, 100, 64, None, 5, 0, 1, p, p, p, p, 64, None)
    assert rc == _lib.EVI_ERR_INVALID and "row_scale" in _lib.last_error()
    rc = lib.evi_cosine_topk_gemm_fp8(p, 4, p, 100, 96, p, 5, 0, 1, p, p, p, p, 64, None)
    assert rc == _lib.EVI_ERR_UNSUPPORTED and "multiple of 64" in _lib.last_error()
    rc = lib.evi_cosine_topk_gemm_fp8(p, 4, p, 100, 1344, p, 5, 0, 0, p, p, p, p, 64, None)
    assert rc == _lib.EVI_ERR_UNSUPPORTED
