"""Row labels and per-query allow-sets of the GEMM-shaped many-query pass: the argument rules, the C-ABI boundary and the
host-side validation.  CPU only: every refusal here happens before any device work."""
import ctypes

import pytest
import torch

from evi_rag_amd import _lib, ops
from evi_rag_amd.dist import ShardedIndex

Q, N, D = 3, 8, 64


def _qx(kind):
    q = torch.zeros(Q, D)
    if kind == "f16":
        return q, torch.zeros(N, D, dtype=torch.float16), {}
    if kind == "fp8":
        return q, torch.zeros(N, D, dtype=torch.uint8), {"row_scale": torch.ones(N)}
    return q, torch.zeros(N, D), {}


def _mask():
    return torch.ones(N, dtype=torch.bool)


def _labels():
    return torch.zeros(N, dtype=torch.uint8)


def _allow(dtype=torch.int64):
    return torch.ones(Q, dtype=dtype)


@pytest.mark.parametrize("kwargs,message", [
    (dict(row_mask=_mask(), row_labels=_labels(), query_allow=_allow()), "two spellings of one filter"),
    (dict(row_mask=_mask(), query_allow=_allow()), "query_allow goes with row_labels"),
    (dict(row_labels=_labels()), "row_labels needs query_allow"),
    (dict(row_mask=torch.ones(N, dtype=torch.uint8)), "row_mask must be a bool tensor"),
    (dict(row_mask=torch.ones(N + 1, dtype=torch.bool)), "row_mask must be a bool tensor of length N = 8"),
    (dict(row_labels=torch.zeros(N, dtype=torch.int32), query_allow=_allow()), "row_labels must be a uint8 tensor"),
    (dict(row_labels=torch.zeros(N - 1, dtype=torch.uint8), query_allow=_allow()), "row_labels must be a uint8 tensor of length N = 8"),
    (dict(row_labels=_labels(), query_allow=torch.ones(Q, dtype=torch.float32)), "query_allow must be an int32 or int64 tensor"),
    (dict(row_labels=_labels(), query_allow=torch.ones(Q + 1, dtype=torch.int64)), "query_allow must be an int32 or int64 tensor of length Q = 3"),
])
@pytest.mark.parametrize("kind", ["f32", "f16", "fp8"])
def test_filter_keywords_are_refused_with_a_message(kind, kwargs, message):
    """The argument rules of cosine_topk's filter, raised on CPU tensors: before the device check."""
    q, x, kw = _qx(kind)
    with pytest.raises(ValueError, match=message):
        ops.cosine_topk_gemm(q, x, 2, **kw, **kwargs)


@pytest.mark.parametrize("kwargs", [dict(row_mask=_mask()), dict(row_labels=_labels(), query_allow=_allow()),
                                    dict(row_labels=_labels(), query_allow=_allow(torch.int32))])
@pytest.mark.parametrize("kind", ["f32", "f16", "fp8"])
def test_a_valid_filter_reaches_the_device_check(kind, kwargs):
    """cosine_topk_gemm takes the three keywords (before they existed: TypeError); a valid filter on CPU tensors gets as
    far as the device check."""
    q, x, kw = _qx(kind)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.cosine_topk_gemm(q, x, 2, **kw, **kwargs)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.cosine_topk_gemm(q, x, 2, fallback=False, **kw, **kwargs)


def test_cosine_topk_points_to_the_filtered_pass():
    """ops.cosine_topk keeps refusing method='gemm' with a filter and names the call that takes one."""
    q, x, _ = _qx("f32")
    with pytest.raises(ValueError, match=r"cosine_topk_gemm\(\.\.\., row_labels="):
        ops.cosine_topk(q, x, 2, method="gemm", row_mask=_mask())


def test_the_entry_point_is_declared_exported_and_bound():
    name = "evi_cosine_topk_gemm_filtered"
    lib = ctypes.CDLL(_lib.LIB_PATH)
    assert name in _lib.header_symbols(), "not declared in include/evi_hip.h"
    assert hasattr(lib, name), "not exported by libevi_hip.so"
    restype, argtypes = _lib.bound_symbols()[name]
    assert restype is ctypes.c_int and len(argtypes) == 19
    assert hasattr(_lib.load(), name)


def _call(lib, p, *, kind=0, labels=True, allow=True, products=3, shadow=None, D=64, k=5, ws=64, row_scale=None):
    return lib.evi_cosine_topk_gemm_filtered(p, 4, p, kind, 100, D, row_scale, p if labels else None, p if allow else None, k, 0,
                                             products, shadow, p, p, p, p, ws, None)


def test_the_entry_point_validates_on_the_host():
    """The refusals happen before any launch, so they are safe without a GPU."""
    lib = _lib.load()
    dummy = ctypes.create_string_buffer(64)
    p = ctypes.addressof(dummy)
    assert _call(lib, p, labels=False) == _lib.EVI_ERR_INVALID and "row_labels" in _lib.last_error()
    assert _call(lib, p, allow=False) == _lib.EVI_ERR_INVALID and "query_allow" in _lib.last_error()
    for kind in (7, -1, 4):
        assert _call(lib, p, kind=kind) == _lib.EVI_ERR_INVALID and "kind must be" in _lib.last_error()
    # an e4m3 index has one selection precision and no bf16 shadow
    for kind in (2, 3):
        assert _call(lib, p, kind=kind, products=1, row_scale=p) == _lib.EVI_ERR_INVALID and "products = 3" in _lib.last_error()
        assert _call(lib, p, kind=kind, shadow=p, row_scale=p) == _lib.EVI_ERR_INVALID and "shadow" in _lib.last_error()
        assert _call(lib, p, kind=kind) == _lib.EVI_ERR_INVALID and "row_scale" in _lib.last_error()
    # the rules of the unfiltered pass still apply behind the filter's own
    assert _call(lib, p, products=2) == _lib.EVI_ERR_INVALID and "products must be" in _lib.last_error()
    assert _call(lib, p, k=0) == _lib.EVI_ERR_INVALID and "k must be" in _lib.last_error()
    assert _call(lib, p, D=24) == _lib.EVI_ERR_UNSUPPORTED and "multiple of 16" in _lib.last_error()
    assert _call(lib, p, kind=1, D=48) == _lib.EVI_ERR_UNSUPPORTED and "multiple of 32" in _lib.last_error()
    assert _call(lib, p, kind=1, products=1, shadow=p) == _lib.EVI_ERR_INVALID and "shadow" in _lib.last_error()


def test_the_filtered_pass_uses_the_unfiltered_workspace_size():
    """Labels and allow words are caller buffers: evi_cosine_topk_gemm_workspace_bytes has no filtered form (its values are
    pinned in test_library_abi.py), and a filtered call with one byte less is refused like an unfiltered one."""
    lib = _lib.load()
    dummy = ctypes.create_string_buffer(64)
    p = ctypes.addressof(dummy)
    need = lib.evi_cosine_topk_gemm_workspace_bytes(4, 100, 64, 5)
    assert _call(lib, p, ws=need - 1) == _lib.EVI_ERR_NOMEM and str(need) in _lib.last_error()


def test_sharded_index_with_the_gemm_method_takes_a_filter():
    x = torch.zeros(N, D)
    idx = ShardedIndex(x, N, method="gemm", row_mask=_mask())
    assert idx.method == "gemm" and idx.row_mask is not None
    with pytest.raises(RuntimeError, match="no CPU fallback"):  # the filtered many-query pass, not cosine_topk's refusal
        idx.topk(torch.zeros(Q, D), 2)
    lab = ShardedIndex(x, N, method="gemm", row_labels=_labels())
    with pytest.raises(ValueError, match="row_labels needs query_allow"):
        lab.topk(torch.zeros(Q, D), 2)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        lab.topk(torch.zeros(Q, D), 2, query_allow=_allow())
