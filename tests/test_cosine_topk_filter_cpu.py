"""Row labels and per-query allow-sets of the exact top-k scans: the argument rules, the C-ABI boundary and the host-side
validation.  CPU only: every refusal here happens before any device work."""
import ctypes

import pytest
import torch

from evi_rag_amd import _lib, ops
from evi_rag_amd.dist import ShardedIndex

NEW = ("evi_cosine_topk_filtered", "evi_cosine_topk_two_stage_filtered")

Q, N, D = 3, 8, 16


def _qx():
    return torch.zeros(Q, D), torch.zeros(N, D)


def _mask():
    return torch.ones(N, dtype=torch.bool)


def _labels():
    return torch.zeros(N, dtype=torch.uint8)


def _allow(dtype=torch.int64):
    return torch.ones(Q, dtype=dtype)


@pytest.mark.parametrize("kwargs,message", [
    (dict(row_mask=_mask(), row_labels=_labels(), query_allow=_allow()), "two spellings of one filter"),
    (dict(query_allow=_allow()), "query_allow goes with row_labels"),
    (dict(row_mask=_mask(), query_allow=_allow()), "query_allow goes with row_labels"),
    (dict(row_labels=_labels()), "row_labels needs query_allow"),
    (dict(row_mask=torch.ones(N + 1, dtype=torch.bool)), "row_mask must be a bool tensor of length N = 8"),
    (dict(row_mask=torch.ones(N, dtype=torch.uint8)), "row_mask must be a bool tensor"),
    (dict(row_mask=torch.ones(N, 1, dtype=torch.bool)), "row_mask must be a bool tensor"),
    (dict(row_labels=torch.zeros(N - 1, dtype=torch.uint8), query_allow=_allow()), "row_labels must be a uint8 tensor of length N = 8"),
    (dict(row_labels=torch.zeros(N, dtype=torch.int32), query_allow=_allow()), "row_labels must be a uint8 tensor"),
    (dict(row_labels=_labels(), query_allow=torch.ones(Q + 1, dtype=torch.int64)), "query_allow must be an int32 or int64 tensor of length Q = 3"),
    (dict(row_labels=_labels(), query_allow=torch.ones(Q, dtype=torch.float32)), "query_allow must be an int32 or int64 tensor"),
    (dict(row_labels=_labels(), query_allow=torch.ones(Q, dtype=torch.uint8)), "query_allow must be an int32 or int64 tensor"),
])
@pytest.mark.parametrize("entry", ["scan", "two_stage"])
def test_filter_keywords_are_refused_with_a_message(entry, kwargs, message):
    q, x = _qx()
    with pytest.raises(ValueError, match=message):
        if entry == "scan":
            ops.cosine_topk(q, x, 2, **kwargs)
        else:
            ops.cosine_topk_two_stage(q, x, x.half(), 2, **kwargs)


@pytest.mark.parametrize("kwargs", [dict(row_mask=_mask()), dict(row_labels=_labels(), query_allow=_allow(torch.int32))])
def test_gemm_method_refuses_a_filter(kwargs):
    q, x = _qx()
    with pytest.raises(ValueError, match="method='gemm' takes no row filter"):
        ops.cosine_topk(q, x, 2, method="gemm", **kwargs)
    with pytest.raises(ValueError, match="method='gemm' takes no row filter"):
        ops.cosine_topk(q, torch.zeros(N, 64, dtype=torch.uint8), 2, method="gemm", row_scale=torch.ones(N), **kwargs)


@pytest.mark.parametrize("kwargs", [dict(row_mask=_mask()), dict(row_labels=_labels(), query_allow=_allow()),
                                    dict(row_labels=_labels(), query_allow=_allow(torch.int32))])
def test_filtered_calls_refuse_cpu_tensors(kwargs):
    """A valid filter on CPU tensors reaches the device check (before the filter keywords existed: TypeError)."""
    q, x = _qx()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.cosine_topk(q, x, 2, **kwargs)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.cosine_topk(q, x, 2, method="scan", **kwargs)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.cosine_topk_two_stage(q, x, x.half(), 2, **kwargs)


def test_sharded_index_checks_its_filter_slice():
    x = torch.zeros(N, D)
    with pytest.raises(ValueError, match="two spellings of one filter"):
        ShardedIndex(x, N, row_mask=_mask(), row_labels=_labels())
    with pytest.raises(ValueError, match="row_mask must be a torch.bool tensor with one entry per local row"):
        ShardedIndex(x, N, row_mask=torch.ones(N - 1, dtype=torch.bool))
    with pytest.raises(ValueError, match="row_labels must be a torch.uint8 tensor with one entry per local row"):
        ShardedIndex(x, N, row_labels=torch.zeros(N, dtype=torch.int64))
    idx = ShardedIndex(x, N, row_labels=_labels())
    with pytest.raises(ValueError, match="row_labels needs query_allow"):
        idx.topk(torch.zeros(Q, D), 2)
    with pytest.raises(ValueError, match="query_allow goes with row_labels"):
        ShardedIndex(x, N).topk(torch.zeros(Q, D), 2, query_allow=_allow())
    with pytest.raises(ValueError, match="a custom local_topk takes no row filter"):
        ShardedIndex(x, N, row_mask=_mask(), local_topk=lambda *a: None).topk(torch.zeros(Q, D), 2)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ShardedIndex(x, N, row_mask=_mask()).topk(torch.zeros(Q, D), 2)


def test_filtered_symbols_are_declared_exported_and_bound():
    lib = ctypes.CDLL(_lib.LIB_PATH)
    declared = set(_lib.header_symbols())
    bound = set(_lib.bound_symbols())
    assert bound == declared, f"binding/header mismatch: {bound ^ declared}"
    for name in declared:
        assert hasattr(lib, name), f"{name} declared in include/evi_hip.h but not exported"
    for name in NEW:
        assert name in declared and name in bound and hasattr(lib, name)


def test_filtered_entry_points_validate_on_the_host():
    """The refusals happen before any launch, so they are safe without a GPU."""
    lib = _lib.load()
    dummy = ctypes.create_string_buffer(64)
    p = ctypes.addressof(dummy)
    rc = lib.evi_cosine_topk_filtered(p, 4, p, 0, 100, 64, None, None, p, 5, 0, p, p, p, 64, None)
    assert rc == _lib.EVI_ERR_INVALID and "row_labels" in _lib.last_error()
    rc = lib.evi_cosine_topk_filtered(p, 4, p, 0, 100, 64, None, p, None, 5, 0, p, p, p, 64, None)
    assert rc == _lib.EVI_ERR_INVALID and "query_allow" in _lib.last_error()
    for kind in (7, -1, 4):
        rc = lib.evi_cosine_topk_filtered(p, 4, p, kind, 100, 64, None, p, p, 5, 0, p, p, p, 64, None)
        assert rc == _lib.EVI_ERR_INVALID and "kind must be" in _lib.last_error()
    # the existing rules still apply behind the filter's own
    rc = lib.evi_cosine_topk_filtered(p, 4, p, 0, 100, 24, None, p, p, 5, 0, p, p, p, 64, None)
    assert rc == _lib.EVI_ERR_UNSUPPORTED and "multiple of 16" in _lib.last_error()
    rc = lib.evi_cosine_topk_filtered(p, 4, p, 0, 100, 64, None, p, p, 0, 0, p, p, p, 64, None)
    assert rc == _lib.EVI_ERR_INVALID and "k must be" in _lib.last_error()
    rc = lib.evi_cosine_topk_filtered(p, 4, p, 2, 100, 64, None, p, p, 5, 0, p, p, p, 64, None)
    assert rc == _lib.EVI_ERR_INVALID and "row_scale" in _lib.last_error()
    rc = lib.evi_cosine_topk_two_stage_filtered(p, 4, p, p, 100, 64, None, p, 5, 0, p, p, p, 1, p, 64, None)
    assert rc == _lib.EVI_ERR_INVALID and "row_labels" in _lib.last_error()
    rc = lib.evi_cosine_topk_two_stage_filtered(p, 4, p, p, 100, 64, p, None, 5, 0, p, p, p, 1, p, 64, None)
    assert rc == _lib.EVI_ERR_INVALID and "query_allow" in _lib.last_error()


def test_filtered_calls_use_the_unfiltered_workspace_sizes():
    """Labels and allow words are caller buffers: the size functions have no filtered form and keep their values (pinned
    in test_library_abi.py); a filtered call with less than the minimum is refused like an unfiltered one."""
    lib = _lib.load()
    dummy = ctypes.create_string_buffer(64)
    p = ctypes.addressof(dummy)
    need = lib.evi_cosine_topk_min_workspace_bytes(4, 100, 64, 5)
    rc = lib.evi_cosine_topk_filtered(p, 4, p, 0, 100, 64, None, p, p, 5, 0, p, p, p, need - 1, None)
    assert rc == _lib.EVI_ERR_NOMEM and str(need) in _lib.last_error()
