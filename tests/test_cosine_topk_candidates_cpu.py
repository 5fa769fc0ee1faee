"""Top-k over per-query candidate id lists: the argument rules, the C-ABI boundary and the host-side validation.
CPU only: every refusal here happens before any device work."""
import ctypes

import pytest
import torch

from evi_rag_amd import _lib, ops
from evi_rag_amd.dist import ShardedIndex

NEW = ("evi_cosine_topk_candidates_workspace_bytes", "evi_cosine_topk_candidates")

Q, N, D, C = 3, 8, 16, 4


def _qx():
    return torch.zeros(Q, D), torch.zeros(N, D)


def _padded(dtype=torch.int64):
    return torch.zeros(Q, C, dtype=dtype)


def _flat(dtype=torch.int64):
    return torch.zeros(Q * C, dtype=dtype)


def _ptr(n=Q + 1, dtype=torch.int64):
    return torch.arange(n, dtype=dtype) * C


def test_candidate_symbols_are_declared_exported_and_bound():
    lib = ctypes.CDLL(_lib.LIB_PATH)
    declared = set(_lib.header_symbols())
    bound = set(_lib.bound_symbols())
    assert bound == declared, f"binding/header mismatch: {bound ^ declared}"
    for name in NEW:
        assert name in declared and name in bound and hasattr(lib, name)


@pytest.mark.parametrize("candidates,kwargs,message", [
    (_padded(torch.int32), {}, r"candidates \[Q, C\] must be int64"),
    (_padded(torch.float32), {}, r"candidates \[Q, C\] must be int64"),
    (_flat(torch.float32), dict(cand_ptr=_ptr()), r"candidates \[T\] must be int64 or int32"),
    (_flat(torch.int16), dict(cand_ptr=_ptr()), r"candidates \[T\] must be int64 or int32"),
    (torch.zeros(Q, C, 1, dtype=torch.int64), {}, "candidates must be a tensor"),
    (torch.zeros((), dtype=torch.int64), {}, "candidates must be a tensor"),
    (_flat(), {}, "a 1-D candidate list needs cand_ptr"),
    (_flat(torch.int32), {}, "a 1-D candidate list needs cand_ptr"),
    (_padded(), dict(cand_ptr=_ptr()), "cand_ptr goes with a 1-D candidate list"),
    (torch.zeros(Q + 1, C, dtype=torch.int64), {}, "one row per query"),
    (_flat(), dict(cand_ptr=_ptr(Q)), r"cand_ptr must have Q \+ 1 = 4 entries, got 3"),
    (_flat(), dict(cand_ptr=_ptr(Q + 2)), r"cand_ptr must have Q \+ 1 = 4 entries, got 5"),
    (_flat(), dict(cand_ptr=_ptr(dtype=torch.int32)), "cand_ptr must be a 1-D int64 tensor"),
    (_flat(), dict(cand_ptr=_ptr().view(2, 2)), "cand_ptr must be a 1-D int64 tensor"),
    (_padded(), dict(fp8_mfma=True), "fp8_mfma goes with an e4m3"),
])
def test_argument_rules_are_refused_with_a_message(candidates, kwargs, message):
    q, x = _qx()
    with pytest.raises(ValueError, match=message):
        ops.cosine_topk_candidates(q, x, candidates, 2, **kwargs)


def test_e4m3_index_needs_row_scale_and_half_index_refuses_fp8_mfma():
    q = torch.zeros(Q, 64)
    with pytest.raises(ValueError, match="an fp8 index needs row_scale"):
        ops.cosine_topk_candidates(q, torch.zeros(N, 64, dtype=torch.uint8), _padded(), 2)
    with pytest.raises(ValueError, match="fp8_mfma goes with an e4m3"):
        ops.cosine_topk_candidates(q, torch.zeros(N, 64, dtype=torch.float16), _padded(), 2, fp8_mfma=True)
    with pytest.raises(ValueError, match="queries and index must be 2D"):
        ops.cosine_topk_candidates(q[0], torch.zeros(N, 64), _padded(), 2)


def test_it_takes_no_filter_keywords_and_no_method():
    q, x = _qx()
    with pytest.raises(TypeError):
        ops.cosine_topk_candidates(q, x, _padded(), 2, method="scan")
    with pytest.raises(TypeError):
        ops.cosine_topk_candidates(q, x, _padded(), 2, row_mask=torch.ones(N, dtype=torch.bool))


@pytest.mark.parametrize("candidates,kwargs", [(_padded(), {}), (_flat(), dict(cand_ptr=_ptr())), (_flat(torch.int32), dict(cand_ptr=_ptr()))])
def test_valid_arguments_on_cpu_tensors_reach_the_device_check(candidates, kwargs):
    q, x = _qx()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.cosine_topk_candidates(q, x, candidates, 2, **kwargs)


def test_sharded_index_refuses_a_custom_local_topk_and_cpu_tensors():
    x = torch.zeros(N, D)
    with pytest.raises(ValueError, match="a custom local_topk takes no candidate lists"):
        ShardedIndex(x, N, local_topk=lambda *a: None).topk_candidates(torch.zeros(Q, D), _padded(), 2)
    with pytest.raises(ValueError, match="a 1-D candidate list needs cand_ptr"):
        ShardedIndex(x, N).topk_candidates(torch.zeros(Q, D), _flat(), 2)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ShardedIndex(x, N).topk_candidates(torch.zeros(Q, D), _flat(), 2, cand_ptr=_ptr())


def _call(lib, p, *, q="p", Q=4, idx="p", kind=0, N=100, D=64, row_scale=None, ids="p", ptr="p", T=50, k=5, out_s="p", out_i="p",
          ws="p", ws_bytes=None):
    """evi_cosine_topk_candidates with every pointer = the dummy buffer unless named None; the workspace size defaults to
    exactly what the size function asks for."""
    pick = lambda v: p if v == "p" else v  # noqa: E731
    if ws_bytes is None:
        ws_bytes = lib.evi_cosine_topk_candidates_workspace_bytes(Q, T, max(k, 1))
    return lib.evi_cosine_topk_candidates(pick(q), Q, pick(idx), kind, N, D, pick(row_scale), pick(ids), pick(ptr), T, k, 0, N,
                                          pick(out_s), pick(out_i), None, pick(ws), ws_bytes, None)


def test_entry_point_validates_on_the_host():
    """The refusals happen before any launch, so they are safe without a GPU."""
    lib = _lib.load()
    dummy = ctypes.create_string_buffer(64)
    p = ctypes.addressof(dummy)
    for kind in (-1, 4, 7):
        assert _call(lib, p, kind=kind) == _lib.EVI_ERR_INVALID and "kind must be" in _lib.last_error()
    # D follows the rule of the scan of the same kind
    for kind, D_bad, text in ((0, 24, "multiple of 16"), (0, 0, "multiple of 16"), (0, 1296, "multiple of 16"), (1, 48, "multiple of 32"),
                              (2, 96, "multiple of 64"), (3, 32, "multiple of 64")):
        rc = _call(lib, p, kind=kind, D=D_bad, row_scale="p")
        assert rc == _lib.EVI_ERR_UNSUPPORTED and text in _lib.last_error(), (kind, D_bad, _lib.last_error())
    for k in (0, -3, _lib.EVI_TOPK_MAX_K + 1):
        assert _call(lib, p, k=k) == _lib.EVI_ERR_INVALID and "k must be in [1, 2048]" in _lib.last_error()
    for kind in (2, 3):
        assert _call(lib, p, kind=kind) == _lib.EVI_ERR_INVALID and "row_scale" in _lib.last_error()
    assert _call(lib, p, N=2 ** 31 - 1) == _lib.EVI_ERR_INVALID and "2^31-1 rows" in _lib.last_error()
    assert _call(lib, p, T=-1, ws_bytes=64) == _lib.EVI_ERR_INVALID and "T >= 0" in _lib.last_error()
    for name in ("q", "idx", "ids", "ptr", "out_s", "out_i", "ws"):
        rc = _call(lib, p, **{name: None})
        assert rc == _lib.EVI_ERR_INVALID and "null pointer" in _lib.last_error(), name
    need = lib.evi_cosine_topk_candidates_workspace_bytes(4, 50, 5)
    rc = _call(lib, p, ws_bytes=need - 1)
    assert rc == _lib.EVI_ERR_NOMEM and str(need) in _lib.last_error()
    # Q == 0 is valid and does nothing (no pointer is looked at)
    assert _call(lib, p, Q=0, q=None, out_s=None, out_i=None, ws=None, ws_bytes=0) == _lib.EVI_OK


def test_workspace_size_is_positive_and_monotone_in_T():
    lib = _lib.load()
    sizes = [lib.evi_cosine_topk_candidates_workspace_bytes(32, T, 500) for T in (0, 1, 16, 1000, 1536 * 32, 65536 * 32, 2 ** 30)]
    assert all(s > 0 for s in sizes)
    assert all(a <= b for a, b in zip(sizes, sizes[1:])) and sizes[0] < sizes[-1]
    assert sizes[-1] < 64 * 2 ** 30  # tens of bytes per entry, not hundreds
    assert lib.evi_cosine_topk_candidates_workspace_bytes(32, 1000, 1) == lib.evi_cosine_topk_candidates_workspace_bytes(32, 1000, 2048)
    assert lib.evi_cosine_topk_candidates_workspace_bytes(-1, 10, 5) == 0
    assert lib.evi_cosine_topk_candidates_workspace_bytes(4, -1, 5) == 0
    assert lib.evi_cosine_topk_candidates_workspace_bytes(4, 10, 0) == 0
