"""CPU-side checks of the C-ABI boundary: the library loads and exports every declared symbol."""
import ctypes
import os

import pytest

from evi_rag_amd import _lib


def test_library_is_built():
    assert os.path.exists(_lib.LIB_PATH), "run __graft_entry__.build() first"


def test_every_header_symbol_is_exported_and_bound():
    lib = ctypes.CDLL(_lib.LIB_PATH)
    declared = _lib.header_symbols()
    assert declared, "header declares no functions?"
    for name in declared:
        assert hasattr(lib, name), f"{name} declared in include/evi_hip.h but not exported"
    bound = set(_lib.bound_symbols())
    assert bound == set(declared), f"binding/header mismatch: {bound ^ set(declared)}"


def test_version_and_error_text():
    lib = _lib.load()
    assert lib.evi_version() == 1
    # argument validation happens on the host before any device work, so it is safe without a GPU
    rc = lib.evi_topk_merge(None, None, 0, 1, 1, None, None, None)
    assert rc == _lib.EVI_ERR_INVALID
    assert "P >= 1" in _lib.last_error()
    with pytest.raises(ValueError):
        _lib.check(rc)


def test_workspace_sizes_are_monotone():
    lib = _lib.load()
    full = lib.evi_cosine_topk_workspace_bytes(32, 1 << 23, 768, 500)
    small = lib.evi_cosine_topk_min_workspace_bytes(32, 1 << 23, 768, 500)
    assert 0 < small <= full
    assert lib.evi_cosine_topk_workspace_bytes(32, 100, 768, 500) <= small


def test_ops_refuse_cpu_tensors():
    import torch
    from evi_rag_amd import ops

    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.cosine_topk(torch.zeros(2, 16), torch.zeros(4, 16), 2)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.normalize_embeddings(torch.ones(2, 16))


# Exact workspace / buffer sizes of the scorer and the top-k scans for a table of shapes (pinned from a build whose layouts
# were not refactored): a layout change that moves or resizes a field shows up here before it reaches a device.
# (N, E, B, D, H, dde_rounds, dde_reverse_rounds, num_relations) ->
#   prepare, forward workspace, backward workspace, saved per direction mode, saved_full per direction mode
_SCORER_SIZES = [
    ((100, 300, 2, 64, 64, 2, 2, 16),  # E < 1024: no pair rows
     (210688, 855296, 4317440, (619200, 463200, 463200), (690688, 534784, 534784))),
    ((5000, 20000, 8, 64, 32, 2, 2, 0),  # R = 0: per-edge relation rows
     (144896, 41580288, 156733952, (31040000, 23200000, 23200000), (38647808, 30807808, 30807808))),
    ((500, 2000, 4, 32, 64, 1, 0, 5000),  # R > E: per-edge relation rows
     (96000, 4195840, 15914496, (3104000, 2320000, 2320000), (3599104, 2815232, 2815232))),
    ((10000, 50000, 128, 64, 64, 2, 2, 40000),  # B R > 2^22: relation table without pair rows
     (210688, 143860992, 462261248, (103200000, 77200000, 77200000), (130179840, 104179968, 104179968))),
    ((20000, 60000, 16, 64, 64, 2, 2, 50),  # pair rows
     (210688, 153175552, 527213824, (123840000, 92640000, 92640000), (136038912, 104838912, 104838912))),
    ((120000, 600000, 32, 128, 96, 2, 2, 500),  # E > 262144: three edge chunks
     (683008, 1190206976, 5217041408, (2160000000, 1617600000, 1617600000), (2283442176, 1741042176, 1741042176))),
    ((1, 0, 1, 4, 4, 0, 0, 0),  # no edges
     (6656, 10496, 27648, (144, 104, 104), (4096, 4096, 4096))),
]
# (Q, N, D, k) -> GEMM top-k workspace, two-stage workspace
_TOPK_SIZES = [
    ((1, 1000, 64, 10), (140544, 345856)),
    ((32, 1 << 20, 384, 100), (4920064, 268766720)),
    ((64, 5000, 768, 500), (10040576, 2354688)),
    ((7, 300000, 1024, 50), (1093120, 77052672)),
]


@pytest.mark.parametrize("shape,want", _SCORER_SIZES)
def test_scorer_layout_sizes_are_pinned(monkeypatch, shape, want):
    for var in ("EVI_EDGE_CHUNK", "EVI_SCORER_PAIRS", "EVI_SCORER_GEMM"):
        monkeypatch.delenv(var, raising=False)
    lib = _lib.load()
    N, E, B, D, H, rounds, rev, R = shape
    got = (lib.evi_retriever_prepare_bytes(D, H, rounds, rev),
           lib.evi_retriever_forward_workspace_bytes(N, E, B, D, H, rounds, rev, R),
           lib.evi_retriever_backward_workspace_bytes(N, E, B, D, H, rounds, rev, R),
           tuple(lib.evi_retriever_saved_bytes(E, D, H, mode) for mode in range(3)),
           tuple(lib.evi_retriever_saved_bytes_full(N, E, B, D, H, rounds, rev, R, mode) for mode in range(3)))
    assert got == want


@pytest.mark.parametrize("shape,want", _TOPK_SIZES)
def test_topk_workspace_sizes_are_pinned(shape, want):
    lib = _lib.load()
    got = (lib.evi_cosine_topk_gemm_workspace_bytes(*shape), lib.evi_cosine_topk_two_stage_workspace_bytes(*shape))
    assert got == want


# (Q, N, D, k) -> scan workspace, minimum scan workspace, GEMM top-k workspace, two-stage workspace, packed record: the values
# of the build before the scan's layout moved onto Bump (shapes of the bit-for-bit tests' odd-D cases and the two bench shapes)
_TOPK_ALL_SIZES = [
    ((96, 2000, 144, 10), (541440, 541440, 13834496, 1015808, 11520)),
    ((33, 1200, 272, 10), (353024, 353024, 4667648, 559872, 3960)),
    ((96, 200, 144, 10), (80640, 80640, 13143296, 555008, 11520)),
    ((96, 2000, 96, 10), (535296, 535296, 13809920, 1009664, 11520)),
    ((96, 200, 96, 10), (74496, 74496, 13118720, 548864, 11520)),
    ((5, 2000, 416, 10), (576256, 576256, 726528, 663552, 600)),
    ((5, 200, 416, 10), (115456, 115456, 690432, 202752, 600)),
    ((32, 1 << 23, 768, 500), (2147718400, 17011968, 5020416, 2148171264, 192000)),
    ((512, 400000, 768, 500), (102634752, 17011968, 80324608, 108893696, 3072000)),
]


@pytest.mark.parametrize("shape,want", _TOPK_ALL_SIZES)
def test_topk_size_functions_are_pinned(shape, want):
    lib = _lib.load()
    Q, _, _, k = shape
    got = (lib.evi_cosine_topk_workspace_bytes(*shape), lib.evi_cosine_topk_min_workspace_bytes(*shape),
           lib.evi_cosine_topk_gemm_workspace_bytes(*shape), lib.evi_cosine_topk_two_stage_workspace_bytes(*shape),
           lib.evi_topk_packed_bytes(Q, k))
    assert got == want
