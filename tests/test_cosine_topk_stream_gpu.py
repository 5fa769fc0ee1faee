"""GPU parity for the scan kernel's load-group stream (k_cosine_score): tile-count edges of the one-loop stream, every
load-group shape, three segments with and without row_scale, a list on which every candidate passes, the f16 / e4m3 kinds
through the same template, and the selection of the dense first segment with ties placed 8 192 rows apart (today one
workgroup per query selects that segment; the test pins the ordering contract for a selection split into 8 192-row slices).

Inputs follow SURVEY.md §8(d) (N(0,1) rows, row 0 zero, 1 % duplicated rows, one zero query); the reference is
oracle.cosine.cosine_scores and the check tests.helpers.check_topk_against_scores with its default tolerance.  Sizes are
written in W = 16 x the device's CU count: one tile of 16 rows per wave of a full grid.  A base index and its reference
scores are made once per width and shared; a case takes its first N rows."""
import functools

import numpy as np
import pytest
import torch

from oracle import cosine as ocos
from tests.helpers import check_topk_against_scores

pytestmark = pytest.mark.gpu

EPS = 1e-6
DENSE = 65536  # rows of the dense first segment


def _w(dev):
    return 16 * torch.cuda.get_device_properties(dev).multi_processor_count


def _make_index(n, d, seed, dup_frac=0.01):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((n, d), dtype=np.float32)
    x[0] = 0.0
    ndup = int(n * dup_frac)
    if ndup > 0 and n > 2:
        src = rng.integers(1, n, size=ndup)
        dst = rng.integers(1, n, size=ndup)
        x[dst] = x[src]
    return x


def _make_queries(q_count, d, seed):
    q = np.random.default_rng(seed).standard_normal((q_count, d), dtype=np.float32)
    if q_count > 2:
        q[1] = 0.0  # a zero query: all scores tie at 0 -> pure id order
    return q


@functools.lru_cache(maxsize=2)
def _base(dev, d, q_count, n_max):
    """(normalised index on the device, normalised queries on the device, oracle scores [Q, n_max]) of one width."""
    from evi_rag_amd import ops

    x = _make_index(n_max, d, seed=n_max * 7 + d)
    q = _make_queries(q_count, d, seed=q_count + 13)
    xn = ops.normalize_embeddings(torch.from_numpy(x).to(dev), EPS)
    qn = ops.normalize_embeddings(torch.from_numpy(q).to(dev), EPS)
    ref = ocos.cosine_scores(q, x, EPS)
    ref.setflags(write=False)
    return xn, qn, ref


def _rows(dev, spec):
    w = _w(dev)
    return {"1": 1, "15": 15, "16": 16, "17": 17, "16W-1": 16 * w - 1, "16W": 16 * w, "16W+1": 16 * w + 1,
            "32W+5": 32 * w + 5, "S+1": DENSE + 1, "S+16": DENSE + 16, "S+16W": DENSE + 16 * w,
            "S+16W+1": DENSE + 16 * w + 1}[spec]


# 1. tile-count edges: a wave with no tile, exactly one, one wave with two, a ragged last tile; dense form alone and the
#    same remainders in the filtered form behind a full dense segment
@pytest.mark.parametrize("spec", ["1", "15", "16", "17", "16W-1", "16W", "16W+1", "32W+5", "S+1", "S+16", "S+16W", "S+16W+1"])
@pytest.mark.parametrize("D", [16, 768])
def test_stream_tile_count_edges(dev, D, spec):
    from evi_rag_amd import ops

    w = _w(dev)
    Q, k = 32, 10
    n_max = max(32 * w + 5, DENSE + 16 * w + 1)
    xn, qn, ref = _base(dev, D, Q, n_max)
    N = _rows(dev, spec)
    sc, ids = ops.cosine_topk(qn, xn[:N], k, row_id_base=1000)
    torch.cuda.synchronize()
    check_topk_against_scores(sc.cpu().numpy(), ids.cpu().numpy(), ref[:, :N], k, id_base=1000)
    m = min(k, N)
    assert np.array_equal(ids[1, :m].cpu().numpy(), np.arange(m) + 1000)


# 2. every load-group shape: one group (D = 16), two groups of one (32), odd group counts (48, 80), U = 2 (64), U = 4 with
#    two groups (128), U = 2 with six (192), and the 16-query passes of D = 1280
@pytest.mark.parametrize("D", [16, 32, 48, 80, 64, 128, 192, 1280])
def test_stream_every_load_group_shape(dev, D):
    from evi_rag_amd import ops

    Q, k = 17, 50
    N = DENSE + 16 * _w(dev) + 3
    x = _make_index(N, D, seed=N * 7 + D)
    q = _make_queries(Q, D, seed=Q + 13)
    xn = ops.normalize_embeddings(torch.from_numpy(x).to(dev), EPS)
    qn = ops.normalize_embeddings(torch.from_numpy(q).to(dev), EPS)
    sc, ids = ops.cosine_topk(qn, xn, k)
    torch.cuda.synchronize()
    check_topk_against_scores(sc.cpu().numpy(), ids.cpu().numpy(), ocos.cosine_scores(q, x, EPS), k)
    assert np.array_equal(ids[1].cpu().numpy(), np.arange(k))


def _check_long_list(sc, ids, ref, k):
    """check_topk_against_scores, query by query, on the columns that can matter: the returned ids and every row whose
    oracle score is within 1e-3 (500 x the helper's tie margin) of the oracle's k-th.  The helper sorts all N columns
    per query, seconds per call at a million rows; the columns left out are below every score it compares, and keeping
    the rest in id order keeps its order and tie rules what they are."""
    for r in range(ref.shape[0]):
        kth = np.partition(ref[r], -k)[-k]
        cols = np.union1d(np.flatnonzero(ref[r] >= kth - 1e-3), ids[r][ids[r] >= 0])
        pos = np.searchsorted(cols, ids[r])
        assert np.array_equal(cols[pos], ids[r]), f"q={r}: id out of range"
        check_topk_against_scores(sc[r:r + 1], pos[None, :], ref[r:r + 1, cols], k)


# 3. three segments (65 536 + 1 048 576 + the rest), pre-normalised rows and raw rows + row_scale
def test_stream_three_segments_with_and_without_row_scale(dev):
    from evi_rag_amd import ops

    D, Q, k = 16, 33, 500
    N = DENSE + DENSE * 16 + 16 * _w(dev) + 7
    x = _make_index(N, D, seed=N * 7 + D)
    q = _make_queries(Q, D, seed=Q + 13)
    xd = torch.from_numpy(x).to(dev)
    qn = ops.normalize_embeddings(torch.from_numpy(q).to(dev), EPS)
    ref = ocos.cosine_scores(q, x, EPS)
    sc, ids = ops.cosine_topk(qn, ops.normalize_embeddings(xd, EPS), k)
    _check_long_list(sc.cpu().numpy(), ids.cpu().numpy(), ref, k)
    sc2, ids2 = ops.cosine_topk(qn, xd, k, row_scale=ops.row_inv_norm(xd, EPS))
    _check_long_list(sc2.cpu().numpy(), ids2.cpu().numpy(), ref, k)
    assert np.array_equal(ids[1].cpu().numpy(), np.arange(k)) and np.array_equal(ids2[1].cpu().numpy(), np.arange(k))


# 4. every candidate passes: for query 0 each later row beats every earlier one, so the 4 096 rows behind the dense
#    segment all reach the threshold (256 per workgroup against 64 staging slots: LDS staging overflows into the global
#    append); for query 1 none does
def test_stream_every_candidate_passes(dev):
    from evi_rag_amd import ops

    N, D, k = DENSE + 4096, 16, 100
    base = np.zeros((N, D), dtype=np.float32)
    base[:, 0] = 1.0
    base[:, 1] = np.linspace(-1.0, 1.0, N, dtype=np.float32)  # cosine with e1 increases with the row id
    q = np.zeros((2, D), dtype=np.float32)
    q[0, 1] = 1.0
    q[1, 1] = -1.0
    xn = ops.normalize_embeddings(torch.from_numpy(base).to(dev), EPS)
    sc, ids = ops.cosine_topk(torch.from_numpy(q).to(dev), xn, k)
    check_topk_against_scores(sc.cpu().numpy(), ids.cpu().numpy(), ocos.cosine_scores(q, base, EPS), k)
    ids = ids.cpu().numpy()
    assert np.array_equal(ids[0], np.arange(N - 1, N - 1 - k, -1))
    assert np.array_equal(ids[1], np.arange(k))


# 5. the other kinds through the same template, each against the comparison its own test in test_cosine_topk_gpu.py uses
@pytest.mark.parametrize("D", [32, 64])
def test_stream_f16_index(dev, D):
    from evi_rag_amd import ops

    Q, k = 17, 50
    N = DENSE + 16 * _w(dev) + 1
    x = _make_index(N, D, seed=N + D)
    q = np.random.default_rng(Q).standard_normal((Q, D), dtype=np.float32)
    xn = ops.normalize_embeddings(torch.from_numpy(x).to(dev), EPS)
    qn = ops.normalize_embeddings(torch.from_numpy(q).to(dev), EPS)
    x16 = xn.to(torch.float16)
    sc, ids = ops.cosine_topk(qn, x16, k, row_id_base=7)
    ref_full = (qn.cpu().numpy().astype(np.float64) @ x16.cpu().numpy().astype(np.float64).T).astype(np.float32)
    check_topk_against_scores(sc.cpu().numpy(), ids.cpu().numpy(), ref_full, k, id_base=7, score_tol=2e-6)


@pytest.mark.parametrize("D", [64, 128])
def test_stream_fp8_widened_index(dev, D):
    from evi_rag_amd import ops

    Q, k = 17, 50
    N = DENSE + 16 * _w(dev) + 1
    x = _make_index(N, D, seed=N + D + 1)
    q = np.random.default_rng(Q + 2).standard_normal((Q, D), dtype=np.float32)
    xn = ops.normalize_embeddings(torch.from_numpy(x).to(dev), EPS)
    qn = ops.normalize_embeddings(torch.from_numpy(q).to(dev), EPS)
    codes, scale = ops.quantize_rows_fp8(xn)
    sc, ids = ops.cosine_topk(qn, codes, k, row_scale=scale, row_id_base=7, fp8_mfma=False)
    deq = ocos.e4m3_decode_table()[codes.cpu().numpy()].astype(np.float64)
    ref_full = ((qn.cpu().numpy().astype(np.float64) @ deq.T) * scale.cpu().numpy().astype(np.float64)).astype(np.float32)
    check_topk_against_scores(sc.cpu().numpy(), ids.cpu().numpy(), ref_full, k, id_base=7, score_tol=2e-6)


@pytest.mark.parametrize("D", [64, 128])
def test_stream_fp8_native_index(dev, D):
    """As test_cosine_topk_fp8_native_mfma_variant: scores within the two-piece bound 2^-8 max|q| sum|x_row| of the exact
    ones of the dequantised rows, sorted and unique, and differing from the widening variant only at near-ties."""
    from evi_rag_amd import ops

    Q, k = 17, 50
    N = DENSE + 16 * _w(dev) + 1
    x = _make_index(N, D, seed=N + D + 3)
    q = np.random.default_rng(Q + 5).standard_normal((Q, D), dtype=np.float32)
    q[0] *= 1e-3
    q[1] *= 1e4
    xn = ops.normalize_embeddings(torch.from_numpy(x).to(dev), EPS)
    qd = torch.from_numpy(q).to(dev)
    codes, scale = ops.quantize_rows_fp8(xn)
    sc, ids = ops.cosine_topk(qd, codes, k, row_scale=scale, row_id_base=7, fp8_mfma=True)
    sw, iw = ops.cosine_topk(qd, codes, k, row_scale=scale, row_id_base=7, fp8_mfma=False)
    deq = ocos.e4m3_decode_table()[codes.cpu().numpy()].astype(np.float64) * scale.cpu().numpy().astype(np.float64)[:, None]
    exact = q.astype(np.float64) @ deq.T
    bound = (2.0 ** -8) * np.abs(q).max(axis=1, keepdims=True) * np.abs(deq).sum(axis=1)[None, :]
    s_np, i_np = sc.cpu().numpy(), ids.cpu().numpy() - 7
    assert (i_np >= 0).all() and (i_np < N).all()
    for r in range(Q):
        row_ids = i_np[r]
        assert np.unique(row_ids).size == k
        err = np.abs(s_np[r].astype(np.float64) - exact[r, row_ids])
        assert (err <= bound[r, row_ids] + 1e-6 * np.abs(exact[r, row_ids]) + 1e-30).all(), (r, err.max())
        ds = np.diff(s_np[r])
        assert (ds <= 0).all() and (np.diff(row_ids)[ds == 0] > 0).all()
        kth = np.sort(exact[r])[::-1][k - 1]
        for rid in np.setdiff1d(row_ids, iw[r].cpu().numpy() - 7):
            assert abs(exact[r, rid] - kth) <= 2 * bound[r, rid] + 1e-30, (r, rid)
    overlap = np.mean([len(np.intersect1d(i_np[r], iw[r].cpu().numpy() - 7)) / k for r in range(Q)])
    assert overlap >= 0.97, overlap


# 6. the selection of the dense first segment.  One workgroup per query does it today, so there are no slices in the code;
#    a split over 8 192-row slices was measured slower and left out, and this pins the contract such a split must keep:
#    ties whose members lie in different 8 192-row slices of the segment (the
#    best rows of query 0 are copies of one row, one per slice and two more straddling a slice border), one query whose
#    scores are all equal, k from 1 to the maximum; ids in the documented order (score descending, then id ascending)
@pytest.mark.parametrize("k", [1, 500, 2048])
@pytest.mark.parametrize("N", [DENSE, 70000])
def test_dense_segment_selection_with_ties_across_slices(dev, N, k):
    from evi_rag_amd import ops

    D, Q = 16, 5
    x = _make_index(N, D, seed=N * 7 + D)
    q = _make_queries(Q, D, seed=Q + 13)
    slice_rows = 8192
    copies = [3 + s * slice_rows for s in range(DENSE // slice_rows)] + [slice_rows - 1, slice_rows, 5 * slice_rows - 1]
    x[copies] = q[0]  # cosine 1 with query 0: the top of its list is these rows in id order
    for s in range(1, DENSE // slice_rows):  # and a second family of equal rows further down the list, one per slice
        x[s * slice_rows + 100] = x[100]
    xn = ops.normalize_embeddings(torch.from_numpy(x).to(dev), EPS)
    qn = ops.normalize_embeddings(torch.from_numpy(q).to(dev), EPS)
    sc, ids = ops.cosine_topk(qn, xn, k)
    torch.cuda.synchronize()
    check_topk_against_scores(sc.cpu().numpy(), ids.cpu().numpy(), ocos.cosine_scores(q, x, EPS), k)
    ids = ids.cpu().numpy()
    top = min(k, len(copies))
    assert np.array_equal(ids[0, :top], np.sort(copies)[:top])
    assert np.array_equal(ids[1], np.arange(k))  # the all-equal (zero) query: pure id order
