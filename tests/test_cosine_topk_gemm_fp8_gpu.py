"""Many-query (GEMM-shaped) top-k over an e4m3 index: bit-for-bit equal to the scan of the same variant, refusals, the norm
guard, argument errors, and the selection error measured against the derived bound."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _data(Q, N, D, seed):
    """(queries, e4m3 codes, row_scale) on the GPU: N(0,1) rows, row 0 all-zero, 1 % duplicated rows, normalised, then
    quantised.  Made once per shape and never modified."""
    from evi_rag_amd import ops

    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(seed)
    x = torch.randn((N, D), device=dev, generator=g)
    x[0] = 0.0
    ndup = N // 100
    if ndup > 0 and N > 2:
        src = torch.randint(1, N, (ndup,), device=dev, generator=g)
        dst = torch.randint(1, N, (ndup,), device=dev, generator=g)
        x[dst] = x[src]
    q = torch.randn((Q, D), device=dev, generator=g)
    codes, scale = ops.quantize_rows_fp8(ops.normalize_embeddings(x))
    return ops.normalize_embeddings(q), codes, scale


@pytest.mark.parametrize("fp8_mfma", [False, True])
@pytest.mark.parametrize(
    "Q,N,D,k",
    [
        (256, 200000, 768, 500),  # several slabs: the filter-epilogue form runs; 12 chunks
        (100, 20000, 64, 40),     # one 64-byte chunk per row
        (96, 2000, 192, 10),      # three chunks; kk = 266: a partly filled last candidate tile; N below the first slab
        (96, 200, 192, 10),       # N < kk: count-limited lists
        (33, 1200, 128, 10),      # Q not a multiple of 16 or 32
    ],
)
def test_gemm_fp8_equals_scan_bit_for_bit(dev, Q, N, D, k, fp8_mfma):
    from evi_rag_amd import ops

    qn, codes, scale = _data(Q, N, D, N + D)
    s0, i0 = ops.cosine_topk(qn, codes, k, row_scale=scale, row_id_base=3, method="scan", fp8_mfma=fp8_mfma)
    s1, i1 = ops.cosine_topk_gemm(qn, codes, k, row_scale=scale, row_id_base=3, fallback=False, fp8_mfma=fp8_mfma)
    assert ops.cosine_topk_gemm.last_products == 3
    assert torch.equal(i0, i1)
    assert torch.equal(s0, s1)
    s2, i2 = ops.cosine_topk(qn, codes, k, row_scale=scale, row_id_base=3, method="gemm", fp8_mfma=fp8_mfma)
    assert ops.cosine_topk.last_method == "gemm"
    assert ops.cosine_topk_gemm.last_products == 3  # not the scan behind a failed proof
    assert torch.equal(i0, i2)
    assert torch.equal(s0, s2)


def test_gemm_fp8_refuses_ties(dev):
    from evi_rag_amd import ops

    g = torch.Generator(device=dev).manual_seed(5)
    row = ops.normalize_embeddings(torch.randn((1, 64), device=dev, generator=g))
    codes, scale = ops.quantize_rows_fp8(row.repeat(5000, 1))
    qn = ops.normalize_embeddings(torch.randn((40, 64), device=dev, generator=g))
    with pytest.raises(RuntimeError, match="could not prove"):
        ops.cosine_topk_gemm(qn, codes, 50, row_scale=scale, fallback=False)
    s0, i0 = ops.cosine_topk(qn, codes, 50, row_scale=scale, method="scan")
    s1, i1 = ops.cosine_topk_gemm(qn, codes, 50, row_scale=scale)
    assert ops.cosine_topk_gemm.last_products == 0
    assert torch.equal(i0, i1) and torch.equal(s0, s1)


def test_gemm_fp8_norm_guard(dev):
    from evi_rag_amd import ops

    qn, codes, scale = _data(96, 2000, 192, 2000 + 192)
    codes = codes.clone()  # a tensor of this test's own: the verdict is cached on it
    long_scale = scale * 2.0  # stored rows of norm ~ 2
    assert not ops.rows_are_unit_norm(codes, long_scale)
    with pytest.raises(ValueError, match="rows of norm <= 1"):
        ops.cosine_topk_gemm(qn, codes, 10, row_scale=long_scale, fallback=False)
    s0, i0 = ops.cosine_topk(qn, codes, 10, row_scale=long_scale, method="scan")
    s1, i1 = ops.cosine_topk_gemm(qn, codes, 10, row_scale=long_scale)
    assert ops.cosine_topk_gemm.last_products == 0
    assert torch.equal(i0, i1) and torch.equal(s0, s1)
    long_scale.mul_(0.5)  # in place, back to the true scales: the cached verdict must not survive
    assert ops.rows_are_unit_norm(codes, long_scale)
    s2, i2 = ops.cosine_topk_gemm(qn, codes, 10, row_scale=long_scale, fallback=False)
    assert ops.cosine_topk_gemm.last_products == 3
    s3, i3 = ops.cosine_topk(qn, codes, 10, row_scale=scale, method="scan")
    assert torch.equal(i2, i3) and torch.equal(s2, s3)


def test_gemm_fp8_argument_errors(dev):
    from evi_rag_amd import ops

    qn, codes, scale = _data(33, 1200, 128, 1200 + 128)
    with pytest.raises(ValueError, match="row_scale"):
        ops.cosine_topk_gemm(qn, codes, 10)
    with pytest.raises(ValueError, match="products"):
        ops.cosine_topk_gemm(qn, codes, 10, row_scale=scale, products=1)
    with pytest.raises(ValueError, match="shadow"):
        ops.cosine_topk_gemm(qn, codes, 10, row_scale=scale, shadow=torch.empty(codes.shape, dtype=torch.bfloat16, device=dev))
    with pytest.raises(NotImplementedError, match="multiple of 64"):  # D = 96
        ops.cosine_topk_gemm(qn[:, :96], codes[:, :96].contiguous(), 10, row_scale=scale * 0.5)
    with pytest.raises(NotImplementedError, match="exceeds"):  # k + reserve > 2048, as the f32 path
        ops.cosine_topk_gemm(qn, codes, 1400, row_scale=scale)


@pytest.mark.parametrize("fp8_mfma", [False, True])
def test_gemm_fp8_selection_error_is_inside_the_bound(dev, fp8_mfma):
    """Selection scores against the scan's, row by row, at Q = 96, N = 20000, D = 256: max |delta| <= eps |q| max|row| with
    eps = GEMM_FP8_EPS_UNIT, the constant derived in cosine_topk.hip (kApproxEpsFp8Unit)."""
    from evi_rag_amd import ops

    Q, N, D, step = 96, 20000, 256, 2000
    qn, codes, scale = _data(Q, N, D, N + D)
    sel = ops.cosine_topk_gemm_fp8_selection_scores(qn, codes, scale, fp8_mfma=fp8_mfma)  # [N, Q]
    scan = torch.empty((Q, N), dtype=torch.float32, device=dev)
    for lo in range(0, N, step):  # the scan's score of EVERY row: top-`step` of slices of `step` rows (k <= 2048)
        s, i = ops.cosine_topk(qn, codes[lo: lo + step], step, row_scale=scale[lo: lo + step], method="scan", fp8_mfma=fp8_mfma)
        assert bool((i >= 0).all())
        scan[:, lo: lo + step].scatter_(1, i, s)
    row_norm = codes.view(torch.float8_e4m3fn).float().norm(dim=1) * scale
    max_row_norm = float(row_norm.max())
    assert 1.0 <= max_row_norm <= ops.GEMM_FP8_ROW_NORM_MAX
    delta = (sel.t() - scan).abs().max(dim=1).values  # per query
    bound = ops.GEMM_FP8_EPS_UNIT * qn.norm(dim=1) * max_row_norm
    print(f"fp8_mfma={fp8_mfma}: max |selection - scan| = {float(delta.max()):.3e}, bound {float(bound.min()):.3e}, "
          f"largest stored-row norm {max_row_norm:.4f}")
    assert bool((delta <= bound).all())
