"""Row labels and per-query allow-sets in the exact scans (GPU).

The yardstick is the UNFILTERED scan on the compacted index: `cosine_topk(q, x, k, row_mask=m)` must equal
`cosine_topk(q, x[m], k)` with the ids mapped through `nonzero(m)`, scores and ids bit for bit (a row's score does not
depend on where the row sits, and compaction keeps the id order, so ties break alike).  Scores are compared as int32
bit patterns, so NaN scores compare too."""
import functools

import numpy as np
import pytest
import torch
import torch.distributed as dist

from oracle import cosine as ocos
from tests.helpers import check_topk_against_scores

pytestmark = pytest.mark.gpu

EPS = 1e-6
DENSE = 65536  # rows of the dense first segment (default schedule)
KINDS = ("f32", "f16", "fp8_widen", "fp8_mfma")
MASKS = ("half", "percent", "all", "none", "dense_hidden", "k_minus_1_late", "last_tile")
SMALL, MID, LARGE = (5, 3000, 64, 10), (33, 70001, 64, 50), (17, 1200000, 64, 100)


def _raw(Q, N, D, seed):
    """_make_index of tests/test_cosine_topk_gpu.py (N(0,1) rows, row 0 zero, 1 % duplicated rows) plus queries, one of
    them zero."""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((N, D), dtype=np.float32)
    x[0] = 0.0
    ndup = int(N * 0.01)
    x[rng.integers(1, N, size=ndup)] = x[rng.integers(1, N, size=ndup)]
    q = rng.standard_normal((Q, D), dtype=np.float32)
    q[Q // 2] = 0.0
    return q, x


@functools.lru_cache(maxsize=3)
def _problem(shape, kind):
    """(queries, index, row_scale, scan keywords) of one shape in one storage kind, built once per module run."""
    from evi_rag_amd import ops

    Q, N, D, _ = shape
    dev = torch.device("cuda:0")
    q, x = _raw(Q, N, D, seed=N + D)
    qn = ops.normalize_embeddings(torch.from_numpy(q).to(dev), EPS)
    xn = ops.normalize_embeddings(torch.from_numpy(x).to(dev), EPS)
    if kind == "f32":
        return qn, xn, None, {}
    if kind == "f16":
        return qn, xn.half(), None, {}
    x8, scale = ops.quantize_rows_fp8(xn)
    return qn, x8, scale, {"fp8_mfma": kind == "fp8_mfma"}


def _mask(name, N, k, dev):
    g = torch.Generator(device="cpu").manual_seed(N + len(name))
    first = min(DENSE, N)
    m = torch.zeros(N, dtype=torch.bool)
    if name == "half":
        m = torch.rand(N, generator=g) < 0.5
    elif name == "percent":
        m = torch.rand(N, generator=g) < 0.01
    elif name == "all":
        m[:] = True
    elif name == "dense_hidden":  # the dense segment yields nothing
        m[first:] = True
    elif name == "k_minus_1_late":  # fewer than k visible rows, none in the dense segment (where the index has rows there)
        lo = first if N > first + k else N // 2
        m[lo + torch.randperm(N - lo, generator=g)[: k - 1]] = True
    elif name == "last_tile":  # the last (ragged where N % 16 != 0) tile only
        m[(N - 1) // 16 * 16:] = True
    return m.to(dev)


def _bits(s):
    return s.contiguous().view(torch.int32)


def _assert_same(got, want, what=""):
    assert torch.equal(got[1], want[1]), f"{what}: ids differ"
    assert torch.equal(_bits(got[0]), _bits(want[0])), f"{what}: score bits differ"


def _compacted(q, x, row_scale, k, visible, **kw):
    """The unfiltered scan over the visible rows only, ids mapped back through nonzero(visible)."""
    from evi_rag_amd import ops

    rows = visible.nonzero().view(-1)
    s, i = ops.cosine_topk(q, x[rows], k, row_scale=None if row_scale is None else row_scale[rows], method="scan", **kw)
    if rows.numel():
        i = torch.where(i >= 0, rows[i.clamp(min=0)], i)
    return s, i


@pytest.mark.parametrize("mask", MASKS)
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", [SMALL, MID], ids=["one_segment", "two_segments"])
def test_row_mask_equals_the_compacted_index(dev, shape, kind, mask):
    from evi_rag_amd import ops

    q, x, scale, kw = _problem(shape, kind)
    N, k = shape[1], shape[3]
    m = _mask(mask, N, k, dev)
    got = ops.cosine_topk(q, x, k, row_scale=scale, row_mask=m, method="scan", **kw)
    assert ops.cosine_topk.last_method == "scan"
    _assert_same(got, _compacted(q, x, scale, k, m, **kw), f"{kind} {mask}")
    if mask == "all":
        _assert_same(got, ops.cosine_topk(q, x, k, row_scale=scale, method="scan", **kw), "all true vs the plain call")
    if mask == "none":
        assert bool((got[1] == -1).all()) and bool(torch.isneginf(got[0]).all())
    if mask == "k_minus_1_late":
        assert bool((got[1][:, : k - 1] >= 0).all()) and bool((got[1][:, k - 1:] == -1).all())
    hidden = (~m).nonzero().view(-1)
    assert not bool(torch.isin(got[1], hidden).any()), "a hidden row was returned"


@pytest.mark.parametrize("mask", MASKS)
def test_row_mask_third_segment_f32(dev, mask):
    """1.2 M rows: segments of 65 536, 1 048 576 and the rest at the default schedule."""
    from evi_rag_amd import ops

    q, x, _, _ = _problem(LARGE, "f32")
    N, k = LARGE[1], LARGE[3]
    m = _mask(mask, N, k, dev)
    got = ops.cosine_topk(q, x, k, row_mask=m, method="scan")
    _assert_same(got, _compacted(q, x, None, k, m), mask)
    if mask == "all":
        _assert_same(got, ops.cosine_topk(q, x, k, method="scan"), "all true vs the plain call")


@pytest.mark.parametrize("kind", ["f32", "f16"])
def test_labels_and_allow_sets(dev, kind):
    from evi_rag_amd import ops

    q, x, _, _ = _problem(MID, kind)
    Q, N, _, k = MID
    g = torch.Generator(device="cpu").manual_seed(7)
    labels = torch.randint(0, 6, (N,), generator=g, dtype=torch.int64).to(torch.uint8)
    labels[torch.randperm(N, generator=g)[:700]] = 32   # one past the last label a set can hold
    labels[torch.randperm(N, generator=g)[:700]] = 200
    labels = labels.to(dev)
    sets = [0, 0xFFFFFFFF, 0b000101, 0b101010]
    allow = torch.tensor([sets[i % 4] for i in range(Q)], dtype=torch.int64, device=dev)
    got = ops.cosine_topk(q, x, k, row_labels=labels, query_allow=allow, method="scan")
    # int32 allow-sets are taken bit for bit
    allow32 = torch.tensor([s - (1 << 32) if s >= (1 << 31) else s for s in allow.tolist()], dtype=torch.int32, device=dev)
    _assert_same(ops.cosine_topk(q, x, k, row_labels=labels, query_allow=allow32, method="scan"), got, "int32 vs int64 allow-sets")
    for j, bits in enumerate(sets):
        visible = torch.zeros(N, dtype=torch.bool, device=dev)
        for lab in range(32):
            if (bits >> lab) & 1:
                visible |= labels == lab
        want = _compacted(q, x, None, k, visible)
        rows = torch.arange(j, Q, 4, device=dev)
        _assert_same((got[0][rows], got[1][rows]), (want[0][rows], want[1][rows]), f"allow-set {bits:#x}")
    assert bool((got[1][0::4] == -1).all()), "the empty allow-set sees no row"
    tomb = (labels >= 32).nonzero().view(-1)
    assert not bool(torch.isin(got[1], tomb).any()), "a row labelled 32 or 200 was returned"


def test_filtered_scan_against_the_cpu_oracle(dev):
    """Independent of the unfiltered scan: oracle.cosine.cosine_scores restricted to the visible columns."""
    from evi_rag_amd import ops

    Q, N, D, k = MID
    q, x = _raw(Q, N, D, seed=N + D)  # what _problem normalised
    qn, xn, _, _ = _problem(MID, "f32")
    m = _mask("half", N, k, dev)
    s, i = ops.cosine_topk(qn, xn, k, row_mask=m, method="scan")
    mh = m.cpu().numpy()
    pos = np.cumsum(mh) - 1  # row id -> column of the restricted score matrix
    ids = i.cpu().numpy()
    assert mh[ids].all(), "a hidden row was returned"
    check_topk_against_scores(s.cpu().numpy(), pos[ids], ocos.cosine_scores(q, x, EPS)[:, mh], k)


def test_nan_rows_and_a_nan_query(dev):
    from evi_rag_amd import ops

    Q, N, D, k = MID
    qn, xn, _, _ = _problem(MID, "f32")
    q, x = qn.clone(), xn.clone()
    m = _mask("half", N, k, dev)
    hidden_nan, visible_nan = [100, DENSE + 500], [200, DENSE + 700]  # one of each per segment
    m[hidden_nan] = False
    m[visible_nan] = True
    x[hidden_nan + visible_nan] = float("nan")
    q[3] = float("nan")
    got = ops.cosine_topk(q, x, k, row_mask=m, method="scan")
    _assert_same(got, _compacted(q, x, None, k, m), "NaN rows")
    bad = torch.tensor(hidden_nan, device=dev)
    assert not bool(torch.isin(got[1], bad).any()), "a hidden NaN row was returned"
    assert bool(torch.isin(torch.tensor(visible_nan, device=dev), got[1][0]).all()), "a visible NaN row ranks first"
    # fewer than k visible rows so far (threshold still -inf) when the hidden NaN row of the second segment goes by
    few = torch.zeros(N, dtype=torch.bool, device=dev)
    few[[5, 6, visible_nan[1], N - 1]] = True
    got = ops.cosine_topk(q, x, k, row_mask=few, method="scan")
    _assert_same(got, _compacted(q, x, None, k, few), "NaN rows, threshold at -inf")
    assert not bool(torch.isin(got[1], bad).any())


def test_two_stage_equals_the_filtered_scan(dev):
    from evi_rag_amd import ops

    Q, N, D, k = 32, MID[1], MID[2], MID[3]
    qn, xn, _, _ = _problem(MID, "f32")
    qn = qn[:Q]
    shadow = ops.index_shadow_f16(xn, attach=False)
    half = _mask("half", N, k, dev)
    few = torch.zeros(N, dtype=torch.bool, device=dev)  # fewer than kk = k + 256 visible rows, on both sides of row 65 536
    few[torch.randperm(N, generator=torch.Generator().manual_seed(3))[:100].to(dev)] = True
    few[[DENSE - 1, DENSE, N - 1]] = True
    for name, m in (("half", half), ("few", few)):
        want = ops.cosine_topk(qn, xn, k, row_mask=m, method="scan", row_id_base=7)
        for fb in ("device", "host"):
            _assert_same(ops.cosine_topk_two_stage(qn, xn, shadow, k, row_mask=m, row_id_base=7, fallback=fb), want, f"{name} {fb}")
    # labels through the two-stage scan
    labels = (torch.arange(N, device=dev) % 5).to(torch.uint8)
    allow = torch.tensor([(1 << (i % 5)) | 1 for i in range(Q)], dtype=torch.int32, device=dev)
    _assert_same(ops.cosine_topk_two_stage(qn, xn, shadow, k, row_labels=labels, query_allow=allow),
                 ops.cosine_topk(qn, xn, k, row_labels=labels, query_allow=allow, method="scan"), "labels")


def test_two_stage_failed_proof_falls_back_on_the_device(dev):
    """The visible rows are 600 copies of one row: no gap between the k-th and the kk-th shadow score, the proof fails, the
    status word says so and the gated f32 scan (filtered too) repairs the result on the device."""
    from evi_rag_amd import ops

    Q, N, D, k = 32, MID[1], MID[2], MID[3]
    qn, xn, _, _ = _problem(MID, "f32")
    qn = qn[:Q]
    x = xn.clone()
    rows = torch.randperm(N, generator=torch.Generator().manual_seed(5))[:600].to(dev)
    x[rows] = x[12345].clone()
    m = torch.zeros(N, dtype=torch.bool, device=dev)
    m[rows] = True
    shadow = ops.index_shadow_f16(x, attach=False)
    want = ops.cosine_topk(qn, x, k, row_mask=m, method="scan")
    flag = torch.zeros(1, dtype=torch.int32, device=dev)
    got = ops.cosine_topk_two_stage(qn, x, shadow, k, row_mask=m, status=flag)
    assert int(flag.item()) == 1, "600 tied rows cannot be proven"
    _assert_same(got, want, "device-side fallback")
    assert bool(m[got[1].clamp(min=0)].all())


def test_auto_routing_with_a_filter(dev):
    from evi_rag_amd import ops

    Q, N, D, k = SMALL
    qn, xn, _, _ = _problem(SMALL, "f32")
    x = xn.clone()  # a tensor of its own: the shadow is attached to it
    m = _mask("half", N, k, dev)
    want = ops.cosine_topk(qn, x, k, row_mask=m)
    assert ops.cosine_topk.last_method == "scan"
    many = ops.normalize_embeddings(torch.randn(96, D, device=dev, generator=torch.Generator(device=dev).manual_seed(1)))
    ops.cosine_topk(many, x, k)
    assert ops.cosine_topk.last_method == "gemm"
    s96, i96 = ops.cosine_topk(many, x, k, row_mask=m)  # never the GEMM-shaped pass with a filter
    assert ops.cosine_topk.last_method == "scan"
    _assert_same((s96, i96), _compacted(many, x, None, k, m), "Q = 96")
    ops.index_shadow_f16(x)
    try:
        got = ops.cosine_topk(qn, x, k, row_mask=m)
        assert ops.cosine_topk.last_method == "two_stage"
        _assert_same(got, want, "auto, shadow resident")
        ops.cosine_topk(many, x, k, row_mask=m)
        assert ops.cosine_topk.last_method == "two_stage"
    finally:
        ops.drop_shadow_f16(x)


def _labelled_problem(dev):
    qn, xn, _, _ = _problem(MID, "f32")
    Q, N, _, k = MID
    labels = torch.randint(0, 4, (N,), generator=torch.Generator().manual_seed(11), dtype=torch.int64).to(torch.uint8).to(dev)
    labels[::97] = 77
    allow = torch.tensor([[0b0011, 0b0100, 0b1111][i % 3] for i in range(Q)], dtype=torch.int32, device=dev)
    return qn, xn, labels, allow, k


def test_filtered_shards_merge_to_the_filtered_whole(dev):
    from evi_rag_amd import ops

    qn, xn, labels, allow, k = _labelled_problem(dev)
    N = xn.size(0)
    whole = ops.cosine_topk(qn, xn, k, row_labels=labels, query_allow=allow, method="scan")
    cuts = [0, 20011, DENSE + 19, N]  # two unaligned boundaries
    parts = [ops.cosine_topk(qn, xn[a:b], k, row_labels=labels[a:b], query_allow=allow, row_id_base=a, method="scan")
             for a, b in zip(cuts[:-1], cuts[1:])]
    merged = ops.topk_merge(torch.stack([p[0] for p in parts]), torch.stack([p[1] for p in parts]))
    _assert_same(merged, whole, "three shards")


def _free_port():
    import socket

    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def test_filtered_sharded_index_one_rank_exchange(dev, monkeypatch):
    from evi_rag_amd import ops
    from evi_rag_amd.dist import ShardedIndex

    qn, xn, labels, allow, k = _labelled_problem(dev)
    N = xn.size(0)
    whole = ops.cosine_topk(qn, xn, k, row_labels=labels, query_allow=allow, method="scan")
    m = labels < 2
    whole_m = ops.cosine_topk(qn[:32], xn, k, row_mask=m, method="scan")
    monkeypatch.setenv("EVI_FORCE_EXCHANGE", "1")
    dist.init_process_group("nccl", init_method=f"tcp://127.0.0.1:{_free_port()}", rank=0, world_size=1, device_id=dev)
    try:
        idx = ShardedIndex(xn, N, row_labels=labels)
        assert idx._exchange
        _assert_same(idx.topk(qn, k, query_allow=allow), whole, "topk")
        assert idx.two_lanes
        for lane in range(2):  # one batch per pipeline lane
            s, i, ev = idx.topk_async(qn, k, query_allow=allow)
            ev.synchronize()
            _assert_same((s, i), whole, f"lane {lane}")
        idx.two_lanes = False  # one main stream + a side stream for the exchange
        s, i, ev = idx.topk_async(qn, k, query_allow=allow)
        ev.synchronize()
        _assert_same((s, i), whole, "side stream")
        ts = ShardedIndex(xn, N, row_mask=m, method="two_stage", shadow=ops.index_shadow_f16(xn, attach=False))
        _assert_same(ts.topk(qn[:32], k), whole_m, "two_stage topk")
        s, i, ev = ts.topk_async(qn[:32], k)
        ev.synchronize()
        _assert_same((s, i), whole_m, "two_stage lane")
    finally:
        dist.destroy_process_group()


def test_caller_buffers_with_a_filter(dev):
    from evi_rag_amd import _lib, ops

    qn, xn, labels, allow, k = _labelled_problem(dev)
    Q, N, D = qn.size(0), xn.size(0), xn.size(1)
    want = ops.cosine_topk(qn, xn, k, row_labels=labels, query_allow=allow, method="scan", row_id_base=3)
    lib = _lib.load()
    for nbytes in (lib.evi_cosine_topk_workspace_bytes(Q, N, D, k), lib.evi_cosine_topk_min_workspace_bytes(Q, N, D, k)):
        ws = torch.empty(int(nbytes), dtype=torch.uint8, device=dev)
        out = (torch.full((Q, k), 9.0, device=dev), torch.full((Q, k), 9, dtype=torch.int64, device=dev))
        got = ops.cosine_topk(qn, xn, k, row_labels=labels, query_allow=allow, method="scan", row_id_base=3, workspace=ws, out=out)
        assert got[0] is out[0] and got[1] is out[1]
        _assert_same(got, want, f"workspace of {nbytes} B")
    shadow = ops.index_shadow_f16(xn, attach=False)
    ws = torch.empty(int(lib.evi_cosine_topk_two_stage_workspace_bytes(32, N, D, k)), dtype=torch.uint8, device=dev)
    out = (torch.empty((32, k), device=dev), torch.empty((32, k), dtype=torch.int64, device=dev))
    got = ops.cosine_topk_two_stage(qn[:32], xn, shadow, k, row_labels=labels, query_allow=allow[:32], row_id_base=3, workspace=ws,
                                    out=out)
    assert got[0] is out[0]
    _assert_same(got, (want[0][:32], want[1][:32]), "two-stage, caller buffers")
