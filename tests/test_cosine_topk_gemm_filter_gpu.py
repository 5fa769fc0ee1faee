"""Row labels and per-query allow-sets in the GEMM-shaped many-query pass (GPU).

The yardstick is the UNFILTERED scan on the compacted index, never the filtered pass itself:
`cosine_topk_gemm(q, x, k, row_mask=m)` must equal `cosine_topk(q, x[m], k, method="scan")` with the ids mapped through
`nonzero(m)`, ids by torch.equal and scores as int32 bit patterns.

N = 40 003 rows are three slabs of the pass: 4 096 rows whose scores are stored and appended by k_gt_filter, 32 768 rows
through the threshold epilogue of the GEMM, and a ragged slab of 3 139 rows whose last 256-row tile holds 67.  Q = 300 is
two 256-column tiles, the second ragged.  Rows and queries are unit-normalised N(0, 1) draws without a zero query or a
duplicated row: the smallest (k-th - kk-th visible score) over the queries, computed in float64 for these shapes, k in
{10, 50}, both reserves and visible fractions 1, 0.5 and 0.1, is >= 0.045, more than five times the widest requirement
(0.0084, single product).  So every case that is not a fallback case must PROVE (status 0, last_products in (1, 3)): a
silent fallback to the scan cannot hide a broken pass."""
import functools
import time

import numpy as np
import pytest
import torch
import torch.distributed as dist

pytestmark = pytest.mark.gpu

EPS = 1e-6
N, D = 40003, 64
FIRST, SECOND_END = 4096, 4096 + 32768       # slab boundaries of the pass at this N
LAST_TILE = SECOND_END + (N - SECOND_END) // 256 * 256  # first row of the ragged last 256-row tile
DECOYS = (1000, 20000, LAST_TILE + 50)       # first slab, interior of the second, ragged last tile
KINDS = ("f32", "f16", "fp8_widen", "fp8_mfma")
MASKS = ("half", "tenth", "percent", "all", "none", "first_slab_hidden", "k_minus_1_late", "last_tile")
QK = ((5, 10), (5, 50), (300, 10), (300, 50))


def _raw(n, Q, seed):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((n, D), dtype=np.float32)
    q = rng.standard_normal((Q, D), dtype=np.float32)
    return q, x


@functools.lru_cache(maxsize=None)
def _base():
    """(queries [300, D], f32 index) on the device, unit rows.  Rows DECOYS are copies of queries 0, 1, 2: hidden by every
    mask but `all`, they score 1 and would win."""
    from evi_rag_amd import ops

    dev = torch.device("cuda:0")
    q, x = _raw(N, 300, seed=N + D)
    qn = ops.normalize_embeddings(torch.from_numpy(q).to(dev), EPS)
    xn = ops.normalize_embeddings(torch.from_numpy(x).to(dev), EPS)
    for j, row in enumerate(DECOYS):
        xn[row] = qn[j]
    return qn, xn


@functools.lru_cache(maxsize=None)
def _problem(kind):
    """(queries, index, row_scale, keywords) in one storage kind, built once per module run and never written to."""
    from evi_rag_amd import ops

    qn, xn = _base()
    if kind == "f32":
        return qn, xn, None, {}
    if kind == "f16":
        return qn, xn.half(), None, {}
    x8, scale = ops.quantize_rows_fp8(xn)
    return qn, x8, scale, {"fp8_mfma": kind == "fp8_mfma"}


def _mask(name, k, dev, n=N):
    g = torch.Generator(device="cpu").manual_seed(n + len(name))
    m = torch.zeros(n, dtype=torch.bool)
    if name == "half":
        m = torch.rand(n, generator=g) < 0.5
    elif name == "tenth":
        m = torch.rand(n, generator=g) < 0.1
    elif name == "percent":  # about 400 visible rows: fewer than kk = k + 1024 of the single-product selection
        m = torch.rand(n, generator=g) < 0.01
    elif name == "all":
        m[:] = True
    elif name == "first_slab_hidden":  # k_gt_filter appends nothing; the epilogue meets tau = -inf (a quarter of the rows
        m = torch.rand(n, generator=g) < 0.25  # behind it: about 8 200 in the second slab, inside the 16 384 slots)
        m[:FIRST] = False
    elif name == "k_minus_1_late":  # fewer than k visible rows, none in the first slab
        m[FIRST + torch.randperm(n - FIRST, generator=g)[: k - 1]] = True
    elif name == "last_tile":  # the ragged last tile only
        m[LAST_TILE:] = True
    if name != "all":
        m[list(DECOYS)] = False
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


def _assert_proven(kind, what):
    from evi_rag_amd import ops

    assert ops.cosine_topk_gemm.last_status == 0, f"{what}: status {ops.cosine_topk_gemm.last_status}, the scan produced the result"
    assert ops.cosine_topk_gemm.last_products in (1, 3), f"{what}: last_products {ops.cosine_topk_gemm.last_products}"
    if kind.startswith("fp8"):
        assert ops.cosine_topk_gemm.last_products == 3


@pytest.mark.parametrize("mask", MASKS)
@pytest.mark.parametrize("kind", KINDS)
def test_row_mask_equals_the_compacted_index(dev, kind, mask):
    from evi_rag_amd import ops

    q300, x, scale, kw = _problem(kind)
    for Q, k in QK:
        q = q300[:Q]
        m = _mask(mask, k, dev)
        want = _compacted(q, x, scale, k, m, **kw)
        plans = (None, 1, 3) if (Q == 300 and not kind.startswith("fp8")) else (None,)
        for products in plans:
            what = f"{kind} {mask} Q={Q} k={k} products={products}"
            ops.cosine_topk_gemm.last_status = ops.cosine_topk_gemm.last_products = None
            got = ops.cosine_topk_gemm(q, x, k, row_scale=scale, row_mask=m, products=products, **kw)
            _assert_proven(kind, what)
            if products is not None:
                assert ops.cosine_topk_gemm.last_products == products
            _assert_same(got, want, what)
            if mask == "all":
                _assert_same(got, ops.cosine_topk_gemm(q, x, k, row_scale=scale, products=products, **kw), what + " vs the plain call")
            else:
                assert not bool(torch.isin(got[1], (~m).nonzero().view(-1)).any()), f"{what}: a hidden row was returned"
            if mask == "none":
                assert bool((got[1] == -1).all()) and bool(torch.isneginf(got[0]).all())
            if mask == "k_minus_1_late":
                assert bool((got[1][:, : k - 1] >= 0).all()) and bool((got[1][:, k - 1:] == -1).all())


def test_the_bf16_shadow_selects_for_a_filtered_call(dev):
    from evi_rag_amd import ops

    q, x, _, _ = _problem("f32")
    shadow = ops.index_shadow_bf16(x)
    k = 50
    for mask in ("half", "percent"):
        m = _mask(mask, k, dev)
        want = _compacted(q, x, None, k, m)
        for products in (1, None):
            got = ops.cosine_topk_gemm(q, x, k, row_mask=m, products=products, shadow=shadow)
            assert ops.cosine_topk_gemm.last_status == 0 and ops.cosine_topk_gemm.last_products == 1
            _assert_same(got, want, f"shadow {mask} products={products}")


def _labels(dev, n=N):
    g = torch.Generator().manual_seed(11)
    labels = torch.tensor([0, 1, 2, 3, 31], dtype=torch.uint8)[torch.randint(0, 5, (n,), generator=g)]
    labels[::97] = 77  # a tombstone: matches no allow-set
    labels[list(DECOYS)] = 77
    return labels.to(dev)


SETS = (0b0011, 0b0100, 0b1111, 1 << 31, 0)


def _allow(Q, dtype, dev):
    vals = [SETS[i % len(SETS)] for i in range(Q)]
    if dtype == torch.int32:
        vals = [v - (1 << 32) if v >= (1 << 31) else v for v in vals]  # bit for bit: 1 << 31 is negative
    return torch.tensor(vals, dtype=dtype, device=dev)


def _compacted_labels(q, x, row_scale, k, labels, **kw):
    """The yardstick for labels: per allow-set of SETS, the unfiltered scan over the rows that set sees; query i takes its
    rows from the result of set i % len(SETS) (what _allow hands it)."""
    Q = q.size(0)
    s = torch.empty((Q, k), dtype=torch.float32, device=q.device)
    i = torch.empty((Q, k), dtype=torch.int64, device=q.device)
    for j, bits in enumerate(SETS):
        visible = torch.zeros(labels.numel(), dtype=torch.bool, device=q.device)
        for lab in range(32):
            if (bits >> lab) & 1:
                visible |= labels == lab
        want = _compacted(q, x, row_scale, k, visible, **kw)
        rows = torch.arange(j, Q, len(SETS), device=q.device)
        s[rows], i[rows] = want[0][rows], want[1][rows]
    return s, i


@pytest.mark.parametrize("kind", KINDS)
def test_labels_and_allow_sets(dev, kind):
    from evi_rag_amd import ops

    q, x, scale, kw = _problem(kind)
    Q, k = 300, 50
    labels = _labels(dev)
    got = ops.cosine_topk_gemm(q, x, k, row_scale=scale, row_labels=labels, query_allow=_allow(Q, torch.int64, dev), **kw)
    _assert_proven(kind, f"{kind} int64 allow-sets")
    got32 = ops.cosine_topk_gemm(q, x, k, row_scale=scale, row_labels=labels, query_allow=_allow(Q, torch.int32, dev), **kw)
    _assert_proven(kind, f"{kind} int32 allow-sets")
    _assert_same(got32, got, "int32 vs int64 allow-sets")
    want = _compacted_labels(q, x, scale, k, labels, **kw)
    for j, bits in enumerate(SETS):
        rows = torch.arange(j, Q, len(SETS), device=dev)
        _assert_same((got[0][rows], got[1][rows]), (want[0][rows], want[1][rows]), f"allow-set {bits:#x}")
    empty = torch.arange(len(SETS) - 1, Q, len(SETS), device=dev)
    assert bool((got[1][empty] == -1).all()) and bool(torch.isneginf(got[0][empty]).all()), "the empty allow-set sees no row"
    assert not bool(torch.isin(got[1], (labels >= 32).nonzero().view(-1)).any()), "a tombstone or a decoy row was returned"


def test_hidden_nan_rows_never_enter_a_list(dev):
    """A NaN score passes every threshold test (sc != sc): the label must stop it.  One hidden NaN row per slab; the lists
    then hold no NaN and the proof stands."""
    from evi_rag_amd import ops

    q, xn, _, _ = _problem("f32")
    x = xn.clone()
    k = 10
    m = _mask("half", k, dev)
    nan_rows = [7, 9000, N - 2]
    m[nan_rows] = False
    x[nan_rows] = float("nan")
    for Q in (5, 300):
        got = ops.cosine_topk_gemm(q[:Q], x, k, row_mask=m, check_norms=False)  # the norm check refuses a NaN norm
        _assert_proven("f32", f"hidden NaN rows, Q={Q}")
        _assert_same(got, _compacted(q[:Q], x, None, k, m), f"hidden NaN rows, Q={Q}")
        assert not bool(torch.isin(got[1], torch.tensor(nan_rows, device=dev)).any())


def test_a_zero_query_goes_to_the_filtered_scan(dev):
    from evi_rag_amd import ops

    qn, x, _, _ = _problem("f32")
    q = qn[:5].clone()
    q[2] = 0.0
    k = 10
    m = _mask("tenth", k, dev)  # the zero query's threshold is 0 and every score reaches it: a tenth of a slab fits its list
    got = ops.cosine_topk_gemm(q, x, k, row_mask=m)
    assert ops.cosine_topk_gemm.last_status == 1 and ops.cosine_topk_gemm.last_products == 0, "all scores of a zero query tie"
    _assert_same(got, _compacted(q, x, None, k, m), "zero query")


def test_tied_visible_rows_go_to_the_filtered_scan(dev):
    """600 copies of query 0 among the visible rows: they rank first for it and span the k-th and the kk-th = 306th kept
    score of the three-product selection, so there is no gap to prove."""
    from evi_rag_amd import ops

    q, xn, _, _ = _problem("f32")
    x = xn.clone()
    k = 50
    m = _mask("half", k, dev)
    rows = torch.randperm(N, generator=torch.Generator().manual_seed(5))[:600].to(dev)
    x[rows] = q[0]
    m[rows] = True
    got = ops.cosine_topk_gemm(q, x, k, row_mask=m, products=3)
    assert ops.cosine_topk_gemm.last_status == 1 and ops.cosine_topk_gemm.last_products == 0
    _assert_same(got, _compacted(q, x, None, k, m), "600 tied rows")
    assert bool(torch.isin(got[1][0], rows).all())


def test_a_hidden_prefix_overflows_and_goes_to_the_filtered_scan(dev):
    """60 000 rows, the first 36 864 (two slabs) hidden and the rest visible: the third slab meets tau = -inf with 23 136
    visible rows, more than the 16 384 slots of a list."""
    from evi_rag_amd import ops

    n, Q, k = 60000, 5, 10
    q, x = _raw(n, Q, seed=n + D)
    qn = ops.normalize_embeddings(torch.from_numpy(q).to(dev), EPS)
    xn = ops.normalize_embeddings(torch.from_numpy(x).to(dev), EPS)
    m = torch.zeros(n, dtype=torch.bool, device=dev)
    m[SECOND_END:] = True
    got = ops.cosine_topk_gemm(qn, xn, k, row_mask=m, products=3)
    assert ops.cosine_topk_gemm.last_status == 2 and ops.cosine_topk_gemm.last_products == 0
    _assert_same(got, _compacted(qn, xn, None, k, m), "hidden prefix")
    with pytest.raises(RuntimeError, match="status 2"):
        ops.cosine_topk_gemm(qn, xn, k, row_mask=m, products=3, fallback=False)


def test_row_id_base_and_caller_outputs(dev):
    from evi_rag_amd import ops

    q, x, _, _ = _problem("f32")
    Q, k = 300, 10
    for mask in ("half", "k_minus_1_late"):  # the second: (-inf, -1) slots stay unshifted
        m = _mask(mask, k, dev)
        want = _compacted(q, x, None, k, m)
        out = (torch.full((Q, k), 9.0, device=dev), torch.full((Q, k), 9, dtype=torch.int64, device=dev))
        got = ops.cosine_topk_gemm(q, x, k, row_mask=m, row_id_base=3, out=out)
        _assert_proven("f32", "row_id_base")
        assert got[0] is out[0] and got[1] is out[1]
        _assert_same(got, (want[0], torch.where(want[1] >= 0, want[1] + 3, want[1])), f"row_id_base = 3, {mask}")


def test_filtered_shards_merge_to_the_filtered_whole(dev):
    from evi_rag_amd import ops

    q, x, _, _ = _problem("f32")
    Q, k = 300, 50
    labels, allow = _labels(dev), _allow(Q, torch.int64, dev)
    whole = _compacted_labels(q, x, None, k, labels)
    cuts = [0, 13001, 30017, N]  # two unaligned boundaries
    parts = []
    for a, b in zip(cuts[:-1], cuts[1:]):
        parts.append(ops.cosine_topk_gemm(q, x[a:b], k, row_labels=labels[a:b], query_allow=allow, row_id_base=a))
        _assert_proven("f32", f"shard [{a}, {b})")
    merged = ops.topk_merge(torch.stack([p[0] for p in parts]), torch.stack([p[1] for p in parts]))
    _assert_same(merged, whole, "three shards")


def test_sharded_index_with_the_gemm_method(dev):
    from evi_rag_amd import ops
    from evi_rag_amd.dist import ShardedIndex

    q, x, _, _ = _problem("f32")
    Q, k = 300, 50
    labels, allow = _labels(dev), _allow(Q, torch.int32, dev)
    whole = _compacted_labels(q, x, None, k, labels)
    idx = ShardedIndex(x, N, row_labels=labels, method="gemm")
    _assert_same(idx.topk(q, k, query_allow=allow), whole, "topk")
    _assert_proven("f32", "ShardedIndex.topk")
    m = labels < 2
    _assert_same(ShardedIndex(x, N, row_mask=m, method="gemm").topk(q, k), _compacted(q, x, None, k, m), "row_mask")
    _assert_proven("f32", "ShardedIndex.topk, row_mask")


def _free_port():
    import socket

    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _wait(event, what, limit=60.0):
    """The step's own time limit: a lane that never finishes fails the test instead of hanging it."""
    deadline = time.monotonic() + limit
    while not event.query():
        assert time.monotonic() < deadline, f"{what}: not finished after {limit:.0f} s"
    event.synchronize()


def test_sharded_index_one_rank_exchange_with_the_gemm_method(dev, monkeypatch):
    from evi_rag_amd import ops
    from evi_rag_amd.dist import ShardedIndex

    q, x, _, _ = _problem("f32")
    Q, k = 300, 50
    labels, allow = _labels(dev), _allow(Q, torch.int32, dev)
    whole = _compacted_labels(q, x, None, k, labels)
    monkeypatch.setenv("EVI_FORCE_EXCHANGE", "1")
    dist.init_process_group("nccl", init_method=f"tcp://127.0.0.1:{_free_port()}", rank=0, world_size=1, device_id=dev)
    try:
        idx = ShardedIndex(x, N, row_labels=labels, method="gemm")
        assert idx._exchange
        _assert_same(idx.topk(q, k, query_allow=allow), whole, "topk")
        _assert_proven("f32", "packed exchange")
        assert idx.two_lanes
        for lane in range(2):  # one batch per pipeline lane
            s, i, ev = idx.topk_async(q, k, query_allow=allow)
            _wait(ev, f"lane {lane}")
            _assert_same((s, i), whole, f"lane {lane}")
            _assert_proven("f32", f"lane {lane}")
        idx.two_lanes = False  # one main stream + a side stream for the exchange
        s, i, ev = idx.topk_async(q, k, query_allow=allow)
        _wait(ev, "side stream")
        _assert_same((s, i), whole, "side stream")
        _assert_proven("f32", "side stream")
    finally:
        dist.destroy_process_group()
