"""Exact top-k over per-query candidate id lists (GPU).

The yardstick is the UNFILTERED scan on the compacted index: query i of `cosine_topk_candidates` must equal
`cosine_topk(q[i:i+1], x[rows], k, method="scan")` with rows = sorted(unique(valid ids of list i)) and the ids mapped back
through `rows`, scores and ids bit for bit (a row's score does not depend on where the row sits, and compaction keeps the
id order, so ties break alike).  Scores are compared as int32 bit patterns, so NaN scores would compare too."""
import functools
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist

from oracle import cosine as ocos
from tests.helpers import check_topk_against_scores

pytestmark = pytest.mark.gpu

EPS = 1e-6
N, Q = 30000, 200
KINDS = {"f32": 48, "f32_wide": 272, "f16": 96, "fp8_widen": 192, "fp8_mfma": 192, "f32_raw_scale": 48}  # kind -> D
# list lengths around one scoring tile (16) and around block_topk's sorter limits (1024 for k <= 1024, 8192 above)
GRID = (0, 1, 15, 16, 17, 1023, 1024, 1025, 8192, 8193, 20000)
Q0 = Q // 2 - 5  # the GRID's queries are Q0 .. Q0 + 10: the zero query (Q // 2) is one of them


@functools.lru_cache(maxsize=None)
def _raw(D):
    """_make_index of tests/test_cosine_topk_gpu.py (N(0,1) rows, row 0 zero, 1 % duplicated rows) plus queries, one of
    them zero."""
    rng = np.random.default_rng(N + D)
    x = rng.standard_normal((N, D), dtype=np.float32)
    x[0] = 0.0
    ndup = int(N * 0.01)
    x[rng.integers(1, N, size=ndup)] = x[rng.integers(1, N, size=ndup)]
    q = rng.standard_normal((Q, D), dtype=np.float32)
    q[Q // 2] = 0.0
    return q, x


@functools.lru_cache(maxsize=None)
def _problem(kind):
    """(queries, index, row_scale, fp8 keywords) in one storage kind, built once per module run."""
    from evi_rag_amd import ops

    dev = torch.device("cuda:0")
    q, x = _raw(KINDS[kind])
    qn = ops.normalize_embeddings(torch.from_numpy(q).to(dev), EPS)
    if kind == "f32_raw_scale":
        xr = torch.from_numpy(x).to(dev)
        return qn, xr, ops.row_inv_norm(xr, EPS), {}
    xn = ops.normalize_embeddings(torch.from_numpy(x).to(dev), EPS)
    if kind in ("f32", "f32_wide"):
        return qn, xn, None, {}
    if kind == "f16":
        return qn, xn.half(), None, {}
    x8, scale = ops.quantize_rows_fp8(xn)
    return qn, x8, scale, {"fp8_mfma": kind == "fp8_mfma"}


def _bits(s):
    return s.contiguous().view(torch.int32)


def _assert_same(got, want, what=""):
    assert torch.equal(got[1], want[1]), f"{what}: ids differ"
    assert torch.equal(_bits(got[0]), _bits(want[0])), f"{what}: score bits differ"


def _pack(lists, dev):
    """(cand_ids [T] i64, cand_ptr [Q + 1] i64) of a list of 1-D id tensors."""
    ptr = torch.zeros(len(lists) + 1, dtype=torch.int64)
    ptr[1:] = torch.cumsum(torch.tensor([int(L.numel()) for L in lists]), 0)
    ids = torch.cat([L.to(torch.int64).view(-1) for L in lists]) if lists else torch.zeros(0, dtype=torch.int64)
    return ids.to(dev), ptr.to(dev)


def _reference(q, x, scale, lists, k, kw, base=0, limit=None):
    """Per query: the unfiltered scan over the compacted index of its distinct valid rows, ids mapped back."""
    from evi_rag_amd import ops

    n = x.shape[0]
    limit = base + n if limit is None else limit
    S, I = [], []
    for i, L in enumerate(lists):
        L = L.to(q.device).to(torch.int64)
        rows = torch.unique(L[(L >= base) & (L < base + n) & (L < limit) & (L >= 0)]) - base
        s, ids = ops.cosine_topk(q[i:i + 1], x[rows], k, row_scale=None if scale is None else scale[rows], method="scan", **kw)
        if rows.numel():
            ids = torch.where(ids >= 0, rows[ids.clamp(min=0)] + base, ids)
        S.append(s)
        I.append(ids)
    return torch.cat(S), torch.cat(I)


def _grid_lists(seed=1):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return [torch.randperm(N, generator=g)[:n] for n in GRID]


def _run(kind, lists, k, q_rows=None, **kwargs):
    from evi_rag_amd import ops

    q, x, scale, kw = _problem(kind)
    qs = q[:len(lists)] if q_rows is None else q[q_rows]
    ids, ptr = _pack(lists, q.device)
    status = torch.zeros(1, dtype=torch.int32, device=q.device)
    got = ops.cosine_topk_candidates(qs, x, ids, k, cand_ptr=ptr, row_scale=scale, status=status, **kw, **kwargs)
    return got, status, (qs, x, scale, kw)


@pytest.mark.parametrize("k", [1, 10, 500, 1500])
@pytest.mark.parametrize("kind", list(KINDS))
def test_length_grid_equals_the_compacted_scan(dev, kind, k):
    lists = _grid_lists()
    got, status, (qs, x, scale, kw) = _run(kind, lists, k, q_rows=slice(Q0, Q0 + len(GRID)))
    _assert_same(got, _reference(qs, x, scale, lists, k, kw), f"{kind} k={k}")
    assert int(status.item()) == 0
    for i, n in enumerate(GRID):  # padding past the list (the ids of a list here are distinct)
        real = min(n, k)
        assert bool((got[1][i, :real] >= 0).all()) and bool((got[1][i, real:] == -1).all()), (i, n)
        assert bool(torch.isneginf(got[0][i, real:]).all())
        assert bool(torch.isin(got[1][i, :real], lists[i].to(dev)).all()), "a row that is not listed was returned"


@pytest.mark.parametrize("kind", ["f32", "f32_wide", "f16", "fp8_mfma"])
def test_short_lists_straddle_the_scoring_tiles(dev, kind):
    """Q = 200 lists of 3 .. 40 entries: most scoring tiles are ragged, the tile prefix spans more than 32 queries."""
    g = torch.Generator(device="cpu").manual_seed(3)
    lens = torch.randint(3, 41, (Q,), generator=g).tolist()
    lists = [torch.randint(0, N, (n,), generator=g) for n in lens]
    got, status, (qs, x, scale, kw) = _run(kind, lists, 10)
    _assert_same(got, _reference(qs, x, scale, lists, 10, kw), kind)
    assert int(status.item()) == 0


def _duplicate_lists():
    g = torch.Generator(device="cpu").manual_seed(5)
    five = torch.tensor([7, 29999, 0, 12345, 16])
    pool = torch.randperm(N, generator=g)[:400]
    distinct = torch.randperm(N - 1, generator=g)[:500] + 1
    with_zero = torch.cat([distinct, torch.zeros(300, dtype=torch.int64)])
    return [five[torch.randint(0, 5, (20000,), generator=g)],           # > kSortCap entries, 5 distinct rows
            torch.full((20000,), 4321, dtype=torch.int64),               # one id
            pool[torch.randint(0, 400, (4096,), generator=g)],           # relation-shaped: 90 % repeats
            with_zero[torch.randperm(with_zero.numel(), generator=g)]]   # id 0 (the zero row) 300 times among distinct ids


@pytest.mark.parametrize("k", [10, 1500])
@pytest.mark.parametrize("kind", ["f32", "fp8_widen"])
def test_repeated_ids_count_once(dev, kind, k):
    lists = _duplicate_lists()
    got, status, (qs, x, scale, kw) = _run(kind, lists, k)
    _assert_same(got, _reference(qs, x, scale, lists, k, kw), f"{kind} k={k}")
    assert [int(L.unique().numel()) for L in lists[:2]] == [5, 1]
    for i, L in enumerate(lists):
        real = min(int(L.unique().numel()), k)
        assert bool((got[1][i, :real] >= 0).all()) and bool((got[1][i, real:] == -1).all()), i
        assert bool(torch.isneginf(got[0][i, real:]).all()), i
        assert got[1][i, :real].unique().numel() == real, "a row was returned twice"
    if k == 10:
        assert got[1][0, :5].sort().values.tolist() == [0, 7, 16, 12345, 29999]
    # any permutation of a list gives the same bits
    g = torch.Generator(device="cpu").manual_seed(6)
    shuffled = [L[torch.randperm(L.numel(), generator=g)] for L in lists]
    _assert_same(_run(kind, shuffled, k)[0], got, "permuted lists")


def test_id_rules(dev):
    from evi_rag_amd import ops

    q, x, _, _ = _problem("f32")
    g = torch.Generator(device="cpu").manual_seed(8)
    lists = [torch.randint(0, N, (n,), generator=g) for n in (40, 0, 700, 17, 2000)]
    k = 50
    clean, status, _ = _run("f32", lists, k)
    assert int(status.item()) == 0
    _assert_same(clean, _reference(q[:5], x, None, lists, k, {}), "clean")

    def sprinkle(L, values):
        out = torch.cat([L, torch.tensor(values, dtype=torch.int64).repeat(3)])
        return out[torch.randperm(out.numel(), generator=g)]

    padded, status, _ = _run("f32", [sprinkle(L, [-1, -1, -7, -2 ** 40]) for L in lists], k)
    _assert_same(padded, clean, "-1 padding is ignored")
    assert int(status.item()) == 0
    over, status, _ = _run("f32", [sprinkle(L, [N, N + 5, 2 ** 40, -1]) for L in lists], k)
    _assert_same(over, clean, "ids >= id_limit are skipped")
    assert int(status.item()) == 1
    # a caller-given id_limit below N: rows at or beyond it are refused although the index has them
    low, status, _ = _run("f32", lists, k, id_limit=N // 2)
    _assert_same(low, _reference(q[:5], x, None, lists, k, {}, limit=N // 2), "id_limit below N")
    assert int(status.item()) == 1
    # int32 ids; the [Q, C] padded form
    ids, ptr = _pack(lists, dev)
    _assert_same(ops.cosine_topk_candidates(q[:5], x, ids.to(torch.int32), k, cand_ptr=ptr), clean, "int32 ids")
    C = max(int(L.numel()) for L in lists)
    table = torch.full((5, C), -1, dtype=torch.int64)
    for i, L in enumerate(lists):
        table[i, :L.numel()] = L
    _assert_same(ops.cosine_topk_candidates(q[:5], x, table.to(dev), k), clean, "[Q, C] padded form")
    # cand_ptr need not start at 0 nor end at T: a head and a tail that no query owns are never looked at
    ids2 = torch.cat([ids.new_full((9,), 123), ids, ids.new_full((5,), 77)])
    status.zero_()
    _assert_same(ops.cosine_topk_candidates(q[:5], x, ids2, k, cand_ptr=ptr + 9, status=status), clean, "head and tail")
    assert int(status.item()) == 0


@pytest.mark.parametrize("ptr", [[0, 40, 30, 700, 757, 2757], [0, 40, 40, 740, 757, 99999], [-5, 40, 40, 740, 757, 2757],
                                 [2 ** 40, 40, 40, 740, 757, 2757]], ids=["non_monotone", "past_T", "negative", "huge"])
def test_malformed_cand_ptr_sets_bit_2_and_answers_nothing(dev, ptr):
    """A host-constructed malformed argument, refused by the kernels' own bounds logic: bit 2, every list empty."""
    from evi_rag_amd import ops

    q, x, _, _ = _problem("f32")
    g = torch.Generator(device="cpu").manual_seed(9)
    ids = torch.randint(0, N, (2757,), generator=g).to(dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    s, i = ops.cosine_topk_candidates(q[:5], x, ids, 20, cand_ptr=torch.tensor(ptr, dtype=torch.int64, device=dev), status=status)
    torch.cuda.synchronize(dev)
    assert int(status.item()) & 2
    assert bool((i == -1).all()) and bool(torch.isneginf(s).all())


def test_empty_shapes(dev):
    from evi_rag_amd import ops

    q, x, _, _ = _problem("f32")
    D = x.shape[1]
    ptr0 = torch.zeros(1, dtype=torch.int64, device=dev)
    none = torch.zeros(0, dtype=torch.int64, device=dev)
    s, i = ops.cosine_topk_candidates(q[:0], x, none, 7, cand_ptr=ptr0)
    assert s.shape == (0, 7) and i.shape == (0, 7) and s.dtype == torch.float32 and i.dtype == torch.int64
    s, i = ops.cosine_topk_candidates(q[:0], x, torch.zeros((0, 4), dtype=torch.int64, device=dev), 7)
    assert s.shape == (0, 7) and i.shape == (0, 7)
    for cand, kw in ((none, dict(cand_ptr=torch.zeros(4, dtype=torch.int64, device=dev))),        # T == 0
                     (torch.zeros((3, 0), dtype=torch.int64, device=dev), {})):                    # [Q, 0]
        s, i = ops.cosine_topk_candidates(q[:3], x, cand, 7, **kw)
        assert bool((i == -1).all()) and bool(torch.isneginf(s).all()) and i.shape == (3, 7)
    # N == 0: every id belongs to another shard (or is past the default id_limit = row_id_base + 0)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    s, i = ops.cosine_topk_candidates(q[:3], x[:0], torch.arange(12, device=dev).view(3, 4), 7, id_limit=N, status=status)
    assert bool((i == -1).all()) and bool(torch.isneginf(s).all()) and int(status.item()) == 0
    assert x[:0].shape == (0, D)


def test_results_pass_the_oracle_check(dev):
    """Not only HIP against HIP: every query's result against oracle.cosine.cosine_scores restricted to its distinct ids,
    with check_topk_against_scores' default tolerances (those of tests/test_cosine_topk_gpu.py for the same data)."""
    q_raw, x_raw = _raw(KINDS["f32"])
    lists = _grid_lists()
    for k in (10, 1500):
        (s, ids), _, _ = _run("f32", lists, k, q_rows=slice(Q0, Q0 + len(GRID)))
        s, ids = s.cpu().numpy(), ids.cpu().numpy()
        for i, L in enumerate(lists):
            rows = np.unique(L.numpy())
            if rows.size == 0:
                assert np.all(ids[i] == -1) and np.all(np.isneginf(s[i]))
                continue
            ref = ocos.cosine_scores(q_raw[Q0 + i:Q0 + i + 1], x_raw[rows], EPS)
            real = ids[i] >= 0
            assert np.all(np.isin(ids[i][real], rows))
            local = np.where(real, np.searchsorted(rows, np.where(real, ids[i], rows[0])), -1)
            check_topk_against_scores(s[i:i + 1], local[None, :], ref, k)


def test_three_row_shards_merge_to_the_single_call(dev):
    from evi_rag_amd import ops

    q, x, scale, kw = _problem("fp8_mfma")
    lists = _grid_lists(seed=11)
    ids, ptr = _pack(lists, dev)
    qs = q[Q0:Q0 + len(GRID)]
    k = 500
    whole = ops.cosine_topk_candidates(qs, x, ids, k, cand_ptr=ptr, row_scale=scale, **kw)
    bounds = (0, 9000, 21001, N)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    parts = [ops.cosine_topk_candidates(qs, x[a:b], ids, k, cand_ptr=ptr, row_scale=scale[a:b], row_id_base=a, id_limit=N,
                                        status=status, **kw) for a, b in zip(bounds, bounds[1:])]
    assert int(status.item()) == 0, "a row of another shard is skipped silently"
    merged = ops.topk_merge(torch.stack([p[0] for p in parts]), torch.stack([p[1] for p in parts]))
    _assert_same(merged, whole, "3 shards")
    for (a, b), (_, pi) in zip(zip(bounds, bounds[1:]), parts):
        assert bool(((pi == -1) | ((pi >= a) & (pi < b))).all())


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def test_sharded_index_world_size_one_and_one_rank_exchange(dev, monkeypatch):
    """More than one real rank is not covered here."""
    from evi_rag_amd import ops
    from evi_rag_amd.dist import ShardedIndex

    k = 100
    lists = _grid_lists(seed=12)
    ids, ptr = _pack(lists, dev)
    C = 64
    table = torch.stack([L[:C] for L in lists if L.numel() >= C]).to(dev)
    for kind in ("f32", "fp8_mfma"):
        q, x, scale, kw = _problem(kind)
        qs = q[Q0:Q0 + len(GRID)]
        want = ops.cosine_topk_candidates(qs, x, ids, k, cand_ptr=ptr, row_scale=scale, **kw)
        want2 = ops.cosine_topk_candidates(qs[:table.size(0)], x, table, k, row_scale=scale, **kw)
        idx = ShardedIndex(x, N, row_scale=scale, fp8_mfma=bool(kw.get("fp8_mfma")))
        assert not idx._exchange
        _assert_same(idx.topk_candidates(qs, ids, k, cand_ptr=ptr), want, f"{kind} world 1")
        _assert_same(idx.topk_candidates(qs[:table.size(0)], table, k), want2, f"{kind} world 1 [Q, C]")
    monkeypatch.setenv("EVI_FORCE_EXCHANGE", "1")
    dist.init_process_group("nccl", init_method=f"tcp://127.0.0.1:{_free_port()}", rank=0, world_size=1, device_id=dev)
    try:
        idx = ShardedIndex(x, N, row_scale=scale, fp8_mfma=True)
        assert idx._exchange and idx._packed_ok
        _assert_same(idx.topk_candidates(qs, ids, k, cand_ptr=ptr), want, "one-rank exchange, packed record")
        idx = ShardedIndex(x, N, row_scale=scale, fp8_mfma=True, merge=lambda s, i: ops.topk_merge(s, i))
        assert idx._exchange and not idx._packed_ok
        _assert_same(idx.topk_candidates(qs, ids, k, cand_ptr=ptr), want, "one-rank exchange, custom merge")
    finally:
        dist.destroy_process_group()


def test_replays_in_a_graph_over_new_contents(dev):
    from evi_rag_amd import _lib, ops

    q, x, _, _ = _problem("f32")
    k = 100
    a, b = _grid_lists(seed=13), _grid_lists(seed=14)
    qa, qb = q[:len(GRID)], q[Q0:Q0 + len(GRID)]
    ids_a, ptr = _pack(a, dev)
    ids_b, _ = _pack(b, dev)
    ids_b[5:900:7] = ids_b[4]  # repeats: the distinct counts differ from a's, the shapes do not
    want_a = ops.cosine_topk_candidates(qa, x, ids_a, k, cand_ptr=ptr)
    want_b = ops.cosine_topk_candidates(qb, x, ids_b, k, cand_ptr=ptr)
    assert not torch.equal(want_a[1], want_b[1])
    q_static, ids_static = qa.clone(), ids_a.clone()
    ws = torch.empty(int(_lib.load().evi_cosine_topk_candidates_workspace_bytes(len(GRID), ids_a.numel(), k)), dtype=torch.uint8,
                     device=dev)
    out = (torch.empty((len(GRID), k), dtype=torch.float32, device=dev), torch.empty((len(GRID), k), dtype=torch.int64, device=dev))
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    stream = torch.cuda.Stream(device=dev)
    stream.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(stream):
        ops.cosine_topk_candidates(q_static, x, ids_static, k, cand_ptr=ptr, workspace=ws, out=out, status=status)  # warm-up
    torch.cuda.current_stream(dev).wait_stream(stream)
    torch.cuda.synchronize(dev)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ops.cosine_topk_candidates(q_static, x, ids_static, k, cand_ptr=ptr, workspace=ws, out=out, status=status)
    for qs, ids, want in ((qb, ids_b, want_b), (qa, ids_a, want_a), (qb, ids_b, want_b)):
        q_static.copy_(qs)
        ids_static.copy_(ids)
        graph.replay()
        torch.cuda.synchronize(dev)
        _assert_same(out, want, "replay")
    assert int(status.item()) == 0
