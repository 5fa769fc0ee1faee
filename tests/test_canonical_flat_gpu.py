"""labelling.canonicalize_flat (evi_canonical_edges) against oracle.cosine.canonicalize_positive_mask per graph and the
reference-produced tests/golden/cosine.npz; the batch and build_graphs forms on top of it."""
import functools
import os
import types

import numpy as np
import pytest
import torch

from oracle import cosine as ocos
from tests import canonical_cases as cc

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@functools.lru_cache(maxsize=None)
def _random_case(seed, D, R):
    return cc.random_batch(seed, D, R)   # computed once, shared, never modified


def _assert_matches(out, flat_in, case):
    """keep, counts, offsets and ids equal the oracle's bit for bit; pair_len and the host fields are the input's."""
    from evi_rag_amd import labelling as L

    assert isinstance(out, L.CanonicalPairLabels) and isinstance(out, L.FlatPairLabels)
    out.check_deferred()
    assert out.mask.dtype == torch.uint8 and np.array_equal(out.mask[: case.E].cpu().numpy(), case.want_keep)
    assert out.pair_count.dtype == torch.int32 and np.array_equal(out.pair_count.cpu().numpy(), case.want_count)
    assert out.pair_edge_off.dtype == torch.int64 and np.array_equal(out.pair_edge_off.cpu().numpy(), case.want_off)
    total = int(case.want_off[-1])
    assert np.array_equal(out.pair_edge_ids[:total].cpu().numpy(), case.want_ids)
    assert out.pair_edge_ids.numel() == flat_in.pair_edge_ids.numel()
    assert torch.equal(out.pair_len, flat_in.pair_len)
    for name in ("pair_graph_h", "pair_start_h", "pair_answer_h", "pair_ptr_h", "edge_ptr_h"):
        assert np.array_equal(getattr(out, name), getattr(flat_in, name)), name
    assert (out.B, out.E, out.P) == (flat_in.B, flat_in.E, flat_in.P)


def _golden_case(copies):
    """The golden graph `copies` times over as one batch with batch-global node and edge ids."""
    z = np.load(os.path.join(GOLD, "cosine.npz"), allow_pickle=False)
    E, n = len(z["edge_src"]), int(max(z["edge_src"].max(), z["edge_dst"].max())) + 1
    ids, cnt = z["pair_ids"].astype(np.int64), z["pair_counts"].astype(np.int32)
    c = types.SimpleNamespace(B=copies, E=copies * E, P=copies * len(cnt), R=z["rel_norm"].shape[0], D=z["rel_norm"].shape[1])
    c.edge_ptr = np.arange(copies + 1, dtype=np.int64) * E
    c.edge_index = np.concatenate([np.stack([z["edge_src"], z["edge_dst"]]).astype(np.int64) + g * n for g in range(copies)], axis=1)
    c.rel = np.tile(z["edge_rel"].astype(np.int64), copies)
    c.mask = np.tile(z["positive"].astype(np.uint8), copies)
    c.pair_ptr = np.arange(copies + 1, dtype=np.int64) * len(cnt)
    c.pair_graph = np.repeat(np.arange(copies, dtype=np.int64), len(cnt))
    c.pair_len = np.ones(c.P, np.int32)
    c.pair_count = np.tile(cnt, copies)
    c.pair_off = np.concatenate([[0], np.cumsum(c.pair_count, dtype=np.int64)]).astype(np.int64)
    c.pair_ids = np.concatenate([ids + g * E for g in range(copies)])
    c.q = np.tile(z["q_norm"].astype(np.float32).reshape(1, -1), (copies, 1))
    c.rel_table = z["rel_norm"].astype(np.float32)
    keep = np.zeros(E, np.uint8)
    keep[z["keep_indices"]] = 1
    c.want_keep = np.tile(keep, copies)
    c.want_count = np.tile(z["new_pair_counts"].astype(np.int32), copies)
    c.want_off = np.concatenate([[0], np.cumsum(c.want_count, dtype=np.int64)]).astype(np.int64)
    c.want_ids = np.concatenate([z["new_pair_ids"].astype(np.int64) + g * E for g in range(copies)])
    assert (np.diff(ids) < 0).any()   # the golden lists are not ascending: "original order preserved" is pinned
    return c


@pytest.mark.parametrize("copies", [1, 3])
def test_golden_case_as_a_batch(dev, copies):
    from evi_rag_amd import labelling as L

    case = _golden_case(copies)
    flat, ei, rel, q, table = cc.upload(case, dev)
    _assert_matches(L.canonicalize_flat(flat, ei, rel, q, table), flat, case)


@pytest.mark.parametrize("seed,D,R", cc.RANDOM_SHAPES)
def test_randomised_batch_matches_oracle(dev, seed, D, R):
    from evi_rag_amd import labelling as L

    case = _random_case(seed, D, R)
    flat, ei, rel, q, table = cc.upload(case, dev)
    before = [t.clone() for t in (flat.mask, flat.pair_count, flat.pair_edge_off, flat.pair_edge_ids, flat.pair_len)]
    out = L.canonicalize_flat(flat, ei, rel, q, table)
    _assert_matches(out, flat, case)
    for t, b in zip((flat.mask, flat.pair_count, flat.pair_edge_off, flat.pair_edge_ids, flat.pair_len), before):
        assert torch.equal(t, b)   # the inputs are not written
    assert out.mask.data_ptr() != flat.mask.data_ptr() and out.pair_edge_ids.data_ptr() != flat.pair_edge_ids.data_ptr()
    # per_graph() works as it stands on the result
    per = out.per_graph()
    for g in range(case.B):
        km, ni, nc = case.want_per_graph[g]
        pairs = case.graphs[g]["pairs"]
        assert per[g][0].tolist() == [bool(x) for x in km]
        assert per[g][3] == [int(i) for i in ni] if pairs else per[g][3] == []
        assert per[g][4] == [int(c) for c, (l, _) in zip(nc, pairs) if l >= 0]
        assert per[g][5] == [l for l, _ in pairs if l >= 0]


def test_scalar_and_vector_row_reads_give_the_same_scores(dev):
    """A score depends on the rows' bytes only: the same tables at an address that is not 16-byte aligned (scalar reads)."""
    from evi_rag_amd import labelling as L

    seed, D, R = cc.RANDOM_SHAPES[0]
    case = _random_case(seed, D, R)
    flat, ei, rel, q, table = cc.upload(case, dev)
    q_off = torch.empty(q.numel() + 1, dtype=torch.float32, device=dev)[1:].view_as(q).copy_(q)
    t_off = torch.empty(table.numel() + 1, dtype=torch.float32, device=dev)[1:].view_as(table).copy_(table)
    assert q_off.data_ptr() % 16 != 0 and t_off.data_ptr() % 16 != 0 and q_off.is_contiguous()
    _assert_matches(L.canonicalize_flat(flat, ei, rel, q_off, t_off), flat, case)


def test_graph_over_the_lds_capacity(dev):
    from evi_rag_amd import _lib
    from evi_rag_amd import labelling as L

    cap = int(_lib.load().evi_canonical_edges_lds_capacity())
    seed, D, R = cc.OVERCAP_SHAPE
    case = cc.over_capacity_graph(cap, seed, D, R)
    assert int(case.mask.sum()) == cap + 1
    flat, ei, rel, q, table = cc.upload(case, dev)
    _assert_matches(L.canonicalize_flat(flat, ei, rel, q, table), flat, case)


def test_deferred_faults(dev):
    """A relation id == R on a scored edge is reported by check_deferred (and scored clamped: nothing outside the table is
    read); the same id on a singleton's edge is never looked at."""
    from evi_rag_amd import labelling as L

    seed, D, R = cc.RANDOM_SHAPES[0]
    case = _random_case(seed, D, R)
    flat, ei, rel, q, table = cc.upload(case, dev)
    e4, e3 = int(case.edge_ptr[4]), int(case.edge_ptr[3])
    single = rel.clone()
    single[e3 + 0] = R           # graph 3: singletons only
    single[e4 + 3] = R           # graph 4, edge 3: a singleton beside two groups
    single[int(case.edge_ptr[1])] = R   # a non-positive edge
    out = L.canonicalize_flat(flat, ei, single, q, table)
    _assert_matches(out, flat, case)
    scored = rel.clone()
    scored[e4 + 0] = R           # graph 4, edge 0: a member of the (u,v)+(v,u) group
    out = L.canonicalize_flat(flat, ei, scored, q, table)
    with pytest.raises(ValueError, match="relation id outside"):
        out.check_deferred()
    with pytest.raises(ValueError, match="relation id outside"):
        out.per_graph()
    assert int(out.status.item()) & 1
    # the other graphs are what they were
    keep = out.mask[: case.E].cpu().numpy()
    rest = np.ones(case.E, bool)
    rest[e4: int(case.edge_ptr[5])] = False
    assert np.array_equal(keep[rest], case.want_keep[rest])
    nan_q = q.clone()
    nan_q[4, 0] = float("nan")
    out = L.canonicalize_flat(flat, ei, rel, nan_q, table)
    assert int(out.status.item()) == 2
    with pytest.raises(ValueError, match="not finite"):
        out.check_deferred()


def test_validation_errors_carry_the_reference_texts(dev):
    from evi_rag_amd import labelling as L

    case = _golden_case(1)
    flat, ei, rel, q, table = cc.upload(case, dev)
    with pytest.raises(ValueError, match="question_embedding is empty"):
        L.canonicalize_flat(flat, ei, rel, q[:, :0], table)
    with pytest.raises(ValueError, match="relation_embeddings are empty; cannot canonicalize positives."):
        L.canonicalize_flat(flat, ei, rel, q, table[:0])
    with pytest.raises(ValueError, match=r"Embeddings must be 2D \(relations\) and 1D \(question\) for canonicalization."):
        L.canonicalize_flat(flat, ei, rel, q, table.view(-1))
    with pytest.raises(ValueError, match="Question embedding dim does not match relation embedding dim."):
        L.canonicalize_flat(flat, ei, rel, q[:, :-4], table)


def test_call_replays_in_a_hip_graph(dev):
    """No read-back and no allocation inside the C call: captured once, replayed on new mask and question bytes."""
    from evi_rag_amd import labelling as L

    a = _random_case(*cc.CAPTURE_SHAPE)
    b = cc.variant(a, cc.CAPTURE_VARIANT_SEED)
    assert not np.array_equal(a.mask, b.mask) and not np.array_equal(a.want_keep, b.want_keep)
    flat, ei, rel, q, table = cc.upload(a, dev)
    mask_b, q_b = torch.from_numpy(b.mask).to(dev), torch.from_numpy(b.q).to(dev)
    mask_a, q_a = flat.mask[: a.E].clone(), q.clone()
    stream = torch.cuda.Stream(device=dev)
    stream.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(stream):
        L.canonicalize_flat(flat, ei, rel, q, table)   # warm-up on the side stream: sizes the cached workspace
    torch.cuda.current_stream(dev).wait_stream(stream)
    torch.cuda.synchronize(dev)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = L.canonicalize_flat(flat, ei, rel, q, table)
    for m, qq, case in ((mask_b, q_b, b), (mask_a, q_a, a), (mask_b, q_b, b)):
        flat.mask[: a.E].copy_(m)
        q.copy_(qq)
        graph.replay()
        torch.cuda.synchronize(dev)
        _assert_matches(out, flat, case)


def test_batch_form_equals_the_single_graph_function(dev):
    from evi_rag_amd import labelling as L

    seed, D, R = cc.RANDOM_SHAPES[0]
    case = _random_case(seed, D, R)
    gs = case.graphs
    args = ([g["src"].tolist() for g in gs], [g["dst"].tolist() for g in gs], [g["rel"].tolist() for g in gs],
            [g["mask"].tolist() for g in gs], [[i for _, p in g["pairs"] for i in p] for g in gs],
            [[len(p) for _, p in g["pairs"]] for g in gs])
    q, table = torch.from_numpy(case.q).to(dev), torch.from_numpy(case.rel_table).to(dev)
    got = L.canonicalize_positive_edges_batch(*args, q, table)
    assert len(got) == case.B
    for g in range(case.B):
        single = L.canonicalize_positive_edges(*(a[g] for a in args), q[g], table)
        assert got[g] == single, g
        assert got[g] == tuple(case.want_per_graph[g]), g
    # the early returns: inputs come back as given
    same = L.canonicalize_positive_edges_batch([[], [0, 1]], [[], [1, 0]], [[], [2, 3]], [[], [False, False]], [[], [1, 0]], [[], [2]],
                                               q[:2], table)
    assert same == [([], [], []), ([False, False], [1, 0], [2])]
    # empty pair lists: the keep mask, the lists as given
    km, ids, cnts = L.canonicalize_positive_edges_batch([[0, 1, 0]], [[1, 0, 1]], [[2, 2, 3]], [[True, True, False]], [[]], [[]],
                                                        q[:1], table)[0]
    assert km == [True, False, False] and ids == [] and cnts == []
    with pytest.raises(ValueError, match="pair_edge_counts do not sum"):
        L.canonicalize_positive_edges_batch([[0, 1]], [[1, 0]], [[2, 3]], [[True, True]], [[0, 1]], [[1]], q[:1], table)


def test_build_graphs_canonicalises_the_chunk(dev):
    """build_graphs(canonicalize_relations=True) == build_graphs() followed by the oracle per record."""
    from evi_rag_amd import graph_build

    seed, D, R = cc.BUILD_SHAPE
    rng = np.random.default_rng([seed, 6000])
    ent_vocab = types.SimpleNamespace(entity_id=lambda e: int(e[1:]), embedding_id=lambda e: int(e[1:]) + 1)
    rel_vocab = types.SimpleNamespace(relation_id=lambda r: int(r[1:]))
    samples = []
    for s in range(9):
        n = int(rng.integers(4, 9))                       # few nodes, many triples: parallel edges on the shortest paths
        tri = [(f"e{int(h)}", f"r{int(r)}", f"e{int(t)}") for h, r, t in
               zip(rng.integers(0, n, 40), rng.integers(0, R, 40), rng.integers(0, n, 40))]
        if s == 4:
            tri = [("e0", "r1", "e1")]                    # one edge: nothing to canonicalise
        samples.append(types.SimpleNamespace(graph=tri, q_entity=[f"e{int(i)}" for i in rng.integers(0, n, 2)],
                                             a_entity=[f"e{int(i)}" for i in rng.integers(0, n, 2)], answer_subgraph=[]))
    ids = [f"g{s}" for s in range(len(samples))]
    plain = graph_build.build_graphs(samples, ent_vocab, rel_vocab, ids)
    table = cc.relation_table(seed, R, D)
    canon = cc._canonical_rows(table)
    q = np.zeros((len(samples), D), np.float32)
    for s, rec in enumerate(plain):                       # questions that meet the shared precondition for the built graphs
        gr = {"src": np.asarray(rec.edge_src, np.int64), "dst": np.asarray(rec.edge_dst, np.int64),
              "rel": np.asarray(rec.edge_relation_ids, np.int64), "mask": np.asarray(rec.positive_triple_mask, bool)}
        for attempt in range(cc.MAX_DRAWS):
            q[s] = cc._unit_rows(np.random.default_rng([seed, 7000, s, attempt]), 1, D)[0]
            if cc.meets_precondition(gr, q[s], table, canon):
                break
        assert cc.meets_precondition(gr, q[s], table, canon)
    got = graph_build.build_graphs(samples, ent_vocab, rel_vocab, ids, canonicalize_relations=True,
                                   question_emb_norm=torch.from_numpy(q).to(dev), relation_emb_norm=torch.from_numpy(table).to(dev))
    changed = 0
    for s, (rec, base) in enumerate(zip(got, plain)):
        km, ni, nc = ocos.canonicalize_positive_mask(base.edge_src, base.edge_dst, base.edge_relation_ids, base.positive_triple_mask,
                                                     base.pair_edge_local_ids, base.pair_edge_counts, q[s], table)
        assert rec.positive_triple_mask == list(km) and rec.pair_edge_local_ids == list(ni) and rec.pair_edge_counts == list(nc), s
        changed += rec.positive_triple_mask != base.positive_triple_mask
        for name in ("graph_id", "node_entity_ids", "node_embedding_ids", "node_labels", "edge_src", "edge_dst", "edge_relation_ids",
                     "pair_start_node_locals", "pair_answer_node_locals", "pair_shortest_lengths"):
            assert getattr(rec, name) == getattr(base, name), (s, name)
    assert changed > 0   # the chunk does hold parallel positive edges
