"""Host-side contract of the batched canonical-edge pass (no GPU): sizing entry points, the build_graphs switch, and the
shared test data's own precondition."""
import types

import numpy as np
import pytest

from evi_rag_amd import _lib
from tests import canonical_cases as cc


def test_workspace_bytes_depends_on_sizes_only_and_is_monotone():
    lib = _lib.load()
    ws = lib.evi_canonical_edges_workspace_bytes
    assert ws(0, 0, 1) > 0
    sizes = [(0, 1, 1), (1, 1, 1), (1000, 32, 64), (1000, 2000, 64), (1000, 2000, 768), (10 ** 6, 2000, 768), (1 << 33, 2000, 1024)]
    vals = [int(ws(*s)) for s in sizes]
    assert vals == sorted(vals)
    for E, B, D in sizes:
        assert ws(E + 1, B, D) >= ws(E, B, D) and ws(E, B + 1, D) >= ws(E, B, D) and ws(E, B, D + 1) >= ws(E, B, D)
    assert ws(2 * 10 ** 6, 2000, 768) > ws(10 ** 6, 2000, 768)   # every positive of every graph may have to go through it
    assert int(ws(1000, 32, 64)) == int(ws(1000, 32, 64))


def test_lds_capacity_is_positive():
    assert int(_lib.load().evi_canonical_edges_lds_capacity()) > 0


def test_build_graphs_refuses_canonicalisation_without_embeddings():
    import torch

    from evi_rag_amd import graph_build

    sample = types.SimpleNamespace(graph=[("a", "r", "b")], q_entity=["a"], a_entity=["b"], answer_subgraph=[])
    vocab = types.SimpleNamespace(entity_id=lambda e: 0, embedding_id=lambda e: 0, relation_id=lambda r: 0)
    for kw in ({}, {"question_emb_norm": torch.zeros(1, 4)}, {"relation_emb_norm": torch.zeros(1, 4)}):
        with pytest.raises(RuntimeError, match="Canonicalization requested but embeddings are missing."):
            graph_build.build_graphs([sample], vocab, vocab, ["g0"], canonicalize_relations=True, **kw)


def _all_cases():
    for seed, D, R in cc.RANDOM_SHAPES:
        yield f"random seed={seed} D={D}", cc.random_batch(seed, D, R)
    yield "capture variant", cc.variant(cc.random_batch(*cc.CAPTURE_SHAPE), cc.CAPTURE_VARIANT_SEED)
    cap = int(_lib.load().evi_canonical_edges_lds_capacity())
    seed, D, R = cc.OVERCAP_SHAPE
    yield "over capacity", cc.over_capacity_graph(cap, seed, D, R)


def test_generator_meets_its_precondition_for_every_gpu_case():
    for name, case in _all_cases():
        canon = cc._canonical_rows(case.rel_table)
        assert int(case.draws.max()) <= cc.MAX_DRAWS
        for g, gr in enumerate(case.graphs):
            assert cc.min_group_gap(gr, case.q[g], case.rel_table, canon) >= cc.MIN_GAP, (name, g)
            assert cc.oracle_follows_the_tie_rule(gr, case.q[g], case.rel_table, canon), (name, g)
        print(f"{name}: at most {int(case.draws.max())} draws per graph")
        # 2 D 2^-24 (twice the f32 dot error bound of unit vectors) stays below the gap
        assert 2 * case.D * 2.0 ** -24 <= cc.MIN_GAP
        assert np.allclose(np.linalg.norm(case.q.astype(np.float64), axis=1), 1.0, atol=1e-5)


def test_generator_holds_the_named_cases():
    c = cc.random_batch(*cc.RANDOM_SHAPES[0])
    assert c.B == cc.B_RANDOM and c.R == cc.R_RANDOM
    assert c.graphs[0]["src"].shape[0] == 0
    assert c.graphs[1]["mask"].sum() == 0 and c.graphs[2]["mask"].sum() == 1
    assert c.want_per_graph[3][0] == c.graphs[3]["mask"].tolist()                         # singletons: all kept
    assert sum(c.want_per_graph[4][0]) == 3                                               # (u,v)+(v,u), self loops, one single
    assert sum(c.want_per_graph[5][0]) == 3                                               # 65 + 129 members + one single
    # a repeated relation id: the lowest edge id; byte-identical rows: the lower relation id
    assert c.want_per_graph[6][0] == [True, False, False, True, False, True, False]
    assert c.want_per_graph[7][0][:3] == [True, False, False]
    assert np.array_equal(c.rel_table[cc.TWIN_LO], c.rel_table[cc.TWIN_HI])
    assert (c.pair_len == -1).any() and (c.pair_count[c.pair_len == -1] == 0).all()
    assert (c.mask[c.pair_ids] == 0).any()                                                # pair ids on non-positive edges
    assert (np.bincount(c.pair_ids) > 1).any()                                            # an edge listed in several pairs
    assert (np.diff(c.pair_ids[c.pair_off[3]: c.pair_off[4]]) < 0).any()                  # not ascending
    assert c.rel.max() == c.R - 1
    # the over-capacity graph: capacity + 1 positives, a group across the boundary
    cap = int(_lib.load().evi_canonical_edges_lds_capacity())
    o = cc.over_capacity_graph(cap, *cc.OVERCAP_SHAPE[:2], cc.OVERCAP_SHAPE[2])
    assert int(o.mask.sum()) == cap + 1
    pos = np.nonzero(o.mask)[0]
    assert o.edge_index[0, pos[cap - 1]] == o.edge_index[0, pos[cap]] and o.edge_index[1, pos[cap - 1]] == o.edge_index[1, pos[cap]]
