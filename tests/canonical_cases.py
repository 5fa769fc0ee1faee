"""Shared data for the batched canonical-edge tests (labelling.canonicalize_flat): seeded batches of multigraphs with the
named corner cases, their questions, and the expected result from oracle.cosine.canonicalize_positive_mask per graph.

Precondition of every batch (asserted by `finish`): in every group of two or more positive edges, the two best scores of
DISTINCT relation rows differ by at least MIN_GAP = 2.5e-4 in float64.  (Two relation ids whose table rows are byte-identical
count as one row: their scores are equal by construction and the tie rule, not the arithmetic, decides between them.)
2.5e-4 >= 2 * D * 2^-24 for D <= 2048, twice the worst-case error of an f32 dot product of unit vectors under any summation
order, so the oracle's f32 argmax and the kernel's both pick the float64 winner.  Between copies of ONE row the gap is zero and
the oracle itself has to tie exactly for its pick to be the rule's; `oracle_follows_the_tie_rule` says where it does (a BLAS
matrix-vector product is not bound to).  A graph's question is redrawn, seeded, at most MAX_DRAWS times until both hold.
"""
from __future__ import annotations

import types
from typing import Dict, List

import numpy as np

from oracle import cosine as ocos

MIN_GAP = 2.5e-4
MAX_DRAWS = 64
B_RANDOM = 70
R_RANDOM = 37
TWIN_LO, TWIN_HI = 5, 11          # relation ids whose table rows are byte-identical
# (seed, D, R) of the randomised batches the GPU tests run; 37 is not a multiple of the vector width
RANDOM_SHAPES = [(0, 64, R_RANDOM), (1, 100, R_RANDOM), (2, 768, R_RANDOM), (3, 37, R_RANDOM)]
CAPTURE_SHAPE = (0, 64, R_RANDOM)  # the captured call: this batch, then `variant` of it with seed CAPTURE_VARIANT_SEED
CAPTURE_VARIANT_SEED = 11
OVERCAP_SHAPE = (5, 64, R_RANDOM)
BUILD_SHAPE = (7, 48, 12)          # embeddings of the build_graphs chunk


def _unit_rows(rng, n, D):
    x = rng.standard_normal((n, D))
    return (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32)


def relation_table(seed: int, R: int, D: int) -> np.ndarray:
    rel = _unit_rows(np.random.default_rng([seed, 1000]), R, D)
    if R > TWIN_HI:
        rel[TWIN_HI] = rel[TWIN_LO]
    return rel


def _graph(n_nodes, edges, pairs):
    """edges: [(u, v, rel, positive)], pairs: [(pair_len, [local edge ids])]"""
    e = np.asarray(edges, np.int64).reshape(-1, 4)
    return {"n": int(n_nodes), "src": e[:, 0].copy(), "dst": e[:, 1].copy(), "rel": e[:, 2].copy(),
            "mask": e[:, 3].astype(bool), "pairs": [(int(l), [int(i) for i in ids]) for l, ids in pairs]}


def _random_graph(rng, R):
    n = int(rng.integers(8, 40))
    edges = []
    for _ in range(int(rng.integers(1, 17))):              # multi-edge groups of 2..5 positives, either orientation
        u, v = (int(x) for x in rng.integers(0, n, 2))
        for _ in range(int(rng.integers(2, 6))):
            a, b = (u, v) if rng.random() < 0.5 else (v, u)
            edges.append((a, b, int(rng.integers(0, R)), 1))
        if rng.random() < 0.3:                             # a non-positive edge parallel to the group
            edges.append((u, v, int(rng.integers(0, R)), 0))
    for _ in range(int(rng.integers(0, 12))):
        u, v = (int(x) for x in rng.integers(0, n, 2))
        edges.append((u, v, int(rng.integers(0, R)), int(rng.random() < 0.6)))
    order = rng.permutation(len(edges))
    edges = [edges[i] for i in order]
    E = len(edges)
    pairs = []
    for _ in range(int(rng.integers(1, 5))):
        if rng.random() < 0.2:
            pairs.append((-1, []))                          # a slot without a path
            continue
        ids = rng.permutation(E)[: int(rng.integers(1, E + 1))]   # not ascending; positives and non-positives alike
        pairs.append((int(rng.integers(1, 5)), ids.tolist()))
    if len(pairs) >= 2 and pairs[0][1] and pairs[1][0] >= 0:
        pairs[1] = (pairs[1][0], pairs[1][1] + pairs[0][1][:3])   # edges listed in several pairs (and twice in one)
    return _graph(n, edges, pairs)


def _named_graphs(R):
    g = []
    g.append(_graph(3, [], []))                                                        # 0: no edges
    g.append(_graph(4, [(0, 1, 3, 0), (1, 0, 4, 0), (2, 3, 1, 0)], [(-1, []), (-1, [])]))  # 1: no positive
    g.append(_graph(4, [(0, 1, 3, 0), (1, 2, 4, 1), (2, 3, 1, 0)], [(1, [1, 0]), (2, [2, 1, 1])]))  # 2: one positive
    g.append(_graph(6, [(0, 1, 3, 1), (1, 2, 4, 1), (2, 3, 1, 1), (3, 4, 1, 1), (1, 2, 9, 0), (5, 5, 2, 1)],
                    [(2, [3, 0, 4, 5]), (-1, []), (1, [2])]))                          # 3: singletons only (one a self loop)
    g.append(_graph(5, [(0, 1, 2, 1), (1, 0, 8, 1), (3, 3, 6, 1), (2, 4, 1, 1), (3, 3, 14, 1), (3, 3, 20, 0)],
                    [(1, [4, 2, 1, 0, 3]), (1, [5, 1])]))                              # 4: (u,v)+(v,u); a self-loop group
    big = [(7, 2, (3 * i) % R, 1) if i % 2 else (2, 7, (5 * i + 1) % R, 1) for i in range(65)]
    big += [(4, 9, (7 * i + 2) % R, 1) if i % 3 else (9, 4, (11 * i) % R, 1) for i in range(129)]
    big += [(2, 7, 1, 0), (0, 1, 2, 1)]
    g.append(_graph(10, big, [(3, list(range(195, -1, -5))), (1, [64, 65, 66, 0, 1])]))  # 5: groups of 65 and 129
    g.append(_graph(6, [(0, 1, 7, 1), (2, 3, TWIN_HI, 1), (1, 0, 7, 1), (4, 5, 0, 1), (0, 1, 7, 1), (3, 2, TWIN_LO, 1),
                        (2, 3, TWIN_HI, 1)],
                    [(2, [4, 2, 0, 6, 5, 1])]))                # 6: one relation id repeated; byte-identical relation rows
    g.append(_graph(4, [(0, 1, R - 1, 1), (0, 1, R - 1, 1), (1, 0, R - 1, 1), (2, 3, R - 1, 1), (3, 2, 0, 1)],
                    [(1, [4, 3, 2, 1, 0])]))                                           # 7: relation id R - 1
    return g


def _canonical_rows(rel: np.ndarray) -> np.ndarray:
    """canon[r] = the smallest relation id whose row has the same bytes as row r."""
    first: Dict[bytes, int] = {}
    return np.asarray([first.setdefault(rel[r].tobytes(), r) for r in range(rel.shape[0])], np.int64)


def min_group_gap(graph, q: np.ndarray, rel: np.ndarray, canon: np.ndarray) -> float:
    """Smallest float64 gap between the two best distinct-row scores over the graph's multi-edge groups (inf: none)."""
    scores = rel.astype(np.float64) @ q.astype(np.float64)
    groups = ocos.group_positive_edges_by_pair(graph["src"], graph["dst"], graph["mask"])
    gap = np.inf
    for members in groups.values():
        rows = np.unique(canon[graph["rel"][members]])
        if len(members) < 2 or rows.shape[0] < 2:
            continue
        s = np.sort(scores[rows])
        gap = min(gap, float(s[-1] - s[-2]))
    return gap


def oracle_follows_the_tie_rule(graph, q: np.ndarray, rel: np.ndarray, canon: np.ndarray) -> bool:
    """Whether the oracle's own f32 arithmetic ties exactly where the rule says it must.  The oracle scores a group with one
    matrix-vector product over the members' rows, and a BLAS gemv may round identical rows of one product differently by their
    position in it; its argmax then lands on a later copy of the best row.  The rule under test (first maximum in
    (relation_id, idx) order, identical rows scoring identically) is only pinned by the oracle where, in every group, the
    oracle's pick is the first member in that order that carries the float64-best row."""
    scores = rel.astype(np.float64) @ q.astype(np.float64)
    groups = ocos.group_positive_edges_by_pair(graph["src"], graph["dst"], graph["mask"])
    picks = ocos.select_canonical_edge_indices(groups, graph["rel"], rel, q)
    for members, pick in zip(groups.values(), picks):
        if len(members) < 2:
            continue
        ordered = sorted(members, key=lambda i: (int(graph["rel"][i]), i))
        rows = canon[graph["rel"][ordered]]
        best = rows[int(np.argmax(scores[rows]))]
        if pick != ordered[int(np.nonzero(rows == best)[0][0])]:
            return False
    return True


def meets_precondition(graph, q, rel, canon) -> bool:
    return min_group_gap(graph, q, rel, canon) >= MIN_GAP and oracle_follows_the_tie_rule(graph, q, rel, canon)


def finish(graphs: List[dict], rel: np.ndarray, seed: int):
    """Draws the questions (meeting the precondition), lays the batch out flat and computes the expected result."""
    R, D = rel.shape
    canon = _canonical_rows(rel)
    B = len(graphs)
    q = np.zeros((B, D), np.float32)
    draws = np.zeros(B, np.int64)
    for g, gr in enumerate(graphs):
        for attempt in range(MAX_DRAWS):
            cand = _unit_rows(np.random.default_rng([seed, 2000, g, attempt]), 1, D)[0]
            if meets_precondition(gr, cand, rel, canon):
                break
        assert meets_precondition(gr, cand, rel, canon), f"graph {g}: no question met the precondition in {MAX_DRAWS} draws"
        q[g], draws[g] = cand, attempt + 1
    e_cnt = np.asarray([gr["src"].shape[0] for gr in graphs], np.int64)
    edge_ptr = np.concatenate([[0], np.cumsum(e_cnt)]).astype(np.int64)
    node_ptr = np.concatenate([[0], np.cumsum([gr["n"] for gr in graphs])]).astype(np.int64)
    cat = lambda parts, dt: np.concatenate(parts).astype(dt) if parts else np.empty(0, dt)  # noqa: E731
    c = types.SimpleNamespace(B=B, R=R, D=D, graphs=graphs, q=q, rel_table=rel, draws=draws, edge_ptr=edge_ptr, E=int(edge_ptr[-1]))
    c.edge_index = np.stack([cat([gr["src"] + node_ptr[g] for g, gr in enumerate(graphs)], np.int64),
                             cat([gr["dst"] + node_ptr[g] for g, gr in enumerate(graphs)], np.int64)])
    c.rel = cat([gr["rel"] for gr in graphs], np.int64)
    c.mask = cat([gr["mask"] for gr in graphs], np.uint8)
    c.pair_ptr = np.concatenate([[0], np.cumsum([len(gr["pairs"]) for gr in graphs])]).astype(np.int64)
    c.pair_graph = np.repeat(np.arange(B, dtype=np.int64), np.diff(c.pair_ptr))
    c.pair_len = cat([[l for l, _ in gr["pairs"]] for gr in graphs], np.int32)
    c.pair_count = cat([[len(ids) for _, ids in gr["pairs"]] for gr in graphs], np.int32)
    c.pair_off = np.concatenate([[0], np.cumsum(c.pair_count, dtype=np.int64)]).astype(np.int64)
    c.pair_ids = cat([np.asarray(ids, np.int64) + edge_ptr[g] for g, gr in enumerate(graphs) for _, ids in gr["pairs"]], np.int64)
    c.P = int(c.pair_count.shape[0])
    # expected: the oracle per graph, on graph-local ids
    keep, new_cnt, new_ids, per_graph = [], [], [], []
    for g, gr in enumerate(graphs):
        ids = [i for _, p in gr["pairs"] for i in p]
        cnts = [len(p) for _, p in gr["pairs"]]
        km, ni, nc = ocos.canonicalize_positive_mask(gr["src"].tolist(), gr["dst"].tolist(), gr["rel"].tolist(), gr["mask"].tolist(),
                                                     ids, cnts, q[g], rel)
        per_graph.append((list(km), list(ni), list(nc)))
        keep.append(np.asarray(km, np.uint8).reshape(-1))
        new_cnt.append(np.asarray(nc, np.int32).reshape(-1))
        new_ids.append(np.asarray(ni, np.int64).reshape(-1) + edge_ptr[g])
    c.want_per_graph = per_graph
    c.want_keep = cat(keep, np.uint8)
    c.want_count = cat(new_cnt, np.int32)
    c.want_off = np.concatenate([[0], np.cumsum(c.want_count, dtype=np.int64)]).astype(np.int64)
    c.want_ids = cat(new_ids, np.int64)
    assert c.want_count.shape[0] == c.P and c.want_keep.shape[0] == c.E
    return c


def random_batch(seed: int, D: int, R: int = R_RANDOM, B: int = B_RANDOM):
    rng = np.random.default_rng([seed, 3000])
    graphs = _named_graphs(R)
    while len(graphs) < B:
        graphs.append(_random_graph(rng, R))
    return finish(graphs, relation_table(seed, R, D), seed)


def variant(case, seed: int):
    """The same edges and pair lists with other positives (a third of them cleared) and other questions."""
    rng = np.random.default_rng([seed, 4000])
    graphs = []
    for gr in case.graphs:
        g2 = dict(gr)
        g2["mask"] = gr["mask"] & (rng.random(gr["mask"].shape[0]) >= 1.0 / 3.0)
        graphs.append(g2)
    return finish(graphs, case.rel_table, seed)


def over_capacity_graph(capacity: int, seed: int, D: int, R: int = R_RANDOM):
    """One graph with capacity + 1 positives: two-member groups, a last group of three (or four) whose members lie on both
    sides of position `capacity` in the edge order, a few non-positive edges in between."""
    rng = np.random.default_rng([seed, 5000])
    n_pos = capacity + 1
    last = 3 if n_pos % 2 else 4
    edges = []
    for k in range((n_pos - last) // 2):
        r0 = int(rng.integers(0, R))
        r1 = int((r0 + 1 + rng.integers(0, R - 1)) % R)
        edges.append((k, k + 1, r0, 1))
        edges.append((k + 1, k, r1, 1) if k % 2 else (k, k + 1, r1, 1))
        if k % 97 == 0:
            edges.append((k, k + 1, int(rng.integers(0, R)), 0))
    n = (n_pos - last) // 2 + 3
    edges += [(n - 1, 0, int(r), 1) for r in rng.permutation(R)[:last]]
    E = len(edges)
    assert sum(e[3] for e in edges) == n_pos
    pairs = [(2, rng.permutation(E)[:60].tolist()), (-1, []), (3, list(range(E - 1, E - 41, -1)))]
    return finish([_graph(n, edges, pairs)], relation_table(seed, R, D), seed)


def upload(case, dev):
    """(FlatPairLabels, edge_index, edge_relation_ids, question, relation table) on the device."""
    import torch

    from evi_rag_amd import labelling as L

    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    mask = torch.zeros(max(case.E, 1), dtype=torch.uint8, device=dev)
    mask[: case.E] = t(case.mask)
    z = np.zeros(case.P, np.int64)
    flat = L.FlatPairLabels(case.B, case.E, case.edge_ptr, mask, t(case.pair_len), t(case.pair_count), t(case.pair_off),
                            t(case.pair_ids) if case.pair_ids.shape[0] else torch.empty(1, dtype=torch.int64, device=dev),
                            case.pair_graph, z, z.copy(), case.pair_ptr, edge_ptr=t(case.edge_ptr))
    return flat, t(case.edge_index), t(case.rel), t(case.q), t(case.rel_table)
