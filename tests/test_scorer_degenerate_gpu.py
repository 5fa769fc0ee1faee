"""GPU: the edge scorer's forward and all 25 parameter gradients against the float64 model on DEGENERATE batches.

Every other value / gradient check of the scorer runs on `synthetic.make_batch` batches: every graph has edges, two nodes and
a seed, no self loops, no repeated triples, dense relation ids.  A PyG `Batch` has none of those guarantees.  The batches
here are built by hand: graphs without edges (first, last, two in a row, at and next to a chunk boundary), self loops and
parallel edges, graphs without a seed / of seeds only / with isolated nodes, non-text nodes everywhere and nowhere, relation
ids with holes / one per edge / beyond E / through the relation table, B = 1 / 33 / 40 with a 300-edge star, the three
direction modes with one-sided DDE rounds, and the training-shaped chain through `RetrieverLoss`.

Reference: tests/scorer_f64.py (float64 + autograd, pinned to the reference's goldens by tests/test_scorer_f64_cpu.py).
Bars (the project's existing ones): outputs 2e-4 absolute; every gradient within 2e-5 (EVI_SCORER_GEMM=f32) or 2e-4
(default split-bf16 GEMM) of that gradient's float64 max, 1e-6 floor; a gradient without any term in float64 must be exactly
zero from the kernel.  Two rules for sums that cancel (one-element gradients, gradients that are zero by an invariance) are
derived above KAPPA below.

The gradient runs keep per-edge relation-context rows (a backward follows, and the batches are far below 1 024 edges), so
EVI_SCORER_PAIRS does nothing in them; the (relation, graph) pair rows — pair count equal to E, holes, edgeless graphs, the
switch on and off — are judged forward-only at E = 1 112 by test_relation_graph_pair_rows_forward.

Measured on an MI355X, f32 GEMM / default GEMM — worst output error; worst gradient ratio of the 23 matrix and vector
gradients; worst ratio of the two one-element gradients under their rule (largest condition number met):

    case                                                outputs            gradients          one-element (kappa)
    graphs without edges (one chunk / 65 / 64; replay = recompute)
                                                        3.0e-7 / 7.1e-6    5.6e-7 / 2.3e-5    5.4e-7 / 1.4e-5  (35)
    self loops and parallel edges                       2.1e-7 / 5.8e-6    9.4e-7 / 1.4e-5    8.1e-7 / 4.7e-6  (28)
    no seed / seeds only / isolated nodes               2.8e-7 / 6.7e-6    5.6e-7 / 1.5e-5    1.0e-7 / 3.7e-6  (5)
    a graph of non-text nodes                           2.3e-7 / 7.3e-6    1.5e-6 / 2.0e-5    2.4e-8 / 6.8e-7  (49)
    no non-text node (non_text_entity_emb exactly 0)    2.8e-7 / 7.3e-6    1.1e-6 / 2.3e-5    1.7e-7 / 7.9e-6  (49)
    relation ids {0, 7, E-1} (ids = table; no dedupe)   2.8e-7 / 5.7e-6    8.7e-7 / 1.3e-5    8.2e-7 / 4.6e-6  (7)
    one relation per edge (ids = table; no dedupe)      2.5e-7 / 6.3e-6    8.2e-7 / 8.2e-6    3.8e-7 / 6.0e-6  (4)
    a relation id >= E                                  4.4e-7 / 6.6e-6    8.5e-7 / 1.2e-5    1.2e-7 / 2.3e-6  (12)
    B = 1                                               2.0e-7 / 2.3e-6    3.5e-7 / 5.4e-6    9.1e-8 / 1.0e-6  (3)
    B = 33 tiny graphs                                  3.0e-7 / 8.7e-6    1.4e-6 / 2.2e-5    7.8e-7 / 1.7e-5  (27)
    B = 40 with the 300-edge star                       3.5e-7 / 7.7e-6    1.4e-6 / 2.4e-5    4.7e-7 / 5.9e-6  (36)
    3 direction modes x rounds (0,4) (4,0) (3,1), worst of 9
                                                        4.2e-7 / 9.4e-6    1.2e-6 / 1.6e-4    1.2e-6 / 2.2e-5  (430)
    loss chain, InfoNCE                                 3.0e-7 / 7.1e-6    2.5e-6 / 1.6e-5    7.5e-8 / 6.8e-7  (3)
        loss value off by 3.1e-7; the two gradients that are zero by invariance at 4.1e-3 / 1.2e-3 of their absolute bound
    loss chain, InfoNCE + BCE + edge weights            3.0e-7 / 7.1e-6    5.3e-7 / 8.6e-6    1.7e-7 / 4.7e-7  (6)
        loss value off by 1.2e-8
    pair rows, forward only, default GEMM, E = 1 112    pairs == E: 9.2e-6    holes: 6.3e-6    (pairs on = off = table form)

The closest call is 1.6e-4 (bar 2e-4): struct_gate_net.0.weight, bidirectional, rounds (0, 4), default GEMM — a [1, D] row whose
entries cancel like the bias beside it (kappa 178 there).  Nothing was refused or mishandled: the product accepts every one
of these batches, as the reference does, and a batch of edgeless graphs only gives the reference's empty output.

DDE (`ops.dde_node_struct`, both kernel forms) against float64: a feature of round k is a convex combination of values in
[0, 1] rounded once per round, so it may be off by k half-ulps of 1 = k * 2^-25; the bar per column is k * 2^-24.

    shape, rounds      kernel (both forms, equal)   share of the bar (worst column)   f32 oracle
    star (all three)   2.0e-8                       0.33                              2.0e-8
    hub  (4, 4)        9.6e-8                       0.69                              4.1e-6
    hub  (3, 1)        8.0e-8                       0.56                              4.1e-6
    hub  (0, 2)        8.3e-8                       0.69                              1.9e-7

Both kernel forms meet the derived bar everywhere.  On the hub rows the f32 ORACLE is 4.1e-6 from float64 (it adds a 6 667-entry
row in f32 in edge order): the atol=6e-6 of test_csr_dde_and_bfs_agree_with_the_oracle is the oracle's error, not the kernel's.
"""
import types

import numpy as np
import pytest
import torch

from oracle import graph as ograph
from tests import scorer_f64 as f64

pytestmark = pytest.mark.gpu

OUT_ATOL = 2e-4
GRAD_RTOL = {"f32": 2e-5, "default": 2e-4}
GEMMS = ["f32", "default"]
OUT_KEYS = ("logits", "logits_fwd", "logits_bwd", "edge_embeddings")


# ---- hand-built batches ------------------------------------------------------------------------------------------------
def _graph(n, triples=(), seeds=(0,), emb_ids=None):
    """One graph: n nodes, (head, relation, tail) triples with LOCAL node ids, local seed nodes, embedding ids (0 = non-text;
    default: all text)."""
    return dict(n=int(n), triples=[tuple(int(v) for v in t) for t in triples], seeds=list(seeds), emb_ids=emb_ids)


def _random_graph(rng, n, e, relations, seeds=(0,), emb_ids=None):
    """e random triples over n nodes: self loops and repeats are allowed to happen."""
    rel = np.asarray(relations)
    tri = [(rng.integers(n), rel[rng.integers(rel.size)], rng.integers(n)) for _ in range(e)]
    return _graph(n, tri, seeds, emb_ids)


def _assemble(graphs, D, seed, *, num_relation_rows=None):
    """The flat batch of a list of graphs (numpy; attribute names as a collated PyG batch / synthetic.SyntheticBatch).  The
    relation rows come from a table [R, D] (kept as `relation_table`), R = num_relation_rows or max id + 1."""
    rng = np.random.default_rng(seed)
    ptr, eptr, heads, tails, rels, topic, emb_ids = [0], [0], [], [], [], [], []
    for g in graphs:
        base = ptr[-1]
        for h, r, t in g["triples"]:
            assert 0 <= h < g["n"] and 0 <= t < g["n"]
            heads.append(base + h)
            tails.append(base + t)
            rels.append(r)
        seed_col = np.zeros(g["n"], np.float32)
        seed_col[list(g["seeds"])] = 1.0
        topic.append(np.stack([1.0 - seed_col, seed_col], axis=1))
        ids = g["emb_ids"] if g["emb_ids"] is not None else 1 + base + np.arange(g["n"])
        emb_ids.append(np.asarray(ids, np.int64).reshape(g["n"]))
        ptr.append(base + g["n"])
        eptr.append(eptr[-1] + len(g["triples"]))
    N, E, B = ptr[-1], eptr[-1], len(graphs)
    edge_attr = np.asarray(rels, np.int64)
    R = int(num_relation_rows) if num_relation_rows is not None else int(edge_attr.max()) + 1
    table = rng.standard_normal((R, D)).astype(np.float32)
    return types.SimpleNamespace(
        edge_index=np.stack([np.asarray(heads, np.int64), np.asarray(tails, np.int64)]), ptr=np.asarray(ptr, np.int64),
        edge_ptr=np.asarray(eptr, np.int64), edge_attr=edge_attr, topic_one_hot=np.concatenate(topic).astype(np.float32),
        node_embedding_ids=np.concatenate(emb_ids), question_emb=rng.standard_normal((B, D)).astype(np.float32),
        node_embeddings=rng.standard_normal((N, D)).astype(np.float32), relation_table=table,
        edge_embeddings=table[edge_attr], labels=(rng.random(E) < 0.3).astype(np.float32),
        gvec=rng.standard_normal(E).astype(np.float32), num_nodes=N, num_graphs=B)


def _empty_graphs_batch(D):
    """Graphs without edges first, last and two in a row after exactly 65 edges; a graph with nodes but no edges beside a
    single-edge graph.  Labels: graph 1 has no positive edge, graph 2 only positive ones."""
    rng = np.random.default_rng(101)
    rel = np.arange(9)
    graphs = [_graph(2, (), seeds=(1,)),
              _random_graph(rng, 10, 40, rel, seeds=(0, 3)),
              _random_graph(rng, 8, 25, rel, seeds=(2,)),
              _graph(1, (), seeds=(0,)),
              _graph(3, (), seeds=(0, 2), emb_ids=[0, 0, 0]),  # non-text nodes that no edge reads
              _random_graph(rng, 12, 50, rel, seeds=(5,), emb_ids=[0, 31, 32, 33, 0, 35, 36, 37, 38, 39, 40, 41]),
              _graph(4, (), seeds=(1,)),
              _graph(2, [(0, 4, 1)], seeds=(0,)),
              _random_graph(rng, 6, 20, rel, seeds=(0,)),
              _graph(2, (), seeds=(0,))]
    b = _assemble(graphs, D, seed=1)
    assert b.edge_ptr.tolist() == [0, 0, 40, 65, 65, 65, 115, 115, 116, 136, 136]
    b.labels[0:40] = 0.0
    b.labels[40:65] = 1.0
    b.labels[65:115] = (np.arange(50) % 4 == 0)
    b.edge_is_near = (np.arange(136) % 3 == 0)
    return b


def _loops_batch(D):
    """A one-node graph whose only edges are self loops under different relations; one triple three times; one (head, tail)
    pair under four relations; self loops mixed into an ordinary graph."""
    rng = np.random.default_rng(102)
    g3 = _random_graph(rng, 7, 18, np.arange(6), seeds=(1,))
    g3["triples"] += [(2, 0, 2), (2, 0, 2), (5, 3, 5)]
    graphs = [_graph(1, [(0, 0, 0), (0, 1, 0), (0, 5, 0)], seeds=(0,)),
              _graph(4, [(0, 2, 1), (1, 3, 2), (0, 2, 1), (2, 1, 3), (0, 2, 1)], seeds=(0,)),
              _graph(3, [(0, 0, 2), (0, 1, 2), (0, 4, 2), (0, 5, 2), (2, 4, 0)], seeds=(2,)),
              g3]
    return _assemble(graphs, D, seed=2)


def _seeds_batch(D):
    """A graph without a seed, a graph of seeds only, isolated nodes (some of them seeds) and a graph whose seed is isolated."""
    rng = np.random.default_rng(103)
    rel = np.arange(5)
    g_iso = _graph(9, [(0, 1, 1), (1, 2, 2), (2, 0, 0), (1, 3, 4), (4, 4, 1)], seeds=(0, 7))  # nodes 3, 5..8 touch no edge
    graphs = [_random_graph(rng, 6, 14, rel, seeds=()),
              _random_graph(rng, 5, 12, rel, seeds=(0, 1, 2, 3, 4)),
              g_iso,
              _graph(5, [(0, 0, 1), (1, 1, 2), (2, 2, 0)], seeds=(4,)),
              _random_graph(rng, 8, 20, rel, seeds=(3,))]
    b = _assemble(graphs, D, seed=3)
    assert b.topic_one_hot[:6, 1].sum() == 0 and b.topic_one_hot[6:11, 1].all()
    return b


def _non_text_batch(D, with_non_text):
    """with_non_text: every node of graph 1 has embedding id 0, graphs 0 and 2 have a few; else no id 0 anywhere."""
    rng = np.random.default_rng(104)
    rel = np.arange(6)
    ids0 = ids2 = None
    ids1 = np.arange(1, 7)
    if with_non_text:
        ids0 = np.asarray([5, 0, 7, 8, 0, 9, 11])
        ids1 = np.zeros(6, np.int64)
        ids2 = np.asarray([0, 21, 22, 23, 24])
    graphs = [_random_graph(rng, 7, 22, rel, seeds=(0,), emb_ids=ids0),
              _random_graph(rng, 6, 17, rel, seeds=(2,), emb_ids=ids1),
              _random_graph(rng, 5, 15, rel, seeds=(1,), emb_ids=ids2)]
    b = _assemble(graphs, D, seed=4)
    assert bool((b.node_embedding_ids == 0).any()) == with_non_text
    return b


def _relation_batch(kind, D):
    """holes: ids from {0, 7, E - 1} only (most rows of the de-duplicated table unused); per_edge: inside a graph every edge
    has its own relation, so the (relation, graph) pair count is E; beyond: one id >= E (de-duplication switches itself off)."""
    rng = np.random.default_rng(105)
    shapes = [(6, 15), (1, 2), (7, 19), (5, 12)]
    E = sum(e for _, e in shapes)
    graphs = []
    for n, e in shapes:
        if kind == "holes":
            g = _random_graph(rng, n, e, [0, 7, E - 1])
        elif kind == "per_edge":
            g = _random_graph(rng, n, e, [0])
            g["triples"] = [(h, i, t) for i, (h, _, t) in enumerate(g["triples"])]
        else:
            g = _random_graph(rng, n, e, np.arange(5))
        graphs.append(g)
    if kind == "beyond":
        h, _, t = graphs[2]["triples"][4]
        graphs[2]["triples"][4] = (h, E + 3, t)
    b = _assemble(graphs, D, seed=5, num_relation_rows=E if kind == "holes" else None)
    assert b.edge_attr.size == E
    if kind == "holes":
        assert set(b.edge_attr.tolist()) == {0, 7, E - 1}
    if kind == "per_edge":
        eb = np.repeat(np.arange(len(shapes)), np.diff(b.edge_ptr))
        assert np.unique(eb * E + b.edge_attr).size == E
    if kind == "beyond":
        assert b.edge_attr.max() >= E
    return b


def _tiny_graphs(rng, count):
    """`count` graphs of 1-4 nodes and 0-3 edges (the edge count cycles through 0, 1, 2, 3)."""
    return [_random_graph(rng, 1 + int(rng.integers(4)), i % 4, np.arange(4), seeds=(0,)) for i in range(count)]


def _count_batch(kind, D):
    """one: B = 1; b33: 33 tiny graphs; b40_star: 39 tiny graphs with a 300-edge star into one node in their middle."""
    rng = np.random.default_rng(106)
    if kind == "one":
        graphs = [_random_graph(rng, 9, 30, np.arange(5), seeds=(0, 4))]
    elif kind == "b33":
        graphs = _tiny_graphs(rng, 33)
    else:
        graphs = _tiny_graphs(rng, 39)
        star = _graph(301, [(1 + i, i % 3, 0) for i in range(300)], seeds=(0, 17))
        graphs.insert(20, star)
    return _assemble(graphs, D, seed=6)


# ---- running the product and the float64 model ---------------------------------------------------------------------------
def _to_device(b, dev, *, table_form=False):
    ns = types.SimpleNamespace()
    for k in ("edge_index", "ptr", "edge_attr", "topic_one_hot", "node_embedding_ids", "question_emb", "node_embeddings"):
        setattr(ns, k, torch.from_numpy(getattr(b, k)).to(dev))
    if table_form:
        ns.relation_embedding_table = torch.from_numpy(b.relation_table).to(dev)
        ns.num_relations = int(b.relation_table.shape[0])
    else:
        ns.edge_embeddings = torch.from_numpy(b.edge_embeddings).to(dev)
    ns.num_nodes, ns.num_graphs = b.num_nodes, b.num_graphs
    return ns


def _make_model(D, H, rounds, mode, **kw):
    from evi_rag_amd.retriever import Retriever

    torch.manual_seed(1000 * D + 10 * H + rounds[0])
    m = Retriever(emb_dim=D, hidden_dim=H, dde_cfg={"num_rounds": rounds[0], "num_reverse_rounds": rounds[1]},
                  direction_mode=mode, **kw)
    with torch.no_grad():  # biases and LayerNorm vectors away from their 0 / 1 initial values
        for p in m.parameters():
            if p.dim() == 1:
                p.add_(0.1 * torch.randn_like(p))
    return m


# A gradient is a sum over the edges, g_p = sum_e c_e with c_e = dscalar/dlogit_e * dlogit_e/dp.  Float64 autograd gives the
# terms as well, hence A_p = max over the entries of sum_e |c_e|, the size of what the kernel actually adds up.
#  * No term at all (A_p == 0: non_text_entity_emb without a non-text node): the kernel's gradient must be exactly zero.
#  * "Within X of the gradient's max" judges a kernel while the sum is well conditioned.  A matrix or vector gradient has
#    well-conditioned entries whatever the draw.  A ONE-ELEMENT gradient (struct_gate_net.0.bias, score_head.bias) is a single
#    sum of ~E terms of either sign and may cancel a few hundred times; its own value then says nothing about the error an
#    f32 kernel can reach.  What the arithmetic promises is relative to the terms: a split-bf16 product carries 2^-16 per
#    term (three bf16 products of hi + lo operands, the lo * lo product dropped), so a sum carries up to 2^-16 A_p, and the
#    2e-4 bar equals that promise at the condition number KAPPA = A_p / |g_p| = 2e-4 / 2^-16 = 13.1.  A one-element gradient
#    is therefore held to rtol * max(|g_p|, A_p / KAPPA): the issue's bar as it stands up to KAPPA, the same bar expressed
#    in the terms beyond it (2^-16 A_p for the default GEMM, a tenth of that for the f32 GEMM).
#  * A gradient that float64 itself cannot tell from zero (0 < max |g_p| <= 1e-9 A_p) is zero by an invariance — InfoNCE does
#    not change when all logits of a graph move together, so d/d score_head.bias = d/d state_net.4.bias = 0 — and f32 returns
#    the rounding of the sum instead: each of the E terms rounded a few times (8 allowed) and added in f32 in some order,
#    |error| <= (E + 8) * 2^-24 * A_p.  That absolute bound replaces the relative bar for such a gradient.
KAPPA = 2e-4 / 2.0 ** -16
CANCELLED = 1e-9

_REFERENCE = {}


def _float64_outputs(model, b, rounds, mode):
    """(leaf weights, float64 forward) of the model on batch b."""
    w = f64.leaf_weights(model.state_dict())
    return w, f64.retriever_forward(w, b, num_rounds=rounds[0], num_reverse_rounds=rounds[1], direction_mode=mode)


def _float64_run(model, b, rounds, mode, loss_cfg):
    w, out = _float64_outputs(model, b, rounds, mode)
    if loss_cfg is None:
        scalar = (out["logits"] * torch.from_numpy(b.gvec).double()).sum()
    else:
        scalar = f64.retriever_loss(out["logits"], b.labels, out["query_ids"], b.num_graphs, edge_is_near=b.edge_is_near, **loss_cfg)
    (dl,) = torch.autograd.grad(scalar, out["logits"], retain_graph=True)
    names = list(w)
    terms = torch.autograd.grad(out["logits"], [w[n] for n in names], grad_outputs=torch.diag(dl), is_grads_batched=True,
                                allow_unused=True)  # [E, *shape] per parameter: the c_e
    ref = {k: None if out[k] is None else out[k].detach().numpy() for k in OUT_KEYS}
    # a parameter outside the float64 graph has no term: gradient zero, A_p = 0
    ref["grads"] = {n: np.zeros(tuple(w[n].shape)) if t is None else t.sum(dim=0).numpy() for n, t in zip(names, terms)}
    ref["terms_abs"] = {n: 0.0 if t is None else float(t.abs().sum(dim=0).max()) for n, t in zip(names, terms)}
    ref["scalar"] = float(scalar.detach())
    ref["E"] = int(dl.numel())
    return ref


def _cancelled(ref, name):
    return 0.0 < ref["terms_abs"][name] and float(np.abs(ref["grads"][name]).max()) <= CANCELLED * ref["terms_abs"][name]


def _reference(key, b, D, H, rounds, mode, loss_cfg=None):
    """Float64 outputs, gradients and term sums for a case: computed once per key and shared, read-only, between the GEMM modes
    / chunk sizes / kernel switches that must all reproduce it."""
    if key not in _REFERENCE:
        ref = _float64_run(_make_model(D, H, rounds, mode), b, rounds, mode, loss_cfg)
        for arr in [v for v in ref.values() if isinstance(v, np.ndarray)] + list(ref["grads"].values()):
            arr.setflags(write=False)
        _REFERENCE[key] = ref
    return _REFERENCE[key]


def _set_gemm(monkeypatch, gemm):
    if gemm == "f32":
        monkeypatch.setenv("EVI_SCORER_GEMM", "f32")
    else:
        monkeypatch.delenv("EVI_SCORER_GEMM", raising=False)


def _compare_outputs(tag, out, ref):
    errs = {}
    for k in OUT_KEYS:
        got = getattr(out, k)
        if ref[k] is None:
            assert got is None, k
            continue
        got = got.detach().cpu().numpy()
        assert got.shape == ref[k].shape, k
        errs[k] = float(np.abs(got - ref[k]).max()) if got.size else 0.0
    for k, e in errs.items():
        assert e <= OUT_ATOL, (tag, k, e)
    return max(errs.values())


def _compare(tag, gemm, out, model, ref, label="degenerate"):
    """Outputs and all 25 gradients of the product against the float64 reference (the rules above KAPPA); prints the worst
    figures, then asserts."""
    ratios, one_element, must_be_zero, cancelled = {}, {}, {}, {}
    for name, p in model.named_parameters():
        want, terms_abs = ref["grads"][name], ref["terms_abs"][name]
        assert p.grad is not None, name
        got = p.grad.detach().cpu().numpy()
        assert got.shape == want.shape, name
        err, scale = float(np.abs(got - want).max()), float(np.abs(want).max())
        if terms_abs == 0.0:
            must_be_zero[name] = float(np.abs(got).max())
        elif _cancelled(ref, name):
            cancelled[name] = err / ((ref["E"] + 8) * 2.0 ** -24 * terms_abs)
        elif want.size == 1:
            one_element[name] = (err / max(scale, terms_abs / KAPPA, 1e-6), terms_abs / scale)
        else:
            ratios[name] = err / max(scale, 1e-6)
    assert len(ratios) + len(one_element) + len(must_be_zero) + len(cancelled) == 25
    top = max(ratios, key=ratios.get)
    print(f"\n[{label}] {tag} gemm={gemm}: grad {ratios[top]:.1e} ({top})"
          + "".join(f"  {n}: {r:.1e} at kappa {k:.0f}" for n, (r, k) in one_element.items())
          + "".join(f"  {n} cancelled: {r:.1e} of its bound" for n, r in cancelled.items()))
    worst_out = _compare_outputs(tag, out, ref)
    print(f"[{label}] {tag} gemm={gemm}: out {worst_out:.1e}")
    for name, got_max in must_be_zero.items():
        assert got_max == 0.0, (tag, name, "no term in float64", got_max)
    for name, r in cancelled.items():
        assert np.isfinite(r) and r <= 1.0, (tag, name, "zero by invariance", r)
    for name, (r, _) in one_element.items():
        assert np.isfinite(r) and r <= GRAD_RTOL[gemm], (tag, name, "one element", r)
    for name, r in ratios.items():
        assert np.isfinite(r) and r <= GRAD_RTOL[gemm], (tag, name, r)


def _run_gvec(dev, tag, gemm, monkeypatch, b, D, H, *, rounds=(2, 2), mode="bidirectional", table_form=False, keep=True,
              ref_key=None, label="degenerate", **model_kw):
    """The product's eval-mode graph on batch b: d (logits . gvec) / d parameter, against the float64 model."""
    _set_gemm(monkeypatch, gemm)
    ref = _reference(ref_key or (tag, D, H, rounds, mode), b, D, H, rounds, mode)
    model = _make_model(D, H, rounds, mode, **model_kw).to(dev).eval()
    model.differentiable = True
    model.keep_forward_intermediates = keep
    out = model(_to_device(b, dev, table_form=table_form))
    assert out.logits.requires_grad
    (out.logits * torch.from_numpy(b.gvec).to(dev)).sum().backward()
    torch.cuda.synchronize()
    assert np.array_equal(out.query_ids.cpu().numpy(), np.repeat(np.arange(b.num_graphs), np.diff(b.edge_ptr)))
    _compare(tag, gemm, out, model, ref, label=label)
    return model


# ---- the cases ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("gemm", GEMMS)
@pytest.mark.parametrize("keep", [True, False], ids=["replay", "recompute"])
@pytest.mark.parametrize("chunk", [None, 65, 64], ids=["one-chunk", "chunk-ends-on-empty-run", "chunk-ends-one-edge-before"])
def test_graphs_without_edges(dev, monkeypatch, gemm, keep, chunk):
    """edge_ptr[g] == edge_ptr[g + 1] for the first graph, the last, two in a row and one beside a single-edge graph; the two
    in a row start at edge 65, so EVI_EDGE_CHUNK = 65 ends a chunk exactly on them and 64 one edge before."""
    if chunk is None:
        monkeypatch.delenv("EVI_EDGE_CHUNK", raising=False)
    else:
        monkeypatch.setenv("EVI_EDGE_CHUNK", str(chunk))
    b = _empty_graphs_batch(16)
    _run_gvec(dev, f"empty chunk={chunk} keep={keep}", gemm, monkeypatch, b, 16, 32, keep=keep, ref_key=("empty", 16, 32))


@pytest.mark.parametrize("gemm", GEMMS)
def test_self_loops_and_parallel_edges(dev, monkeypatch, gemm):
    _run_gvec(dev, "loops", gemm, monkeypatch, _loops_batch(32), 32, 16)


@pytest.mark.parametrize("gemm", GEMMS)
def test_graphs_without_seeds_of_seeds_only_and_isolated_nodes(dev, monkeypatch, gemm):
    _run_gvec(dev, "seeds", gemm, monkeypatch, _seeds_batch(16), 16, 16, rounds=(3, 1))


@pytest.mark.parametrize("gemm", GEMMS)
@pytest.mark.parametrize("with_non_text", [True, False], ids=["a-graph-of-non-text-nodes", "no-non-text-node"])
def test_non_text_nodes_everywhere_and_nowhere(dev, monkeypatch, gemm, with_non_text):
    """Without any embedding id 0 the float64 gradient of non_text_entity_emb.weight is identically zero: the kernel's must be
    exactly zero (the rule in _compare); with a graph of non-text nodes only it is not."""
    b = _non_text_batch(32, with_non_text)
    model = _run_gvec(dev, f"non_text={with_non_text}", gemm, monkeypatch, b, 32, 32)
    g = model.non_text_entity_emb.weight.grad
    assert bool((g == 0).all()) == (not with_non_text)


@pytest.mark.parametrize("gemm", GEMMS)
@pytest.mark.parametrize("kind,variant", [("holes", "ids"), ("holes", "table"), ("per_edge", "ids"), ("per_edge", "table"),
                                          ("beyond", "ids"), ("holes", "no-dedupe"), ("per_edge", "no-dedupe")])
def test_relation_id_ranges(dev, monkeypatch, gemm, kind, variant):
    """ids: the relation table is inferred from edge_attr (max id + 1 rows, or none when an id >= E); table: the batch hands
    over `relation_embedding_table` + `num_relations` (rows that no edge uses are projected too; a wrong gradient for one
    would show in relation_proj's weight and bias gradients, which must match float64); no-dedupe: dedupe_relations=False.
    One float64 reference per kind: every variant computes the same function.  These runs keep per-edge relation-context rows
    (a backward follows); the (relation, graph) pair rows are judged by test_relation_graph_pair_rows_forward."""
    monkeypatch.delenv("EVI_SCORER_PAIRS", raising=False)
    b = _relation_batch(kind, 16)
    kw = {"dedupe_relations": False} if variant == "no-dedupe" else {}
    _run_gvec(dev, f"relations {kind}/{variant}", gemm, monkeypatch, b, 16, 32, table_form=(variant == "table"),
              ref_key=("relations", kind), **kw)


def _pair_batch(kind, D):
    """1 112 edges in 5 graphs among 4 edgeless ones (first, two in a row, last) and a one-node graph of two self loops.
    per_edge: inside a graph edge i has relation i, so the number of (relation, graph) pairs is E; holes: ids from
    {0, 7, E - 1} only, so nearly every entry of the [B, R] pair table stays empty."""
    rng = np.random.default_rng(107)
    shapes = [(2, 0), (40, 300), (1, 0), (3, 0), (30, 280), (1, 2), (50, 330), (25, 200), (2, 0)]
    E = sum(e for _, e in shapes)
    graphs = []
    for n, e in shapes:
        g = _random_graph(rng, n, e, [0, 7, E - 1])
        if kind == "per_edge":
            g["triples"] = [(h, i, t) for i, (h, _, t) in enumerate(g["triples"])]
        graphs.append(g)
    b = _assemble(graphs, D, seed=8, num_relation_rows=E if kind == "holes" else None)
    eb = np.repeat(np.arange(len(shapes)), np.diff(b.edge_ptr))
    pairs = np.unique(eb * E + b.edge_attr).size
    assert E == 1112 and (pairs == E if kind == "per_edge" else pairs <= 3 * 5)
    return b


@pytest.mark.parametrize("variant", ["pairs-on", "pairs-off", "pairs-on-table"])
@pytest.mark.parametrize("kind", ["per_edge", "holes"])
def test_relation_graph_pair_rows_forward(dev, monkeypatch, kind, variant):
    """The forward multiplies the relation context by state_net.0's block once per distinct (relation, graph) pair and looks
    the row up per edge — only with the default GEMM, from 1 024 edges on, and only when no backward follows (the backward and
    the forward that keeps its activations use per-edge rows: csrc/scorer.hip, fwd_layout / pair_max and Run::pairs).  So no
    gradient run of this file reaches the pair rows, whatever EVI_SCORER_PAIRS says; this one does: evaluation, default GEMM,
    E = 1 112, with the pair count equal to E, with holes in the id range, and with edgeless graphs (pair count 0) first, last
    and in a row — with the pair rows, with EVI_SCORER_PAIRS=0 and through the relation table, all four outputs against
    float64.  That the switch selects another layout at this size, and none at the gradient runs' sizes, is read off the
    workspace the library asks for (the pair table and rows are part of it)."""
    from evi_rag_amd import _lib

    monkeypatch.delenv("EVI_SCORER_GEMM", raising=False)
    monkeypatch.delenv("EVI_EDGE_CHUNK", raising=False)
    D, H, rounds, mode = 16, 16, (2, 2), "bidirectional"
    b = _pair_batch(kind, D)
    key = ("pairs", kind)
    if key not in _REFERENCE:
        _, out64 = _float64_outputs(_make_model(D, H, rounds, mode), b, rounds, mode)
        _REFERENCE[key] = {k: out64[k].detach().numpy() for k in OUT_KEYS}
    lib = _lib.load()

    def workspace(bb, pairs):
        monkeypatch.setenv("EVI_SCORER_PAIRS", "1" if pairs else "0")
        R = int(bb.edge_attr.max()) + 1
        return int(lib.evi_retriever_forward_workspace_bytes(bb.num_nodes, bb.edge_attr.size, bb.num_graphs, D, H, 2, 2, R))

    assert workspace(b, True) > workspace(b, False)
    small = _relation_batch(kind, D)
    assert workspace(small, True) == workspace(small, False)

    monkeypatch.setenv("EVI_SCORER_PAIRS", "0" if variant == "pairs-off" else "1")
    model = _make_model(D, H, rounds, mode).to(dev).eval()
    with torch.no_grad():
        out = model(_to_device(b, dev, table_form=variant.endswith("table")))
    torch.cuda.synchronize()
    assert not out.logits.requires_grad
    worst = _compare_outputs(f"pair rows {kind}/{variant}", out, _REFERENCE[key])
    print(f"\n[degenerate] pair rows {kind}/{variant}: out {worst:.1e}")


@pytest.mark.parametrize("gemm", GEMMS)
@pytest.mark.parametrize("kind", ["one", "b33", "b40_star"])
def test_graph_counts_around_the_skinny_kernel(dev, monkeypatch, gemm, kind):
    """B = 1, and B = 33 / 40 tiny graphs of 0-3 edges (the question-side products leave the 32-row skinny kernel), the
    latter with a 300-edge star into one node."""
    _run_gvec(dev, f"counts {kind}", gemm, monkeypatch, _count_batch(kind, 32), 32, 32)


@pytest.mark.parametrize("gemm", GEMMS)
@pytest.mark.parametrize("rounds", [(0, 4), (4, 0), (3, 1)], ids=lambda r: f"rounds{r[0]}{r[1]}")
@pytest.mark.parametrize("mode", ["forward", "backward", "bidirectional"])
def test_direction_modes_and_one_sided_rounds(dev, monkeypatch, gemm, rounds, mode):
    _run_gvec(dev, f"modes {mode} {rounds}", gemm, monkeypatch, _empty_graphs_batch(16), 16, 16, rounds=rounds, mode=mode)


@pytest.mark.parametrize("gemm", GEMMS)
@pytest.mark.parametrize("loss_cfg", [dict(infonce_temperature=0.5),
                                      dict(infonce_temperature=1.0, infonce_weight=0.5, bce_weight=1.0, edge_weight_near=2.0,
                                           edge_weight_bridge=0.5)], ids=["infonce", "infonce+bce+edge-weights"])
def test_loss_chain_on_the_empty_graph_batch(dev, monkeypatch, gemm, loss_cfg):
    """train() mode (dropout_p = 0, hide-and-seek off): RetrieverLoss(...)(out, labels, ...).loss.backward() against the
    float64 forward + float64 loss.  Graph 1 has no positive edge and graph 2 only positive ones (both outside InfoNCE), five
    graphs have no edge (outside both terms).  The loss value: |lse(s) - lse(s')| <= max |s - s'| and BCE is 1-Lipschitz in
    the logit, so outputs within 2e-4 bound it by w_infonce * 2 * 2e-4 / T + w_bce * 2e-4 (f32 rounding of an O(1) value,
    ~1e-6, is far below that)."""
    from evi_rag_amd.loss import RetrieverLoss

    _set_gemm(monkeypatch, gemm)
    monkeypatch.delenv("EVI_EDGE_CHUNK", raising=False)
    D, H, rounds, mode = 16, 32, (2, 2), "bidirectional"
    b = _empty_graphs_batch(D)
    ref = _reference(("loss", tuple(sorted(loss_cfg.items()))), b, D, H, rounds, mode, loss_cfg=loss_cfg)
    model = _make_model(D, H, rounds, mode, dropout_p=0.0, hide_seek_cfg={"enabled": False}).to(dev).train()
    out = model(_to_device(b, dev))
    near = torch.from_numpy(b.edge_is_near).to(dev)
    res = RetrieverLoss(**loss_cfg)(out, torch.from_numpy(b.labels).to(dev), edge_batch=out.query_ids, num_graphs=b.num_graphs,
                                    edge_is_near=near)
    res.loss.backward()
    torch.cuda.synchronize()
    err = abs(float(res.loss.detach()) - ref["scalar"])
    bound = loss_cfg.get("infonce_weight", 1.0) * 2 * OUT_ATOL / loss_cfg["infonce_temperature"] + loss_cfg.get("bce_weight", 0.0) * OUT_ATOL
    print(f"\n[degenerate] loss {sorted(loss_cfg)} gemm={gemm}: loss {ref['scalar']:.6f} off by {err:.1e} (bound {bound:.1e})")
    assert ref["scalar"] > 0.1 and err <= bound, (err, bound)
    _compare(f"loss {'+bce' if 'bce_weight' in loss_cfg else 'infonce'}", gemm, out, model, ref)


def test_batch_of_edgeless_graphs_only_gives_the_empty_output(dev):
    """E = 0 for the whole batch: the reference returns empty logits / directional logits / [0, H] features and no relation
    ids before it looks at anything else (retriever.py: _empty_output); so does the product, in eval and in train mode."""
    b = _assemble([_graph(2, ()), _graph(1, ()), _graph(3, ())], 16, seed=7, num_relation_rows=1)
    for train in (False, True):
        model = _make_model(16, 32, (2, 2), "bidirectional", dropout_p=0.0).to(dev).train(train)
        out = model(_to_device(b, dev))
        assert out.logits.shape == (0,) and out.logits_fwd.shape == (0,) and out.logits_bwd.shape == (0,)
        assert out.edge_embeddings.shape == (0, 32) and out.query_ids.shape == (0,) and out.relation_ids is None
        assert model.extract_edge_tokens(_to_device(b, dev)).shape == (0, 32)


# ---- DDE against float64 ---------------------------------------------------------------------------------------------------
def _hub_shape():
    """The batch of test_retriever_gpu.test_csr_dde_and_bfs_agree_with_the_oracle: tiny graphs, hubs (a third of a graph's
    edges end in its node 0), a graph without edges, graphs beyond the CSR build's LDS budget."""
    rng = np.random.default_rng(5)
    sizes = [(40, 90), (3000, 10000), (1, 0), (7000, 9000), (64, 4000), (500, 1), (300, 20000), (9000, 12000), (8192, 14336)]
    ei, ptr, eptr = [], [0], [0]
    for n, e in sizes:
        s = rng.integers(0, n, e)
        d = rng.integers(0, n, e)
        if e > 100:
            d[: e // 3] = 0
        ei.append(np.stack([s, d]) + ptr[-1])
        ptr.append(ptr[-1] + n)
        eptr.append(eptr[-1] + e)
    topic = np.zeros((ptr[-1], 2), np.float32)
    topic[:, 1] = 1.0
    topic[np.asarray([ptr[g] + (0 if n < 3 else 2) for g, (n, _) in enumerate(sizes)])] = [1.0, 0.0]
    return np.concatenate(ei, axis=1).astype(np.int64), np.asarray(ptr, np.int64), np.asarray(eptr, np.int64), topic


@pytest.mark.parametrize("shape", ["star", "hub"])
def test_dde_features_against_float64(dev, monkeypatch, shape):
    """`ops.dde_node_struct` in both kernel forms against the float64 features, column by column: round k within k * 2^-24.
    The f32 oracle's own distance to float64 on the same rows is measured beside it: the oracle sums a row in f32 in edge
    order, so on hub rows it is the oracle, not the kernel, that needs test_csr_dde_and_bfs_agree_with_the_oracle's 6e-6."""
    from evi_rag_amd import ops

    if shape == "star":
        b = _count_batch("b40_star", 16)
        ei, ptr, eptr, topic = b.edge_index, b.ptr, b.edge_ptr, b.topic_one_hot
    else:
        ei, ptr, eptr, topic = _hub_shape()
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    csr = ops.graph_csr(t(ei), t(ptr), t(eptr))
    for rounds in [(4, 4), (3, 1), (0, 2)]:
        want = f64.node_structure_features(topic, ei, *rounds).numpy()
        depth = np.asarray([0] + list(range(1, rounds[0] + 1)) + list(range(1, rounds[1] + 1)), np.float64)
        bar = np.tile(depth, 2) * 2.0 ** -24  # topic-major columns: [topic c][feature]
        oracle = np.abs(ograph.node_structure_features(topic, ei, *rounds).astype(np.float64) - want).max(axis=0)
        for form in ("nodes", "graph"):
            monkeypatch.setenv("EVI_DDE_MODE", form)
            got = ops.dde_node_struct(t(topic), t(ptr), csr, *rounds).cpu().numpy().astype(np.float64)
            err = np.abs(got - want).max(axis=0)
            print(f"\n[degenerate] dde {shape} rounds={rounds} form={form}: kernel {err.max():.1e} "
                  f"(worst column at {float((err / np.maximum(bar, 2.0 ** -24)).max()):.2f} of its bar)  f32 oracle {oracle.max():.1e}")
            assert (err <= bar).all(), (shape, rounds, form, err.tolist(), bar.tolist())
        assert oracle.max() <= 6e-6
        if shape == "hub":  # the f32 oracle itself is outside the kernel's bar there
            assert oracle.max() > bar.max(), (rounds, oracle.max(), bar.max())
