"""GPU: the edge scorer's forward and all 25 parameter gradients against the float64 model, entry by entry, where the narrow
degenerate batches do not reach: WIDE widths, TRAINING-MODE DROPOUT and the ROW-COUNT SEAMS of the weight-gradient products.

tests/test_scorer_degenerate_gpu.py judges every gradient entry against float64, but at D = 16 / 32, H = 16 / 32 and a few
hundred edges: every per-edge kernel is then its one-column-group instantiation and every host-side switch on a row count
takes its first branch.  Here:

 * widths — the per-edge kernels are templated on ceil(width / 256) = 1..5 sixteen-byte column groups per lane, separately for
   D and H (EVI_DPL_DISPATCH; C4 of k_combine_bwd / k_edge_struct_bwd / k_edge_translate_bwd; the 256-column blocks of
   k_node_gather_grad, k_colsum_partial, k_segment_rowsum*).  Eight (D, H) pairs, one per seam of that split (the
   parametrize ids say which), eval-mode graph, both GEMM modes, rounds (2, 2); two of them in the single-direction modes
   and one with the recomputing backward as well.
 * dropout — train() mode, dropout_p = 0.25: the kernel's mask restated from the seed (scorer_f64._dropout_multipliers) is part
   of the float64 reference, so every gradient entry under dropout is judged, in the three direction modes, and with
   EVI_EDGE_CHUNK = 64 (six chunks) against the same reference: the mask row is direction * E + e with the BATCH's e and E.
   One case adds hide-and-seek with p_near = p_far = 1 (a deterministic bias on every edge).
 * row counts at D = 16, H = 32 — `tn_gemm` is exact f32 for K <= 64 rows and split-K beyond, `colsum_into` one block up to
   256 rows and two stages beyond, the segment sums cut a segment into Z = (rows / segments + 255) / 256 slices; K is B on
   the question side, N on the entity side, R (relation table) or E on the relation side and the chunk's edges for the
   state net (csrc/scorer.hip: chunk_backward, batch_backward).  Hand-built batches on both sides of each seam, with
   dedupe_relations off where only then a product runs over E rows (test_row_count_seams says which count feeds what).

Reference: tests/scorer_f64.py.  Bars and rules: those of test_scorer_degenerate_gpu (outputs 2e-4 absolute; gradients within
2e-5 / 2e-4 (f32 / default GEMM) of the gradient's float64 max, 1e-6 floor; one-element gradients rtol * max(|g|, A_p / KAPPA);
no term in float64 means exactly zero), through its `_compare`.  At the wide widths the per-edge term tensors of
`_float64_run` would be E x 5 M doubles, so the reference there is plain reverse mode, and the term sums A_p are computed only
where a rule reads them: for the two one-element parameters by one forward-mode pass each (sum_e |gvec_e d logit_e / d p|), for
non_text_entity_emb by whether any node is non-text; every other gradient carries max |g| (a lower bound of its A_p, never 0
here — asserted) in that slot.  The row-count cases are narrow and use `_float64_run` as it is.

Measured on an MI355X, f32 GEMM / default GEMM — worst output error; worst gradient ratio of the matrix and vector gradients;
worst ratio of the two one-element gradients under their rule (largest condition number met):

    case                                                outputs            gradients          one-element (kappa)
    widths, eval graph, bidirectional
      4 x 4                                             2.6e-7 / 9.5e-6    1.6e-6 / 3.7e-5    3.5e-7 / 6.8e-6  (23)
      256 x 260                                         8.9e-7 / 8.0e-6    1.2e-6 / 1.4e-5    8.2e-7 / 2.8e-7  (24)
      252 x 512                                         1.6e-6 / 8.4e-6    2.9e-6 / 1.5e-5    2.0e-7 / 1.3e-5  (57)
      768 x 768 (replay = recompute)                    1.8e-6 / 8.6e-6    1.6e-6 / 1.2e-5    1.1e-7 / 8.0e-6  (24)
      1024 x 1100                                       2.4e-6 / 9.5e-6    2.6e-6 / 1.3e-5    5.7e-7 / 3.0e-6  (24)
      1280 x 1276                                       3.0e-6 / 8.2e-6    2.6e-6 / 1.3e-5    2.0e-7 / 8.6e-7  (60)
      1276 x 16                                         4.2e-7 / 7.2e-6    1.7e-6 / 1.4e-5    1.3e-6 / 8.9e-6  (15)
      16 x 1280                                         2.1e-6 / 9.6e-6    2.0e-6 / 1.7e-5    1.0e-7 / 3.3e-6  (15)
    widths, single direction
      1024 x 1100 forward / backward (worst)            2.8e-6 / 1.3e-5    2.3e-6 / 2.3e-5    5.5e-7 / 1.2e-5  (25)
      256 x 260 forward / backward (worst)              1.3e-6 / 1.1e-5    1.3e-6 / 1.8e-5    4.1e-7 / 4.3e-6  (56)
    dropout 0.25, train()
      16 x 32 (one chunk = six chunks, replay = recompute)
                                                        3.8e-7 / 8.9e-6    1.2e-6 / 2.3e-5    1.3e-7 / 7.1e-6  (89)
      260 x 1100 (one chunk = six chunks, replay = recompute)
                                                        2.2e-6 / 9.8e-6    2.1e-6 / 1.3e-5    8.8e-8 / 6.7e-6  (27)
      768 x 768                                         1.9e-6 / 9.6e-6    1.7e-6 / 3.9e-5    2.2e-7 / 1.6e-5  (139)
      16 x 32 forward / backward (worst)                4.3e-7 / 1.1e-5    1.1e-6 / 1.4e-5    4.0e-7 / 7.6e-6  (23)
      16 x 32 with hide-and-seek on every edge          3.8e-7 / 8.9e-6    1.3e-6 / 2.5e-5    3.8e-7 / 7.1e-6  (89)
    row counts, 16 x 32 (what each straddles: the parametrize ids and test_row_count_seams)
      E = 1                                             1.1e-7 / 1.1e-7    4.5e-7 / 4.5e-7    6.6e-8 / 6.6e-8  (1)
      E = 32 | 33                                       2.5e-7 / 6.3e-6    2.2e-6 / 3.7e-5    7.2e-7 / 1.9e-6  (33)
      E = 64 | 65                                       3.4e-7 / 7.0e-6    1.2e-6 / 3.7e-5    6.8e-7 / 2.9e-5  (28)
      E = 64 | 65, dedupe_relations=False               3.4e-7 / 6.9e-6    8.7e-7 / 4.1e-5    1.1e-7 / 3.1e-5  (28)
      E = 252 | 253                                     3.5e-7 / 8.0e-6    6.9e-7 / 1.4e-5    5.2e-7 / 3.4e-6  (67)
      E = 256 | 257                                     3.4e-7 / 9.2e-6    1.8e-6 / 1.7e-5    4.8e-7 / 1.8e-6  (42)
      E = 256 | 257, dedupe_relations=False             3.0e-7 / 9.0e-6    2.3e-6 / 1.7e-5    5.4e-7 / 1.6e-6  (42)
      B = 2 with 1 and 513 edges                        3.5e-7 / 9.5e-6    1.1e-6 / 1.5e-5    1.7e-7 / 1.4e-6  (293)
      the same, dedupe_relations=False                  4.6e-7 / 9.6e-6    2.3e-6 / 3.3e-5    1.1e-7 / 3.4e-6  (293)
      B = 64 | 65                                       3.4e-7 / 8.1e-6    4.6e-7 / 1.1e-5    3.2e-7 / 3.4e-6  (26)
      B = 256 | 257 (one edge each)                     4.0e-7 / 9.2e-6    1.6e-6 / 2.6e-5    5.0e-7 / 7.3e-6  (99)
      N = 64 | 65                                       3.6e-7 / 8.6e-6    2.2e-6 / 6.7e-5    7.8e-7 / 1.7e-5  (35)
      N = 256 | 257                                     3.3e-7 / 7.6e-6    8.7e-7 / 6.3e-5    1.1e-7 / 1.4e-5  (451)
      R = 64 | 65 (table)                               3.1e-7 / 7.9e-6    1.1e-6 / 1.5e-5    2.2e-7 / 4.2e-6  (28)
      R = 2 over 600 edges (table)                      3.0e-7 / 6.5e-6    1.4e-6 / 2.2e-5    1.0e-7 / 2.0e-6  (62)

Every bar holds with room at every width: the outputs do not drift with the width under the default GEMM (8e-6 .. 1.3e-5 from
4 to 1280), and the closest call of the file is 6.7e-5 (bar 2e-4): struct_gate_net.0.weight at N = 64, default GEMM, a [1, D]
row that cancels like the bias beside it.  No rule beyond the existing ones was needed and no defect was found: the six-chunk
dropout runs return the one-chunk figures, the replaying and the recomputing backward the same ones.

That the file can fail was shown once with two arithmetic-only changes of csrc/scorer_bwd.hpp (no address or bound touched):
 (a) k_combine_bwd takes dropout multipliers of all ones: all 20 dropout cases here fail (and so do the five widths of
     test_backward_at_wide_dims_matches_finite_differences, which runs with dropout, and
     test_training_mode_dropout_and_hide_and_seek);
 (b) k_combine_bwd leaves the last column group out of the state_net.1.bias sum when C4 > 1: every case here with H > 256
     fails — 30: all widths but 4 x 4 and 1276 x 16, the single-direction and recompute runs, dropout at 260 x 1100 and
     768 x 768 — and none with H <= 256; of the five widths of the finite-difference test only 768 x 768 notices
     (320 x 256 has one group; 1024, 1280 and 256 x 1100 pass with up to a quarter of that gradient vector missing).
"""
import types

import numpy as np
import pytest
import torch
import torch.autograd.forward_ad as fwad

from evi_rag_amd import synthetic
from tests import scorer_f64 as f64
from tests import test_scorer_degenerate_gpu as dg

pytestmark = pytest.mark.gpu

GEMMS = dg.GEMMS
ROUNDS = (2, 2)
DROPOUT_P = 0.25
ONE_ELEMENT = ("struct_gate_net.0.bias", "score_head.bias")


# ---- the batch of the width and dropout cases --------------------------------------------------------------------------------
def _wide_batch(D):
    """Three graphs of ~40 nodes and ~120 edges (E = 360: every weight-gradient product has K > 64, six chunks of 64), nine
    relations, three more nodes made non-text so that non_text_entity_emb has terms; the same graph at every D."""
    sb = synthetic.make_batch(3, nodes_per_graph=40, edges_per_graph=120, emb_dim=D, num_relations=9, seed=7)
    ids = sb.node_embedding_ids.copy()
    ids[[1, sb.num_nodes // 2, sb.num_nodes - 2]] = 0
    E = sb.num_edges
    assert 320 < E <= 384 and int((ids == 0).sum()) >= 3 and int(sb.edge_attr.max()) == 8
    return types.SimpleNamespace(
        edge_index=sb.edge_index, ptr=sb.ptr, edge_ptr=sb.edge_ptr, edge_attr=sb.edge_attr, topic_one_hot=sb.topic_one_hot,
        node_embedding_ids=ids, question_emb=sb.question_emb, node_embeddings=sb.node_embeddings,
        edge_embeddings=sb.edge_embeddings, q_local_indices=sb.q_local_indices, a_local_indices=sb.a_local_indices,
        gvec=np.random.default_rng(1000 + D).standard_normal(E).astype(np.float32), num_nodes=sb.num_nodes,
        num_graphs=sb.num_graphs)


# ---- the float64 reference without per-edge term tensors -----------------------------------------------------------------------
def _float64_run_reverse_mode(model, b, mode, **fwd_kw):
    """Outputs and d (logits . gvec) / d parameter in float64 by reverse mode; `terms_abs` (what dg._compare reads as A_p) is
    exact where a rule depends on it — the one-element parameters, by forward mode; 0 for a parameter outside the graph —
    and max |g| elsewhere."""
    kw = dict(num_rounds=ROUNDS[0], num_reverse_rounds=ROUNDS[1], direction_mode=mode, **fwd_kw)
    w = f64.leaf_weights(model.state_dict())
    out = f64.retriever_forward(w, b, **kw)
    gvec = torch.from_numpy(b.gvec).double()
    names = list(w)
    scalar = (out["logits"] * gvec).sum()
    grads = torch.autograd.grad(scalar, [w[n] for n in names], allow_unused=True)
    ref = {k: None if out[k] is None else out[k].detach().numpy() for k in dg.OUT_KEYS}
    ref["grads"] = {n: np.zeros(tuple(w[n].shape)) if g is None else g.numpy() for n, g in zip(names, grads)}
    ref["terms_abs"] = {n: float(np.abs(g).max()) for n, g in ref["grads"].items()}
    has_non_text = bool((np.asarray(b.node_embedding_ids) == 0).any())
    for n, g in zip(names, grads):
        assert (g is None) == (n == "non_text_entity_emb.weight" and not has_non_text), n
        assert g is None or ref["terms_abs"][n] > 0.0, n
    plain = {n: t.detach() for n, t in w.items()}
    for n in ONE_ELEMENT:
        assert plain[n].numel() == 1
        with fwad.dual_level():
            dual = dict(plain)
            dual[n] = fwad.make_dual(plain[n], torch.ones_like(plain[n]))
            tangent = fwad.unpack_dual(f64.retriever_forward(dual, b, **kw)["logits"]).tangent
        terms = tangent * gvec  # the c_e of this parameter
        ref["terms_abs"][n] = float(terms.abs().sum())
        assert abs(float(terms.sum()) - float(ref["grads"][n].reshape(()))) <= 1e-12 * ref["terms_abs"][n], n
    assert sorted(n for n, g in ref["grads"].items() if g.size == 1) == sorted(ONE_ELEMENT)
    ref["scalar"] = float(scalar.detach())
    ref["E"] = int(gvec.numel())
    return ref


def _reference(key, make):
    """One float64 run per key, shared read-only between the GEMM modes / chunk sizes / replay and recompute."""
    if key not in dg._REFERENCE:
        ref = make()
        for arr in [v for v in ref.values() if isinstance(v, np.ndarray)] + list(ref["grads"].values()):
            arr.setflags(write=False)
        dg._REFERENCE[key] = ref
    return dg._REFERENCE[key]


def _set_chunk(monkeypatch, chunk):
    if chunk is None:
        monkeypatch.delenv("EVI_EDGE_CHUNK", raising=False)
    else:
        monkeypatch.setenv("EVI_EDGE_CHUNK", str(chunk))


def _finish(dev, tag, gemm, b, out, model, ref):
    (out.logits * torch.from_numpy(b.gvec).to(dev)).sum().backward()
    torch.cuda.synchronize()
    assert np.array_equal(out.query_ids.cpu().numpy(), np.repeat(np.arange(b.num_graphs), np.diff(b.edge_ptr)))
    dg._compare(tag, gemm, out, model, ref, label="wide")


def _run_eval(dev, tag, gemm, monkeypatch, D, H, *, mode="bidirectional", keep=True):
    """The eval-mode differentiable graph at (D, H) on the wide batch against float64."""
    dg._set_gemm(monkeypatch, gemm)
    _set_chunk(monkeypatch, None)
    b = _wide_batch(D)
    ref = _reference(("wide", D, H, mode), lambda: _float64_run_reverse_mode(dg._make_model(D, H, ROUNDS, mode), b, mode))
    model = dg._make_model(D, H, ROUNDS, mode).to(dev).eval()
    model.differentiable = True
    model.keep_forward_intermediates = keep
    out = model(dg._to_device(b, dev))
    assert out.logits.requires_grad
    _finish(dev, tag, gemm, b, out, model, ref)


def _run_train(dev, tag, gemm, monkeypatch, D, H, *, mode="bidirectional", keep=True, chunk=None, hide_seek=False):
    """train() mode with dropout_p = 0.25 on the wide batch: the mask follows from the seed the forward draws from torch's CPU
    generator; the float64 model with that mask (and, with hide_seek, the deterministic bias) is the reference."""
    from evi_rag_amd import ops

    dg._set_gemm(monkeypatch, gemm)
    _set_chunk(monkeypatch, chunk)
    b = _wide_batch(D)
    E = int(b.edge_attr.size)
    hs = {"enabled": False}
    if hide_seek:
        hs = {"enabled": True, "p_near": 1.0, "p_far": 1.0, "bias_near": -2.0, "bias_far": -0.5}
    model = dg._make_model(D, H, ROUNDS, mode, dropout_p=DROPOUT_P, hide_seek_cfg=hs).to(dev).train()
    model.keep_forward_intermediates = keep
    batch = dg._to_device(b, dev)
    fwd_kw = {}
    if hide_seek:
        batch.q_local_indices = torch.from_numpy(b.q_local_indices).to(dev)
        batch.a_local_indices = torch.from_numpy(b.a_local_indices).to(dev)
        near = ops.qa_edge_mask(batch.edge_index, b.num_nodes, batch.q_local_indices, batch.a_local_indices).cpu().numpy()
        qa = np.concatenate([b.q_local_indices, b.a_local_indices])
        assert np.array_equal(near, np.isin(b.edge_index[0], qa) | np.isin(b.edge_index[1], qa)) and 0 < near.sum() < E
        fwd_kw["edge_bias"] = np.where(near, -2.0, -0.5)
    s = 11 + D + H
    torch.manual_seed(s)
    seed = int(torch.randint(0, 2 ** 62, (1,), dtype=torch.int64).item())  # what the forward will draw
    mul = f64._dropout_multipliers(seed, E, H, DROPOUT_P)
    assert abs(float((mul > 0).mean()) - (1 - DROPOUT_P)) < 0.02
    ref = _reference(("dropout", D, H, mode, hide_seek), lambda: _float64_run_reverse_mode(
        dg._make_model(D, H, ROUNDS, mode), b, mode, dropout_mul=mul, **fwd_kw))
    torch.manual_seed(s)
    out = model(batch)
    assert out.logits.requires_grad
    _finish(dev, tag, gemm, b, out, model, ref)


# ---- widths ----------------------------------------------------------------------------------------------------------------------
WIDTHS = [
    pytest.param(4, 4, id="4x4-the-minimum-one-float4-63-idle-lanes"),
    pytest.param(256, 260, id="256x260-exactly-one-full-group-and-one-float4-into-the-second"),
    pytest.param(252, 512, id="252x512-63-lanes-of-one-group-and-exactly-two-groups"),
    pytest.param(768, 768, id="768x768-bge-base-three-full-groups"),
    pytest.param(1024, 1100, id="1024x1100-four-full-groups-and-19-lanes-of-the-fifth"),
    pytest.param(1280, 1276, id="1280x1276-five-full-groups-and-63-of-64-lanes-of-the-fifth"),
    pytest.param(1276, 16, id="1276x16-wide-D-narrow-H-dpl-5-against-1"),
    pytest.param(16, 1280, id="16x1280-narrow-D-wide-H-dpl-1-against-5"),
]


@pytest.mark.parametrize("gemm", GEMMS)
@pytest.mark.parametrize("D,H", WIDTHS)
def test_widths_bidirectional(dev, monkeypatch, gemm, D, H):
    _run_eval(dev, f"wide {D}x{H}", gemm, monkeypatch, D, H)


@pytest.mark.parametrize("gemm", GEMMS)
@pytest.mark.parametrize("mode", ["forward", "backward"])
@pytest.mark.parametrize("D,H", [pytest.param(1024, 1100, id="1024x1100-partial-fifth-group"),
                                 pytest.param(256, 260, id="256x260-one-float4-into-the-second-group")])
def test_widths_single_direction(dev, monkeypatch, gemm, mode, D, H):
    _run_eval(dev, f"wide {D}x{H} {mode}", gemm, monkeypatch, D, H, mode=mode)


@pytest.mark.parametrize("gemm", GEMMS)
def test_widths_recomputing_backward_at_768(dev, monkeypatch, gemm):
    """keep_forward_intermediates off (on is test_widths_bidirectional's run): same reference."""
    _run_eval(dev, "wide 768x768 recompute", gemm, monkeypatch, 768, 768, keep=False)


# ---- training mode under dropout ----------------------------------------------------------------------------------------------------
DROPOUT_WIDTHS = [pytest.param(16, 32, id="16x32"), pytest.param(260, 1100, id="260x1100"), pytest.param(768, 768, id="768x768")]


@pytest.mark.parametrize("gemm", GEMMS)
@pytest.mark.parametrize("D,H", DROPOUT_WIDTHS)
def test_dropout_bidirectional(dev, monkeypatch, gemm, D, H):
    _run_train(dev, f"dropout {D}x{H}", gemm, monkeypatch, D, H)


@pytest.mark.parametrize("gemm", GEMMS)
@pytest.mark.parametrize("mode", ["forward", "backward"])
def test_dropout_single_direction(dev, monkeypatch, gemm, mode):
    """The one direction hashes its own rows of the mask: [0] forward, [1] backward (scorer_f64._dropout_multipliers)."""
    _run_train(dev, f"dropout 16x32 {mode}", gemm, monkeypatch, 16, 32, mode=mode)


@pytest.mark.parametrize("gemm", GEMMS)
@pytest.mark.parametrize("keep", [True, False], ids=["replay", "recompute"])
@pytest.mark.parametrize("D,H", DROPOUT_WIDTHS[:2])
def test_dropout_over_six_chunks(dev, monkeypatch, gemm, keep, D, H):
    """EVI_EDGE_CHUNK = 64 at E = 360: the reference is the one-chunk case's, so a mask row built from a chunk-local edge
    number or edge count gives other multipliers from the second chunk on and misses every bar."""
    assert -(-_wide_batch(D).edge_attr.size // 64) == 6
    _run_train(dev, f"dropout {D}x{H} chunk=64 keep={keep}", gemm, monkeypatch, D, H, keep=keep, chunk=64)


@pytest.mark.parametrize("gemm", GEMMS)
def test_dropout_with_hide_and_seek_on_every_edge(dev, monkeypatch, gemm):
    """p_near = p_far = 1: every edge is hidden, the bias is bias_near / bias_far by `ops.qa_edge_mask` (checked here against
    its definition) and enters the float64 model as `edge_bias`; dropout 0.25 on top."""
    _run_train(dev, "dropout 16x32 hide-and-seek", gemm, monkeypatch, 16, 32, hide_seek=True)


# ---- row counts on both sides of the host-side switches, D = 16, H = 32 -------------------------------------------------------------------
def _with_relations(g, rel):
    g["triples"] = [(h, int(r), t) for (h, _, t), r in zip(g["triples"], rel)]
    return g


def _seam_batch(kind, n, D):
    """edges: B = 1 with n edges.  one+513: B = 2 with 1 and 513 edges.  graphs: n graphs of 2..3 edges.  one-edge-graphs: n graphs of
    one edge.  nodes: n nodes,
    most of graph 1's isolated (one of them a seed).  relations: a table of n rows over 130 edges, every row used.
    long-relations: two relations over 600 edges in two graphs."""
    rng = np.random.default_rng(200 + n)
    rel5 = np.arange(5)
    R = None
    if kind == "edges":
        graphs = [dg._random_graph(rng, 2 if n == 1 else 12, n, np.arange(min(5, n)), seeds=(0,))]
    elif kind == "one+513":
        graphs = [dg._random_graph(rng, 2, 1, [0]), dg._random_graph(rng, 30, 513, rel5, seeds=(0, 3))]
    elif kind == "graphs":
        graphs = [dg._random_graph(rng, 3, 2 + i % 2, np.arange(4), seeds=(i % 3,)) for i in range(n)]
    elif kind == "one-edge-graphs":
        graphs = [dg._random_graph(rng, 2, 1, np.arange(4), seeds=(i % 2,)) for i in range(n)]
    elif kind == "nodes":
        g1 = dg._random_graph(rng, 15, 40, rel5, seeds=(1,))
        g1["n"] = n - 20
        g1["seeds"] = [1, n - 21]
        graphs = [dg._random_graph(rng, 20, 60, rel5, seeds=(0,)), g1]
    elif kind == "relations":
        R = n
        rel = np.concatenate([rng.permutation(R), rng.integers(0, R, 130 - R)])
        graphs = [_with_relations(dg._random_graph(rng, 14, 65, [0]), rel[:65]),
                  _with_relations(dg._random_graph(rng, 11, 65, [0], seeds=(2,)), rel[65:])]
    else:
        R = 2
        graphs = [dg._random_graph(rng, 25, 300, [0, 1]), dg._random_graph(rng, 20, 300, [0, 1], seeds=(4,))]
    b = dg._assemble(graphs, D, seed=300 + n, num_relation_rows=R)
    E, B, N = int(b.edge_attr.size), b.num_graphs, b.num_nodes
    if kind == "edges":
        assert (E, B) == (n, 1) and N < 64
    elif kind == "one+513":
        assert np.diff(b.edge_ptr).tolist() == [1, 513] and (E // B + 255) // 256 == 2
    elif kind == "graphs":
        assert B == n and 64 < E <= 256
    elif kind == "one-edge-graphs":
        assert B == n and E == n
    elif kind == "nodes":
        assert N == n and E == 100 and B == 2
    elif kind == "relations":
        assert b.relation_table.shape[0] == n and np.unique(b.edge_attr).size == n and E == 130
    else:
        assert E == 600 and min(np.bincount(b.edge_attr).tolist()) > 256 and b.relation_table.shape[0] == 2
    return b


SEAMS = [
    # (kind, n, dedupe_relations).  Bidirectional, one chunk: ec = E and M = 2 E rows per chunk.
    pytest.param("edges", 1, True, id="E=1"),
    pytest.param("edges", 32, True, id="E=32-dWb-and-struct_proj-at-K=2E=64-exact-f32-small"),
    pytest.param("edges", 33, True, id="E=33-dWb-and-struct_proj-at-K=2E=66-split-K"),
    pytest.param("edges", 64, True, id="E=64-dWa-dWc-at-K=E-exact-f32-small"),
    pytest.param("edges", 65, True, id="E=65-dWa-dWc-at-K=E-split-K"),
    pytest.param("edges", 64, False, id="E=64-no-dedupe-relation_proj-at-K=E-exact-f32-small"),
    pytest.param("edges", 65, False, id="E=65-no-dedupe-relation_proj-at-K=E-split-K"),
    pytest.param("edges", 252, True, id="E=252-struct-partial-table-252-rows-one-colsum-block"),
    pytest.param("edges", 253, True, id="E=253-struct-partial-table-258-rows-two-colsum-blocks"),
    pytest.param("edges", 256, True, id="E=256-question-side-segment_rowsum_mul-one-slice"),
    pytest.param("edges", 257, True, id="E=257-question-side-segment_rowsum_mul-two-slices"),
    pytest.param("edges", 256, False, id="E=256-no-dedupe-relation-colsum-one-block-segment_rowsum-one-slice"),
    pytest.param("edges", 257, False, id="E=257-no-dedupe-relation-colsum-two-stages-segment_rowsum-two-slices"),
    pytest.param("one+513", 2, True, id="B=2-with-1-and-513-edges-segment_rowsum_mul-slices-nearly-all-empty"),
    pytest.param("one+513", 2, False, id="B=2-with-1-and-513-edges-no-dedupe-segment_rowsum-slices-nearly-all-empty"),
    pytest.param("graphs", 64, True, id="B=64-question-side-exact-f32-small"),
    pytest.param("graphs", 65, True, id="B=65-question-side-split-K"),
    pytest.param("one-edge-graphs", 256, True, id="B=256-question-side-colsum-one-block"),
    pytest.param("one-edge-graphs", 257, True, id="B=257-question-side-colsum-two-stages"),
    pytest.param("nodes", 64, True, id="N=64-entity-side-exact-f32-small"),
    pytest.param("nodes", 65, True, id="N=65-entity-side-split-K"),
    pytest.param("nodes", 256, True, id="N=256-entity-side-colsum-one-block"),
    pytest.param("nodes", 257, True, id="N=257-entity-side-colsum-two-stages"),
    pytest.param("relations", 64, True, id="R=64-table-relation-side-exact-f32-small"),
    pytest.param("relations", 65, True, id="R=65-table-relation-side-split-K"),
    pytest.param("long-relations", 2, True, id="R=2-table-600-edges-relation-segments-over-256-rows-two-slices"),
]


@pytest.mark.parametrize("gemm", GEMMS)
@pytest.mark.parametrize("kind,n,dedupe", SEAMS)
def test_row_count_seams(dev, monkeypatch, gemm, kind, n, dedupe):
    """Which count feeds which product, read in csrc/scorer.hip (chunk_backward, batch_backward), one chunk, both directions:
     * state_net.0: dWa, dWc are tn_gemm over K = E rows, dWb and struct_proj.0.weight over K = M = 2 E rows (E = 32 | 33 and
       64 | 65 are their two 64 | 65 seams);
     * the struct-side vectors are column sums of a partial table of 6 ceil(E / 6) rows (252 | 258 at E = 252 | 253), the
       state-side ones of one of ceil(E / 4) rows (at most 150 here: its 256 | 257 seam, E = 1024 | 1028, is not straddled);
     * entity side: tn_gemm and colsum_into over N rows;
     * relation side: with de-duplicated relations (the default; R = max id + 1 = 5 rows in the "edges" batches, the table's
       rows in the table form) tn_gemm and colsum_into run over R rows and k_segment_rowsum_mul over the R relation
       segments; with dedupe_relations=False they run over E rows — tn_gemm at K = E, colsum_into over E rows — and the
       question side sums d r_ctx per graph with k_segment_rowsum instead of k_segment_rowsum_mul;
     * question side: tn_gemm and colsum_into over B rows; the segment sums over the B graphs are cut into
       Z = (E / B + 255) / 256 slices (1 | 2 at E = 256 | 257 with B = 1; 2 at 1 + 513 edges, where one graph's slices are all
       but empty).
    A no-dedupe run computes the same function: it shares the float64 reference of its de-duplicated twin."""
    _set_chunk(monkeypatch, None)
    b = _seam_batch(kind, n, 16)
    kw = {} if dedupe else {"dedupe_relations": False}
    dg._run_gvec(dev, f"seam {kind} {n}{'' if dedupe else ' no-dedupe'}", gemm, monkeypatch, b, 16, 32,
                 table_form=kind.endswith("relations"), ref_key=("seam", kind, n), label="rows", **kw)
