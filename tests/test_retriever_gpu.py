"""GPU parity of the scorer path (S1-S6, G1, G6, G7, G11) against the golden fixtures produced by
the reference's own Retriever and against the numpy oracle on larger synthetic batches."""
import os
import types

import numpy as np
import pytest
import torch

from evi_rag_amd import synthetic
from oracle import graph as ograph
from oracle import scorer as oscorer
from oracle.ranking import stable_desc_order

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _load(name):
    return np.load(os.path.join(GOLD, name + ".npz"), allow_pickle=False)


def _batch_from(z, dev, prefix="b_"):
    b = types.SimpleNamespace()
    for k in z.files:
        if k.startswith(prefix):
            setattr(b, k[len(prefix):], torch.from_numpy(z[k]).to(dev))
    b.num_graphs = int(b.ptr.numel() - 1)
    b.num_nodes = int(b.ptr[-1].item())
    b._slice_dict = {"edge_index": b.edge_ptr}
    return b


def _model_from(z, dev, direction="bidirectional"):
    from evi_rag_amd.retriever import Retriever

    rounds = z["rounds"].tolist()
    m = Retriever(emb_dim=int(z["D"]), hidden_dim=int(z["H"]),
                  dde_cfg={"num_rounds": rounds[0], "num_reverse_rounds": rounds[1]}, direction_mode=direction)
    sd = {k[2:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("w_")}
    m.load_state_dict(sd, strict=True)  # the reference's eval loads strict=True (src/eval.py:111)
    return m.to(dev).eval()


@pytest.mark.parametrize("M,K,N,act", [(1, 32, 32, "tanh"), (37, 48, 20, None), (300, 768, 768, "sigmoid"),
                                        (1000, 2308, 96, None), (129, 16, 130, "tanh"), (64, 30, 16, None)])
def test_gemm_matches_torch_fp32(dev, M, K, N, act):
    """fp32 reference of the same op: torch CPU float64 accumulate, compared at f32 rounding level."""
    from evi_rag_amd import ops

    g = torch.Generator().manual_seed(M * 7 + K)
    x = torch.randn((M, K), generator=g)
    w = torch.randn((N, K), generator=g) / K ** 0.5
    b = torch.randn((N,), generator=g)
    got = ops.linear_act(x.to(dev), w.to(dev), b.to(dev), act).cpu()
    ref = (x.double() @ w.double().T + b.double())
    ref = {"tanh": torch.tanh, "sigmoid": torch.sigmoid, None: lambda v: v}[act](ref).float()
    # one f32 FMA chain of length K per output: error grows ~ K * 2^-24 * |terms|
    torch.testing.assert_close(got, ref, rtol=0, atol=3e-6 * max(1.0, K / 256))


@pytest.mark.parametrize("M,K,N,act", [(1, 32, 32, "tanh"), (300, 768, 768, "sigmoid"), (1000, 2308, 768, None),
                                        (257, 48, 300, "tanh"), (513, 36, 16, None)])
def test_gemm_bf16x3_matches_fp32_reference(dev, M, K, N, act):
    """Split-bf16 GEMM vs an fp64-accumulated fp32 reference: error ~1e-5 of sum|a w|, far inside 1e-3."""
    from evi_rag_amd import ops

    g = torch.Generator().manual_seed(M + K + N)
    x = torch.randn((M, K), generator=g)
    w = torch.randn((N, K), generator=g) / K ** 0.5
    b = torch.randn((N,), generator=g)
    got = ops.linear_act(x.to(dev), w.to(dev), b.to(dev), act, mode="bf16x3").cpu()
    ref = (x.double() @ w.double().T + b.double())
    ref = {"tanh": torch.tanh, "sigmoid": torch.sigmoid, None: lambda v: v}[act](ref).float()
    torch.testing.assert_close(got, ref, rtol=0, atol=4e-5)
    exact = ops.linear_act(x.to(dev), w.to(dev), b.to(dev), act, mode="f32").cpu()
    assert float((got - exact).abs().max()) < 4e-5


def test_retriever_forward_exact_f32_gemm_mode(dev, monkeypatch):
    """EVI_SCORER_GEMM=f32 selects the exact f32-MFMA GEMM; both modes meet the reference golden."""
    monkeypatch.setenv("EVI_SCORER_GEMM", "f32")
    z = _load("retriever_mid")
    model = _model_from(z, dev)
    with torch.no_grad():
        out = model(_batch_from(z, dev))
    np.testing.assert_allclose(out.logits.cpu().numpy(), z["logits"], rtol=0, atol=5e-5)
    np.testing.assert_allclose(out.edge_embeddings.cpu().numpy(), z["edge_embeddings"], rtol=0, atol=5e-5)


def test_gemm_rejects_unaligned(dev):
    from evi_rag_amd import _lib

    lib = _lib.load()
    rc = lib.evi_gemm_nt_f32(None, 4, 6, 6, None, 4, 6, None, 0, None, 4, None)
    assert rc == _lib.EVI_ERR_INVALID and "multiples of 4" in _lib.last_error()


def test_edge_batch_and_qa_mask_match_golden(dev):
    from evi_rag_amd import retriever as R

    z = _load("graph_utils_toy")
    b = _batch_from(z, dev)
    eb, eptr = R.compute_edge_batch(b.edge_index, node_ptr=b.ptr, num_graphs=b.num_graphs, device=dev)
    assert np.array_equal(eb.cpu().numpy(), z["edge_batch"])
    assert np.array_equal(eptr.cpu().numpy(), z["edge_ptr"])
    near = R.compute_qa_edge_mask(b.edge_index, num_nodes=b.num_nodes, q_local_indices=b.q_local_indices,
                                  a_local_indices=b.a_local_indices)
    assert np.array_equal(near.cpu().numpy(), z["near_mask"])
    bad = b.edge_index.clone()
    bad[1, 0] = b.ptr[-1] - 1
    with pytest.raises(ValueError, match="crosses graph boundaries"):
        R.compute_edge_batch(bad, node_ptr=b.ptr, num_graphs=b.num_graphs)
    with pytest.raises(ValueError, match="non-decreasing"):
        R.compute_edge_batch(b.edge_index.flip(1).contiguous(), node_ptr=b.ptr, num_graphs=b.num_graphs)
    with pytest.raises(ValueError, match="exceed num_nodes"):
        R.compute_qa_edge_mask(b.edge_index, num_nodes=b.num_nodes, q_local_indices=torch.tensor([b.num_nodes]),
                               a_local_indices=torch.tensor([], dtype=torch.long))


@pytest.mark.parametrize("shape", [(32, 64, 31), (4, 3000, 10000), (3, 50, 4000)])
def test_csr_and_dde_match_oracle(dev, shape):
    from evi_rag_amd import ops

    B, n, e = shape
    sb = synthetic.make_batch(B, nodes_per_graph=n, edges_per_graph=e, emb_dim=8, seed=B + n, attach_embeddings=False)
    ei = torch.from_numpy(sb.edge_index).to(dev)
    ptr = torch.from_numpy(sb.ptr).to(dev)
    eptr = torch.from_numpy(sb.edge_ptr).to(dev)
    csr = ops.graph_csr(ei, ptr, eptr)
    # CSR content == adjacency lists of the oracle (rows are unordered: compare as sorted multisets)
    in_ptr, in_nbr, in_eid = (t.cpu().numpy() for t in (csr.in_ptr, csr.in_nbr, csr.in_eid))
    out_ptr, out_nbr, out_eid = (t.cpu().numpy() for t in (csr.out_ptr, csr.out_nbr, csr.out_eid))
    N, E = sb.num_nodes, sb.num_edges
    assert in_ptr[0] == 0 and in_ptr[N] == E and out_ptr[N] == E
    assert np.array_equal(np.diff(in_ptr[: N + 1]), np.bincount(sb.edge_index[1], minlength=N))
    assert np.array_equal(np.diff(out_ptr[: N + 1]), np.bincount(sb.edge_index[0], minlength=N))
    assert np.array_equal(np.sort(in_eid[:E]), np.arange(E)) and np.array_equal(np.sort(out_eid[:E]), np.arange(E))
    assert np.array_equal(sb.edge_index[0][in_eid[:E]], in_nbr[:E])
    assert np.array_equal(sb.edge_index[1][out_eid[:E]], out_nbr[:E])
    rows_in = np.repeat(np.arange(N), np.diff(in_ptr[: N + 1]))
    assert np.array_equal(sb.edge_index[1][in_eid[:E]], rows_in)
    for rounds in [(2, 2), (4, 0), (1, 3)]:
        ns = ops.dde_node_struct(torch.from_numpy(sb.topic_one_hot).to(dev), ptr, csr, *rounds).cpu().numpy()
        ref = ograph.node_structure_features(sb.topic_one_hot, sb.edge_index, *rounds)
        np.testing.assert_allclose(ns, ref, rtol=0, atol=2e-6)


@pytest.mark.parametrize("name", ["retriever_toy", "retriever_mid", "retriever_fwd", "retriever_bwd"])
def test_retriever_forward_matches_reference_golden(dev, name):
    """Outputs of the reference Retriever (random-init, seeded) on the committed batches.
    Tolerance 2e-4 absolute on logits/features (north_star: fp scores within 1e-3)."""
    z = _load(name)
    direction = str(z["direction"])
    model = _model_from(z, dev, direction)
    assert list(model.state_dict().keys()) == z["state_dict_keys"].tolist()
    batch = _batch_from(z, dev)
    with torch.no_grad():
        out = model(batch)
        tokens = model.extract_edge_tokens(batch)
    torch.cuda.synchronize()
    assert np.array_equal(out.query_ids.cpu().numpy(), z["query_ids"])
    assert np.array_equal(out.relation_ids.cpu().numpy(), z["relation_ids"])
    np.testing.assert_allclose(out.logits.cpu().numpy(), z["logits"], rtol=0, atol=2e-4)
    np.testing.assert_allclose(out.edge_embeddings.cpu().numpy(), z["edge_embeddings"], rtol=0, atol=2e-4)
    np.testing.assert_allclose(tokens.cpu().numpy(), z["edge_tokens"], rtol=0, atol=2e-4)
    if direction == "bidirectional":
        np.testing.assert_allclose(out.logits_fwd.cpu().numpy(), z["logits_fwd"], rtol=0, atol=2e-4)
        np.testing.assert_allclose(out.logits_bwd.cpu().numpy(), z["logits_bwd"], rtol=0, atol=2e-4)
    # per-graph rankings agree with the reference's except across near-ties
    got, ref = out.logits.cpu().numpy(), z["logits"]
    eptr = z["b_edge_ptr"]
    for g in range(len(eptr) - 1):
        lo, hi = int(eptr[g]), int(eptr[g + 1])
        og, orf = stable_desc_order(got[lo:hi]), stable_desc_order(ref[lo:hi])
        diff = np.nonzero(og != orf)[0]
        if diff.size:
            assert np.max(np.abs(ref[lo:hi][og[diff]] - ref[lo:hi][orf[diff]])) < 4e-4


@pytest.mark.parametrize("dedupe", [True, False])
def test_retriever_forward_matches_oracle_webqsp_shape(dev, dedupe):
    """A WebQSP-shaped batch slice at the bench dims (D = H = 768) against the numpy oracle."""
    from evi_rag_amd.retriever import Retriever

    D = H = 768
    sb = synthetic.make_batch(3, nodes_per_graph=400, edges_per_graph=1200, emb_dim=D, num_relations=64, seed=9)
    torch.manual_seed(3)
    model = Retriever(emb_dim=D, hidden_dim=H, dedupe_relations=dedupe).eval()
    with torch.no_grad():
        for p in model.parameters():
            if p.dim() == 1:
                p.add_(0.1 * torch.randn_like(p))
    w = {k: v.numpy() for k, v in model.state_dict().items()}
    ref = oscorer.retriever_forward(w, sb, num_rounds=2, num_reverse_rounds=2)
    model = model.to(dev)
    out = model(synthetic.as_namespace(sb, device=dev))
    np.testing.assert_allclose(out.logits.cpu().numpy(), ref["logits"], rtol=0, atol=3e-4)
    np.testing.assert_allclose(out.logits_fwd.cpu().numpy(), ref["logits_fwd"], rtol=0, atol=3e-4)
    np.testing.assert_allclose(out.edge_embeddings.cpu().numpy(), ref["edge_embeddings"], rtol=0, atol=3e-4)
    assert np.array_equal(out.query_ids.cpu().numpy(), ref["query_ids"])


@pytest.mark.parametrize("chunk", [256, 1000])
def test_per_edge_pipeline_in_several_chunks_equals_one_chunk(dev, monkeypatch, chunk):
    """EVI_EDGE_CHUNK cuts the per-edge pipeline (edge features -> three GEMMs -> combine, and their backward) into chunks; a
    WebQSP-sized batch is ONE chunk at the default (262 144 edges), so the several-chunk path is exercised here: forward
    outputs must be identical (an edge's row does not depend on its chunk), parameter gradients equal up to the order in which
    the per-chunk partial sums are added."""
    from evi_rag_amd.retriever import Retriever

    sb = synthetic.make_batch(4, nodes_per_graph=300, edges_per_graph=800, emb_dim=64, num_relations=30, seed=21)
    batch = synthetic.as_namespace(sb, device=dev)
    batch.num_relations = 30
    torch.manual_seed(3)
    model = Retriever(emb_dim=64, hidden_dim=96).to(dev).eval()
    gl = torch.randn(sb.num_edges, device=dev)
    res = {}
    for tag, env in (("one", None), ("many", str(chunk))):
        if env is None:
            monkeypatch.delenv("EVI_EDGE_CHUNK", raising=False)
        else:
            monkeypatch.setenv("EVI_EDGE_CHUNK", env)
        model.differentiable = None
        o = model(batch)
        fwd = (o.logits.clone(), o.logits_fwd.clone(), o.logits_bwd.clone(), o.edge_embeddings.clone())
        model.differentiable = True
        model.zero_grad(set_to_none=True)
        (model(batch).logits * gl).sum().backward()
        res[tag] = (fwd, {n: p.grad.clone() for n, p in model.named_parameters()})
    for a, b in zip(res["one"][0], res["many"][0]):
        assert torch.equal(a, b)
    for n, g in res["one"][1].items():
        scale = float(g.abs().max()) + 1e-12
        assert float((g - res["many"][1][n]).abs().max()) <= 2e-5 * scale + 1e-7, n


@pytest.mark.parametrize("B,E_g,R,D,features", [(5, 900, 37, 96, True), (3, 2100, 600, 256, False), (2, 700, 1, 64, True),
                                                  (64, 40, 9, 32, True)])
def test_relation_graph_pair_rows_equal_the_per_edge_rows_bit_for_bit(dev, monkeypatch, B, E_g, R, D, features):
    """The forward multiplies r_ctx Wc^T once per distinct (relation, graph) pair (device-side count, GemmBatch::m_dev) and the
    combine kernel looks the row up; EVI_SCORER_PAIRS=0 keeps one row per edge.  Same arithmetic on the same values: every output
    must be IDENTICAL — logits, both directions, the edge features.  Cases: few / many relations per graph, ONE relation, more
    graphs than a pair table row is wide."""
    from evi_rag_amd.retriever import Retriever

    sb = synthetic.make_batch(B, nodes_per_graph=max(60, E_g // 4), edges_per_graph=E_g, emb_dim=D, num_relations=R, seed=B + R)
    torch.manual_seed(R)
    model = Retriever(emb_dim=D, hidden_dim=D).to(dev).eval()
    model.emit_edge_embeddings = features
    batch = synthetic.as_namespace(sb, device=dev)
    batch.num_relations = R
    outs = {}
    for flag in ("0", "1"):
        monkeypatch.setenv("EVI_SCORER_PAIRS", flag)
        o = model(batch)
        outs[flag] = (o.logits.clone(), o.logits_fwd.clone(), o.logits_bwd.clone(),
                      None if o.edge_embeddings is None else o.edge_embeddings.clone())
    for a, b in zip(outs["0"], outs["1"]):
        assert (a is None and b is None) or torch.equal(a, b)
    ref = oscorer.retriever_forward({k: v.cpu().numpy() for k, v in model.state_dict().items()}, sb, num_rounds=2, num_reverse_rounds=2)
    assert float(np.max(np.abs(outs["1"][0].cpu().numpy() - ref["logits"]))) <= 3e-4


@pytest.mark.parametrize("D,H,E_g", [(768, 768, 1200), (1024, 1024, 700), (96, 64, 300)])
def test_retriever_forward_f16x2_option_within_the_score_tolerance(dev, D, H, E_g):
    """matmul_precision="f16x2" (opt-in, evaluation only): two f16 MFMA products — activations split hi + lo in f16, every
    weight rounded once to f16.  The bar is north_star's score tolerance (1e-3 on the logits against the f32 oracle); measured
    far inside it.  The default ("split") is run beside it on the same batch for the comparison the docs quote; the backward
    refuses the option."""
    from evi_rag_amd.retriever import Retriever

    sb = synthetic.make_batch(3, nodes_per_graph=400, edges_per_graph=E_g, emb_dim=D, num_relations=64, seed=D + 1)
    torch.manual_seed(D)
    model = Retriever(emb_dim=D, hidden_dim=H).eval()
    with torch.no_grad():
        for p in model.parameters():
            if p.dim() == 1:
                p.add_(0.1 * torch.randn_like(p))
    w = {k: v.numpy() for k, v in model.state_dict().items()}
    ref = oscorer.retriever_forward(w, sb, num_rounds=2, num_reverse_rounds=2)
    model = model.to(dev)
    batch = synthetic.as_namespace(sb, device=dev)
    out_split = model(batch)
    model.matmul_precision = "f16x2"
    out = model(batch)
    err = float(np.max(np.abs(out.logits.cpu().numpy() - ref["logits"])))
    err_split = float(np.max(np.abs(out_split.logits.cpu().numpy() - ref["logits"])))
    from tests.helpers import report

    report("retriever_forward_f16x2", D=D, H=H, max_abs_dlogit_f16x2=err, max_abs_dlogit_split=err_split)
    print(f"\nf16x2 D={D} H={H}: max |dlogit| {err:.2e} (split-bf16: {err_split:.2e})")
    assert err <= 1e-3, err
    assert err_split <= 3e-4
    np.testing.assert_allclose(out.edge_embeddings.cpu().numpy(), ref["edge_embeddings"], rtol=0, atol=2e-3)
    assert not torch.equal(out.logits, out_split.logits)  # it really is another arithmetic
    model.emit_edge_embeddings = False  # logits-only form: score_head folded into state_net.4
    lite = model(batch)
    assert float((lite.logits - out.logits).abs().max()) <= 2e-4
    model.differentiable = True
    with pytest.raises(ValueError, match="evaluation-time option"):
        model(batch)
    with pytest.raises(ValueError, match="matmul_precision"):
        Retriever(emb_dim=D, hidden_dim=H, matmul_precision="fp4")


@pytest.mark.parametrize("D,H", [(1024, 1024), (384, 256), (1280, 64)])
def test_retriever_forward_other_dims(dev, D, H):
    """The reference default (emb_dim = hidden_dim = 1024, configs/model/retriever_module.yaml:10-11),
    a MiniLM-sized D and the largest supported D, against the numpy oracle."""
    from evi_rag_amd.retriever import Retriever

    sb = synthetic.make_batch(2, nodes_per_graph=120, edges_per_graph=300, emb_dim=D, num_relations=20, seed=D)
    torch.manual_seed(D)
    model = Retriever(emb_dim=D, hidden_dim=H, dde_cfg={"num_rounds": 1, "num_reverse_rounds": 2}).eval()
    w = {k: v.numpy() for k, v in model.state_dict().items()}
    ref = oscorer.retriever_forward(w, sb, num_rounds=1, num_reverse_rounds=2)
    out = model.to(dev)(synthetic.as_namespace(sb, device=dev))
    np.testing.assert_allclose(out.logits.cpu().numpy(), ref["logits"], rtol=0, atol=3e-4)
    np.testing.assert_allclose(out.edge_embeddings.cpu().numpy(), ref["edge_embeddings"], rtol=0, atol=3e-4)


@pytest.mark.parametrize("graphs", [1, 2, 5, 17, 31, 32, 33])
def test_question_side_projections_for_every_row_count(dev, graphs):
    """query_proj / q_gate / q_bias run on `graphs` rows: up to 32 rows on the one-wave-per-column f32 kernel (gemm_skinny.hip,
    whose row sums are scattered over the lane pairs by a butterfly), beyond that on the MFMA tile.  Every row count around the
    kernel's edges against the numpy oracle (src/models/components/retriever.py:214-223)."""
    from evi_rag_amd.retriever import Retriever

    D, H = 96, 64
    sb = synthetic.make_batch(graphs, nodes_per_graph=30, edges_per_graph=70, emb_dim=D, num_relations=11, seed=graphs)
    torch.manual_seed(graphs)
    model = Retriever(emb_dim=D, hidden_dim=H).eval()
    with torch.no_grad():
        for p in model.parameters():
            if p.dim() == 1:
                p.add_(0.1 * torch.randn_like(p))
    w = {k: v.numpy() for k, v in model.state_dict().items()}
    ref = oscorer.retriever_forward(w, sb, num_rounds=2, num_reverse_rounds=2)
    out = model.to(dev)(synthetic.as_namespace(sb, device=dev))
    np.testing.assert_allclose(out.logits.cpu().numpy(), ref["logits"], rtol=0, atol=1e-4)
    np.testing.assert_allclose(out.edge_embeddings.cpu().numpy(), ref["edge_embeddings"], rtol=0, atol=1e-4)


def test_retriever_forward_multi_chunk_batch(dev):
    """More than 65 536 edges: the scorer processes the batch in edge chunks; one big graph with a
    hub node (DDE hub path) and a small one."""
    from evi_rag_amd.retriever import Retriever

    D = H = 32
    sb = synthetic.make_batch(2, nodes_per_graph=6000, edges_per_graph=70000, emb_dim=D, num_relations=2000, seed=77,
                              alpha=1.6, size_jitter=0.1)
    assert sb.num_edges > 70000
    torch.manual_seed(5)
    model = Retriever(emb_dim=D, hidden_dim=H).eval()
    w = {k: v.numpy() for k, v in model.state_dict().items()}
    ref = oscorer.retriever_forward(w, sb, num_rounds=2, num_reverse_rounds=2)
    out = model.to(dev)(synthetic.as_namespace(sb, device=dev))
    np.testing.assert_allclose(out.logits.cpu().numpy(), ref["logits"], rtol=0, atol=2e-4)
    np.testing.assert_allclose(out.logits_bwd.cpu().numpy(), ref["logits_bwd"], rtol=0, atol=2e-4)
    np.testing.assert_allclose(out.edge_embeddings.cpu().numpy(), ref["edge_embeddings"], rtol=0, atol=2e-4)


def test_retriever_error_contract(dev):
    from evi_rag_amd.retriever import Retriever

    with pytest.raises(ValueError, match="num_topics must be 2"):
        Retriever(emb_dim=16, hidden_dim=16, num_topics=3)
    with pytest.raises(ValueError, match="topic_pe must be enabled"):
        Retriever(emb_dim=16, hidden_dim=16, topic_pe=False)
    with pytest.raises(ValueError, match="direction_mode must be one of"):
        Retriever(emb_dim=16, hidden_dim=16, direction_mode="sideways")
    with pytest.raises(ValueError, match="at most 4 rounds"):
        Retriever(emb_dim=16, hidden_dim=16, dde_cfg={"num_rounds": 5})
    m = Retriever(emb_dim=16, hidden_dim=16).to(dev).eval()
    with pytest.raises(ValueError, match="Batch missing edge_index"):
        m(types.SimpleNamespace())
    sb = synthetic.make_batch(2, nodes_per_graph=10, edges_per_graph=12, emb_dim=16, seed=1)
    ns = synthetic.as_namespace(sb, device=dev)
    del ns.topic_one_hot
    with pytest.raises(ValueError, match="topic_one_hot is required"):
        m(ns)
    ns = synthetic.as_namespace(sb, device=dev)
    ns.edge_index = ns.edge_index[:, :0]
    out = m(ns)  # empty edge list -> empty outputs (reference :206-207)
    assert out.logits.numel() == 0 and out.edge_embeddings.shape == (0, 16)
    # train() with hide-and-seek on (the reference default) needs the seed / answer indices, like the reference (:325-329)
    ns = synthetic.as_namespace(sb, device=dev)
    for attr in ("q_local_indices", "a_local_indices", "edge_is_near"):
        if hasattr(ns, attr):
            delattr(ns, attr)
    mh = Retriever(emb_dim=16, hidden_dim=16, hide_seek_cfg={"enabled": True, "p_near": 0.7, "p_far": 0.1, "bias_near": -2.0,
                                                             "bias_far": -0.5}).to(dev)
    with pytest.raises(ValueError, match="q_local_indices/a_local_indices required for hide-and-seek"):
        mh.train()(ns)


def test_logits_only_forward_matches_full(dev):
    """emit_edge_embeddings=False folds score_head into state_net.4: same logits, no feature tensor."""
    from evi_rag_amd import synthetic
    from evi_rag_amd.retriever import Retriever

    sb = synthetic.make_batch(6, nodes_per_graph=200, edges_per_graph=700, emb_dim=64, num_relations=30, seed=17)
    batch = synthetic.as_namespace(sb, device=dev)
    for mode in ("bidirectional", "forward", "backward"):
        torch.manual_seed(3)
        model = Retriever(emb_dim=64, hidden_dim=96, direction_mode=mode).to(dev).eval()
        full = model(batch)
        model.emit_edge_embeddings = False
        lite = model(batch)
        assert lite.edge_embeddings is None and full.edge_embeddings is not None
        np.testing.assert_allclose(lite.logits.cpu().numpy(), full.logits.cpu().numpy(), rtol=0, atol=2e-5)
        if mode == "bidirectional":
            np.testing.assert_allclose(lite.logits_fwd.cpu().numpy(), full.logits_fwd.cpu().numpy(), rtol=0, atol=2e-5)
            np.testing.assert_allclose(lite.logits_bwd.cpu().numpy(), full.logits_bwd.cpu().numpy(), rtol=0, atol=2e-5)
        tokens = model.extract_edge_tokens(batch)  # still available on request
        np.testing.assert_allclose(tokens.cpu().numpy(), full.edge_embeddings.cpu().numpy(), rtol=0, atol=1e-6)


def test_hide_seek_bias_in_eval(dev):
    """hide_seek_cfg.apply_in_eval: with p = 1 every edge is penalised, so the directional logits move by exactly
    bias_near / bias_far (by the Q/A mask) and the combined logit follows; p = 0 leaves the output untouched."""
    from evi_rag_amd.retriever import Retriever, compute_qa_edge_mask

    sb = synthetic.make_batch(4, nodes_per_graph=60, edges_per_graph=150, emb_dim=32, num_relations=9, seed=23)
    batch = synthetic.as_namespace(sb, device=dev)
    torch.manual_seed(5)
    plain = Retriever(emb_dim=32, hidden_dim=32).to(dev).eval()
    ref = plain(batch)
    cfg = dict(enabled=True, apply_in_eval=True, p_near=1.0, p_far=1.0, bias_near=-2.0, bias_far=-0.5)
    hs = Retriever(emb_dim=32, hidden_dim=32, hide_seek_cfg=cfg).to(dev).eval()
    hs.load_state_dict(plain.state_dict())
    near = compute_qa_edge_mask(batch.edge_index, num_nodes=batch.num_nodes, q_local_indices=batch.q_local_indices,
                                a_local_indices=batch.a_local_indices)
    bias = torch.where(near, torch.tensor(-2.0, device=dev), torch.tensor(-0.5, device=dev))
    for emit in (True, False):
        hs.emit_edge_embeddings = emit
        out = hs(batch)
        np.testing.assert_allclose(out.logits_fwd.cpu().numpy(), (ref.logits_fwd + bias).cpu().numpy(), rtol=0, atol=2e-5)
        np.testing.assert_allclose(out.logits_bwd.cpu().numpy(), (ref.logits_bwd + bias).cpu().numpy(), rtol=0, atol=2e-5)
        np.testing.assert_allclose(out.logits.cpu().numpy(), (ref.logits + bias).cpu().numpy(), rtol=0, atol=3e-5)
    off = Retriever(emb_dim=32, hidden_dim=32, hide_seek_cfg=dict(cfg, p_near=0.0, p_far=0.0)).to(dev).eval()
    off.load_state_dict(plain.state_dict())
    assert torch.equal(off(batch).logits, ref.logits)
    with pytest.raises(ValueError, match="must be <= 0"):
        Retriever(emb_dim=32, hidden_dim=32, hide_seek_cfg=dict(cfg, bias_far=0.1))


def test_out_of_range_relation_id_on_the_hint_path_is_reported_not_read_out_of_bounds(dev):
    """A packed split states batch.num_relations (embedding_store.attach) and the forward trusts it without a read-back;
    a relation id beyond it must not index past rel_repr: the edge is scored with a clamped row, every other logit is
    untouched, and Retriever.check_deferred() raises the IndexError the reference raises at its embedding gather."""
    from evi_rag_amd.retriever import Retriever

    D = H = 64
    sb = synthetic.make_batch(3, nodes_per_graph=50, edges_per_graph=120, emb_dim=D, num_relations=16, seed=4)
    torch.manual_seed(0)
    model = Retriever(emb_dim=D, hidden_dim=H).to(dev).eval()
    good = synthetic.as_namespace(sb, device=dev)
    good.num_relations = 16
    ref = model(good).logits.clone()
    model.check_deferred()  # nothing to report
    bad = synthetic.as_namespace(sb, device=dev)
    bad.num_relations = 16
    bad.edge_attr = bad.edge_attr.clone()
    bad.edge_attr[7] = 10_000_000  # far outside the relation table
    bad.edge_attr[11] = -3
    out = model(bad).logits
    torch.cuda.synchronize()
    keep = torch.ones_like(ref, dtype=torch.bool)
    keep[7] = keep[11] = False
    assert torch.equal(out[keep], ref[keep]) and bool(torch.isfinite(out).all())
    with pytest.raises(IndexError, match="edge_attr out of range"):
        model.check_deferred()
    model.check_deferred()  # the flag was reset


def test_csr_dde_and_bfs_agree_with_the_oracle(dev, monkeypatch):
    """The CSR build (one workgroup per (graph, side), rows staged in LDS and written out coalesced) must give the right rows
    (as multisets; the order inside a row is unspecified), DDE features and BFS levels.  The batch mixes tiny graphs, a hub,
    a graph without edges, and graphs beyond the build's LDS budget — the 20 000-edge and the 9 000-node ones, built by the
    global-memory path inside the same kernel — and one exactly at it (8 192 nodes, 14 336 edges)."""
    from evi_rag_amd import _lib, ops

    rng = np.random.default_rng(5)
    sizes = [(40, 90), (3000, 10000), (1, 0), (7000, 9000), (64, 4000), (500, 1), (300, 20000), (9000, 12000), (8192, 14336)]
    ei, ptr, eptr = [], [0], [0]
    for n, e in sizes:
        s = rng.integers(0, n, e)
        d = rng.integers(0, n, e)
        if e > 100:
            d[: e // 3] = 0  # a hub: a third of the edges end in node 0
        ei.append(np.stack([s, d]) + ptr[-1])
        ptr.append(ptr[-1] + n)
        eptr.append(eptr[-1] + e)
    ei = np.concatenate(ei, axis=1).astype(np.int64)
    N, E, B = ptr[-1], eptr[-1], len(sizes)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    csr = ops.graph_csr(t(ei), t(np.asarray(ptr, np.int64)), t(np.asarray(eptr, np.int64)))
    in_ptr, in_nbr, in_eid = (x.cpu().numpy() for x in (csr.in_ptr, csr.in_nbr, csr.in_eid))
    out_ptr, out_nbr, out_eid = (x.cpu().numpy() for x in (csr.out_ptr, csr.out_nbr, csr.out_eid))
    assert np.array_equal(np.diff(in_ptr[: N + 1]), np.bincount(ei[1], minlength=N)) and in_ptr[0] == 0 and in_ptr[N] == E
    assert np.array_equal(np.diff(out_ptr[: N + 1]), np.bincount(ei[0], minlength=N)) and out_ptr[N] == E
    assert np.array_equal(np.sort(in_eid[:E]), np.arange(E)) and np.array_equal(np.sort(out_eid[:E]), np.arange(E))
    assert np.array_equal(ei[0][in_eid[:E]], in_nbr[:E]) and np.array_equal(ei[1][out_eid[:E]], out_nbr[:E])
    assert np.array_equal(ei[1][in_eid[:E]], np.repeat(np.arange(N), np.diff(in_ptr[: N + 1])))
    assert np.array_equal(ei[0][out_eid[:E]], np.repeat(np.arange(N), np.diff(out_ptr[: N + 1])))
    # DDE over that CSR vs the oracle
    topic = np.zeros((N, 2), np.float32)
    topic[:, 1] = 1.0
    seeds = np.asarray([ptr[g] + (0 if n < 3 else 2) for g, (n, _) in enumerate(sizes)])
    topic[seeds] = [1.0, 0.0]
    for rounds in [(2, 2), (0, 3), (4, 1), (0, 0)]:
        # both forms of the kernel: node-parallel over the batch, and one workgroup per graph with the graph's feature block in
        # LDS (the 9 000-node graph's block does not fit and runs on its global rows) — equal bit for bit (f64 row sums)
        monkeypatch.setenv("EVI_DDE_MODE", "nodes")
        ns = ops.dde_node_struct(t(topic), t(np.asarray(ptr, np.int64)), csr, *rounds)
        monkeypatch.setenv("EVI_DDE_MODE", "graph")
        ns_g = ops.dde_node_struct(t(topic), t(np.asarray(ptr, np.int64)), csr, *rounds)
        monkeypatch.delenv("EVI_DDE_MODE")
        assert torch.equal(ns, ns_g), rounds
        # the oracle (like PyG's scatter-mean) sums a row in f32 in edge order, the kernels in f64 rounded once: the 6 667-entry
        # hub rows of the 20 000-edge graph carry a few f32 ulps of summation error on the ORACLE's side
        np.testing.assert_allclose(ns.cpu().numpy(), ograph.node_structure_features(topic, ei, *rounds), rtol=0, atol=6e-6)
    # multi-source BFS per graph vs the oracle (queue mode for the small graphs, scan mode for the 7000-node one)
    lib = _lib.load()
    jg = torch.arange(B, dtype=torch.int32, device=dev)
    src = np.concatenate([[ptr[g], ptr[g] + min(5, n - 1), ptr[g]] for g, (n, _) in enumerate(sizes)]).astype(np.int64)
    sp = np.arange(0, 3 * B + 1, 3).astype(np.int64)
    doff = np.asarray(ptr[:-1], np.int64)
    dist = torch.empty(N, dtype=torch.int32, device=dev)
    sp_d, src_d, doff_d, ptr_d = t(sp), t(src), t(doff), t(np.asarray(ptr, np.int64))  # kept alive across the launches
    ei_d, eptr_d = t(ei), t(np.asarray(eptr, np.int64))
    dist_e = torch.empty(N, dtype=torch.int32, device=dev)
    for mode in (0, 1, 2):
        _lib.check(lib.evi_bfs_levels(jg.data_ptr(), sp_d.data_ptr(), src_d.data_ptr(), doff_d.data_ptr(), B,
                                      ptr_d.data_ptr(), csr.in_ptr.data_ptr(), csr.in_nbr.data_ptr(),
                                      csr.out_ptr.data_ptr(), csr.out_nbr.data_ptr(), mode, dist.data_ptr(), ops._stream(dev)))
        # the edge-parallel LDS search (graphs whose edge list fits 48 KiB; the 20 000-edge graph takes the CSR path inside it)
        _lib.check(lib.evi_bfs_levels_edges(jg.data_ptr(), sp_d.data_ptr(), src_d.data_ptr(), doff_d.data_ptr(), B, ptr_d.data_ptr(),
                                            eptr_d.data_ptr(), ei_d.data_ptr(), E, csr.in_ptr.data_ptr(), csr.in_nbr.data_ptr(),
                                            csr.out_ptr.data_ptr(), csr.out_nbr.data_ptr(), mode, dist_e.data_ptr(), ops._stream(dev)))
        assert torch.equal(dist, dist_e), mode
        got = dist.cpu().numpy()
        for g, (n, e) in enumerate(sizes):
            s_l, d_l = (ei[0, eptr[g]: eptr[g + 1]] - ptr[g]).tolist(), (ei[1, eptr[g]: eptr[g + 1]] - ptr[g]).tolist()
            if mode == 0:
                adj = ograph.build_undirected_adjacency(n, s_l, d_l)
            elif mode == 1:
                adj = ograph.build_directed_adjacency(n, s_l, d_l)
            else:
                adj = ograph.build_directed_adjacency(n, d_l, s_l)
            ref = ograph.bfs_dist(n, adj, [0, min(5, n - 1), 0])
            assert got[ptr[g]: ptr[g + 1]].tolist() == ref, (mode, g)


def test_prepared_weight_cache_follows_the_weights(dev):
    """Eval mode keeps the weight-derived pieces of the forward (state_net.0 column blocks, folded head, bf16 planes) across
    calls: the result must equal the uncached forward bit for bit, and an in-place change of ANY weight, a
    load_state_dict or a switch to train mode must be seen by the next forward."""
    from evi_rag_amd.retriever import Retriever

    D = H = 64
    sb = synthetic.make_batch(3, nodes_per_graph=60, edges_per_graph=150, emb_dim=D, num_relations=16, seed=8)
    batch = synthetic.as_namespace(sb, device=dev)
    torch.manual_seed(1)
    model = Retriever(emb_dim=D, hidden_dim=H).to(dev).eval()
    model.cache_prepared_weights = False
    ref = model(batch)
    ref_lite_model = model
    model.cache_prepared_weights = True
    a = model(batch)
    b = model(batch)  # second call: served from the cache
    assert model._prep_cache is not None
    for x, y in ((a, ref), (b, ref)):
        assert torch.equal(x.logits, y.logits) and torch.equal(x.edge_embeddings, y.edge_embeddings)
    model.emit_edge_embeddings = False  # folded head from the cache
    lite = model(batch).logits
    model.cache_prepared_weights = False
    assert torch.equal(lite, ref_lite_model(batch).logits)
    model.cache_prepared_weights = True
    model.emit_edge_embeddings = True
    # an in-place edit of one weight
    with torch.no_grad():
        model.state_net[4].weight.mul_(1.5)
        model.score_head.bias.add_(0.25)
    c = model(batch)
    model.cache_prepared_weights = False
    want = model(batch)
    model.cache_prepared_weights = True
    assert torch.equal(c.logits, want.logits) and not torch.equal(c.logits, ref.logits)
    # load_state_dict of other weights
    torch.manual_seed(2)
    other = Retriever(emb_dim=D, hidden_dim=H).to(dev).eval()
    model.load_state_dict(other.state_dict(), strict=True)
    assert torch.equal(model(batch).logits, other(batch).logits)
    # train mode never serves from the cache
    model.train()
    assert model._prepared_weights(model._weights_struct(), dev) is None


@pytest.mark.parametrize("K,M,N", [(1, 8, 8), (31, 20, 768), (257, 300, 260), (4096, 768, 768), (70001, 768, 20), (65536, 512, 1280),
                                   (131072, 768, 20), (1000, 300, 1), (513, 16, 32), (64, 1280, 33)])
def test_gemm_tn_equals_the_f64_product_and_is_reproducible(dev, K, M, N):
    """evi_gemm_tn_bf16x3 (a.T @ b, the weight-gradient product): within the split-bf16 bound of the f64 product of the same
    f32 operands (|err| <= 4e-5 * sum_k |a||b| elementwise), for K that is not a multiple of the k-tile or the slice, M / N
    that leave partial tiles; bit-identical on a second call; `accumulate` adds."""
    from evi_rag_amd import ops

    g = torch.Generator(device=dev).manual_seed(K + M + N)
    a = torch.randn(K, M, device=dev, generator=g)
    b = torch.randn(K, N, device=dev, generator=g)
    got = ops.gemm_tn(a, b)
    want = a.double().t() @ b.double()
    bound = 4e-5 * (a.double().abs().t() @ b.double().abs()) + 1e-30  # N <= 32 runs exact f32 FMAs: far inside it
    assert bool(((got.double() - want).abs() <= bound).all()), float(((got.double() - want).abs() / bound).max())
    again = ops.gemm_tn(a, b)
    assert torch.equal(got, again)
    acc = got.clone()
    ops.gemm_tn(a, b, acc, accumulate=True)
    assert torch.allclose(acc, 2 * got, rtol=1e-5, atol=1e-4)  # (got + p0) + p1 ... rounds differently from 2 (p0 + p1 ...)
