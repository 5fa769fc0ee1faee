"""GPU: the retriever oracle (evi_oracle_answer_hits + reasoner_oracle.py) against the reference's recorded run and the
CPU restatement, chunk and LDS invariance, graph capture, and `experiment=reasoner_oracle` end to end after an
`experiment=eval_retriever` run of the same tree."""
import gzip
import json
import os

import numpy as np
import pytest
import torch

from tests import answer_hits_oracle as aho

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "reasoner_oracle.json.gz")


def golden_cases():
    with gzip.open(GOLDEN, "rt", encoding="utf-8") as fh:
        return json.load(fh)["cases"]


@pytest.mark.parametrize("case", golden_cases(), ids=lambda c: c["name"])
def test_counts_and_files_equal_the_reference(case, dev, tmp_path):
    from evi_rag_amd.reasoner_oracle import ReasonerModule, ReasonerOracleDataModule, oracle_counts

    path = aho.write_case(tmp_path / "cache", case)
    dm = ReasonerOracleDataModule(dataset="toyqa", split="test", eval_retriever_path=str(path), k_values=case["data_k_values"])
    dm.setup()
    for use_lds in (True, False):
        uniq, found, _ = oracle_counts(dm.data, case["model_ks"], use_lds=use_lds)
        assert uniq.tolist() == case["uniq"] and found.tolist() == case["found"], use_lds
    module = ReasonerModule(mode="oracle", output_dir=str(tmp_path / "out"), dataset="toyqa", split="test", prompt_tag="oracle",
                            k_values=case["model_k_values"])
    metrics = module.run(dm.data)
    pred = tmp_path / "out" / "toyqa-oracle-test.jsonl"
    assert pred.read_text() == case["jsonl"]
    assert pred.with_suffix(".metrics.json").read_text() == case["metrics"]
    assert json.dumps(metrics, indent=2) == case["metrics"] and module.predict_metrics == metrics


def _random_samples(rng, n, *, max_answers, max_edges, ent_range):
    out = []
    for i in range(n):
        na = int(rng.integers(0, max_answers + 1)) if i % 7 else int(rng.integers(1, 4))
        ne = int(rng.integers(0, max_edges + 1))
        answers = rng.integers(0, ent_range, na).tolist()
        heads = rng.integers(0, ent_range, ne).tolist()
        tails = rng.integers(0, ent_range, ne).tolist()
        if i % 11 == 0 and answers:
            answers[0] = np.iinfo(np.int64).max  # sorts with the padding
            heads[:1] = [np.iinfo(np.int64).max] * min(1, ne)
        out.append({"id": str(i), "question": "q", "answer_entity_ids": answers, "head_entity_ids": heads, "tail_entity_ids": tails})
    return out


def test_random_grid_against_the_restatement(dev):
    from evi_rag_amd.reasoner_oracle import oracle_counts

    rng = np.random.default_rng(11)
    grids = [(60, 8, 600, 50), (40, 300, 300, 2000), (12, 5000, 600, 20000), (4, 10000, 600, 10**6), (30, 3, 0, 10)]
    for n, max_answers, max_edges, ent_range in grids:
        samples = _random_samples(rng, n, max_answers=max_answers, max_edges=max_edges, ent_range=ent_range)
        ks = sorted(set(int(k) for k in rng.integers(1, 700, int(rng.integers(1, 12)))))
        scan = int(rng.choice([max(ks), max(ks) // 2 + 1, 1000]))
        uniq, found, num_edges = oracle_counts(samples, ks, max_scan_k=scan, chunk_size=int(rng.integers(1, 40)))
        for i, s in enumerate(samples):
            want = aho.counts(s["head_entity_ids"], s["tail_entity_ids"], s["answer_entity_ids"], ks, scan)
            assert (int(uniq[i]), found[i].tolist()) == want, (n, i)
            assert num_edges[i] == len(s["head_entity_ids"])
    # more k values than one launch takes: the groups are launched one after the other
    samples = _random_samples(rng, 20, max_answers=20, max_edges=300, ent_range=100)
    ks = list(range(1, 301, 3))
    uniq, found, _ = oracle_counts(samples, ks)
    for i, s in enumerate(samples):
        assert (int(uniq[i]), found[i].tolist()) == aho.counts(s["head_entity_ids"], s["tail_entity_ids"], s["answer_entity_ids"], ks, 298)


def test_results_do_not_depend_on_chunk_size_or_lds(dev):
    from evi_rag_amd.reasoner_oracle import oracle_counts

    rng = np.random.default_rng(3)
    samples = _random_samples(rng, 300, max_answers=3000, max_edges=500, ent_range=3000)
    ks = [1, 10, 25, 50, 100, 200, 300, 400, 500]
    stats = {}
    ref = oracle_counts(samples, ks, chunk_size=300, stats=stats)
    assert stats["launches"] == 1
    for chunk, use_lds in ((1, True), (7, True), (64, False), (1000, True)):
        got = oracle_counts(samples, ks, chunk_size=chunk, use_lds=use_lds)
        assert all(np.array_equal(a, b) for a, b in zip(got, ref)), (chunk, use_lds)


def test_device_pass_replays_in_a_graph(dev):
    from evi_rag_amd import reasoner_oracle as ro

    rng = np.random.default_rng(5)
    samples = _random_samples(rng, 64, max_answers=6000, max_edges=500, ent_range=4000)  # LDS and workspace samples
    ks = [1, 10, 100, 500]

    def flat(samples):
        e_ptr, head = ro._cat([s["head_entity_ids"] for s in samples])
        _, tail = ro._cat([s["tail_entity_ids"] for s in samples])
        a_ptr, ans = ro._cat([s["answer_entity_ids"] for s in samples])
        return [torch.from_numpy(a).to(dev) for a in (e_ptr, head, tail, a_ptr, ans)]

    inputs = flat(samples)
    static = [t.clone() for t in inputs]
    uniq = torch.empty(64, dtype=torch.int32, device=dev)
    found = torch.empty(64 * len(ks), dtype=torch.int32, device=dev)
    ws = torch.empty(ro.workspace_bytes(int(static[4].numel())), dtype=torch.uint8, device=dev)
    stream = torch.cuda.Stream(device=dev)
    stream.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(stream):
        ro.answer_hits(*static, ks, 500, uniq=uniq, found=found, workspace=ws, lds_answers=1024)  # warm-up (kernel attribute)
    torch.cuda.current_stream(dev).wait_stream(stream)
    torch.cuda.synchronize(dev)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ro.answer_hits(*static, ks, 500, uniq=uniq, found=found, workspace=ws, lds_answers=1024)
    want = ro.oracle_counts(samples, ks)
    for _ in range(2):
        uniq.fill_(-1)
        found.fill_(-1)
        graph.replay()
        torch.cuda.synchronize(dev)
        assert uniq.cpu().numpy().tolist() == want[0].tolist()
        assert found.cpu().numpy().reshape(64, len(ks)).tolist() == want[1].tolist()
    # new contents in the captured buffers: the flat answer list reversed (answers move between samples)
    perm = torch.flip(inputs[4], dims=[0])
    static[4].copy_(perm)
    graph.replay()
    torch.cuda.synchronize(dev)
    e_ptr, head, tail, a_ptr = (t.cpu().numpy() for t in inputs[:4])
    ans = perm.cpu().numpy()
    for i in range(64):
        s = slice(int(e_ptr[i]), int(e_ptr[i + 1]))
        a = ans[int(a_ptr[i]):int(a_ptr[i + 1])].tolist()
        assert (int(uniq[i]), found.view(64, len(ks))[i].tolist()) == aho.counts(head[s].tolist(), tail[s].tolist(), a, ks, 500)


def _toy_tree(tmp_path, monkeypatch):
    """The synthetic tree, data and checkpoint of test_eval_entry_gpu.py, plus the reasoner_oracle overlay."""
    from evi_rag_amd import packed_dataset as pd, synthetic
    from evi_rag_amd.retriever import Retriever
    from tests.config_tree import write_tree
    from tests.test_reasoner_oracle_cpu import write_oracle_overlay

    data_dir = tmp_path / "data"
    monkeypatch.setenv("EVI_TEST_PROJECT_ROOT", str(tmp_path / "proj"))
    cfg_dir = write_tree(tmp_path, data_dir)
    write_oracle_overlay(cfg_dir)
    rng = np.random.default_rng(5)
    ent = torch.from_numpy(rng.standard_normal((2000, 16)).astype(np.float32))
    rel = torch.from_numpy(rng.standard_normal((9, 16)).astype(np.float32))
    for variant, seed in (("toyqa", 1), ("toyqa-sub", 2)):
        emb = data_dir / variant / "materialized" / "embeddings"
        emb.mkdir(parents=True)
        torch.save(ent, emb / "entity_embeddings.pt")
        torch.save(rel, emb / "relation_embeddings.pt")
        for split, graphs in (("validation", 6), ("test", 9)):
            base = synthetic.make_batch(graphs, nodes_per_graph=40, edges_per_graph=150, emb_dim=16, num_relations=9, seed=seed * 10 + graphs)
            pd.write_packed(emb / f"{split}.packed", pd.samples_from_flat_batch(base))
    torch.manual_seed(3)
    trained = Retriever(emb_dim=16, hidden_dim=16)
    torch.save({"state_dict": {f"model.{k}": v for k, v in trained.state_dict().items()}, "global_step": 1}, tmp_path / "retriever.ckpt")
    return cfg_dir, data_dir, trained


def test_reasoner_oracle_entry_point_end_to_end(dev, tmp_path, monkeypatch):
    from evi_rag_amd import eval as ev

    cfg_dir, data_dir, _ = _toy_tree(tmp_path, monkeypatch)
    ev.run(cfg_dir, ["experiment=eval_retriever", "dataset=toyqa", f"ckpt.retriever={tmp_path / 'retriever.ckpt'}"], device=str(dev))
    results = ev.run(cfg_dir, ["experiment=reasoner_oracle", "dataset=toyqa"], device=str(dev))
    assert [(v, s) for v, s, _ in results] == [("toyqa", "test"), ("toyqa-sub", "test")]
    out_dir = tmp_path / "proj" / "logs" / "reasoner_oracle_toyqa" / "runs" / "fixed"
    ks = [1, 5, 20]
    for variant, _, metrics in results:
        payload = torch.load(data_dir / "toyqa" / "artifacts" / variant / "eval_retriever" / "test.pt", weights_only=True)
        jsonl, metrics_text = aho.files(aho.samples_from_cache(payload, max(ks)), ks)
        pred = out_dir / f"{variant}-oracle-test.jsonl"
        assert pred.read_text() == jsonl
        assert pred.with_suffix(".metrics.json").read_text() == metrics_text
        assert (out_dir / f"metrics_{variant}.json").read_text() == metrics_text  # predict_metrics, under the run's naming
        assert json.dumps(metrics, indent=2) == metrics_text and metrics["oracle/total"] == 9.0
    with pytest.raises(NotImplementedError, match="not part of this backend"):
        ev.run(cfg_dir, ["experiment=reasoner_oracle", "dataset=toyqa", "model.mode=llm"], device=str(dev))


def test_oracle_agrees_with_answer_hit_at_k(dev, tmp_path, monkeypatch):
    """Where every graph has edges and answers, the oracle over the persisted top-k lists is AnswerHitAtK over the logits."""
    from evi_rag_amd import eval as ev
    from evi_rag_amd import metrics as M
    from evi_rag_amd import packed_dataset as pd
    from evi_rag_amd.embedding_store import GlobalEmbeddingStore
    from evi_rag_amd.retriever import Retriever

    cfg_dir, data_dir, trained = _toy_tree(tmp_path, monkeypatch)
    ev.run(cfg_dir, ["experiment=eval_retriever", "dataset=toyqa", f"ckpt.retriever={tmp_path / 'retriever.ckpt'}"], device=str(dev))
    (_, _, oracle), = ev.run(cfg_dir, ["experiment=reasoner_oracle", "dataset=toyqa", "run.dataset_variants=null",
                                       "run.require_dual_datasets=false"], device=str(dev))
    emb_dir = data_dir / "toyqa" / "materialized" / "embeddings"
    store = GlobalEmbeddingStore(emb_dir, device=dev)
    ds = pd.PackedRetrievalDataset(emb_dir / "test.packed", device=dev, embeddings=store)
    model = Retriever(emb_dim=16, hidden_dim=16).to(dev).eval()
    model.load_state_dict(trained.state_dict())
    ks = [1, 5, 20]
    metric = M.AnswerHitAtK(ks)
    n = 0
    with torch.no_grad():
        for batch in pd.PackedLoader(ds, batch_size=4):
            out = model(batch)
            assert bool((batch.answer_entity_ids_ptr.diff() > 0).all())
            metric.update(preds=out.logits.view(-1), target=batch.labels.view(-1) > 0.5, indexes=out.query_ids.view(-1).long(),
                          batch=batch, num_graphs=int(batch.num_graphs))
            n += int(batch.num_graphs)
    got = {k: float(v) for k, v in metric.compute().items()}
    assert oracle["oracle/total"] == n == 9
    for k in ks:
        hit, rec = got[f"answer_hit@{k}"], got[f"answer_recall@{k}"]
        # AnswerHitAtK returns its means as f32 tensors: the hit sums are integers, so the f32 means agree exactly
        assert hit == float(np.float32(oracle[f"oracle/answer_hit@{k}"])), k
        assert abs(rec - oracle[f"oracle/answer_recall@{k}"]) <= 1e-6, k
