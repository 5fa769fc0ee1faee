"""GPU: BFS candidate chains through evi_bfs_chains — the reference's recorded lines byte for byte, a random settings grid
and a hub sample against the CPU restatement, batching / chunking / LDS / hash-width invariance, the export's files."""
import gzip
import json
import os
import re

import numpy as np
import pytest
import torch

from tests import bfs_chain_oracle as oracle

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "bfs_chains.json.gz")
_FLOATS = ("edge_scores", "edge_labels", "question_emb")


def golden_cases():
    with gzip.open(GOLDEN, "rt", encoding="utf-8") as fh:
        return json.load(fh)["cases"]


def tensor_record(rec):
    return {k: (torch.tensor(v, dtype=torch.float32 if k in _FLOATS else torch.long) if isinstance(v, list) else v)
            for k, v in rec.items()}


def as_sample(rec):
    from evi_rag_amd.g_agent import GAgentSample

    t = tensor_record(rec)
    fields = set(GAgentSample.__dataclass_fields__)
    return GAgentSample(**{k: v for k, v in t.items() if k in fields})


def settings_of(d):
    from evi_rag_amd.bfs_chains import BFSChainSettings

    return BFSChainSettings(**d)


def lines_of(samples, chains):
    return [json.dumps({"sample_id": str(s.sample_id), "question": str(s.question), "candidate_chains": c})
            for s, c in zip(samples, chains)]


@pytest.mark.parametrize("case", golden_cases(), ids=lambda c: c["name"])
def test_device_path_equals_reference_lines(case, tmp_path):
    from evi_rag_amd import bfs_chains as bc

    settings = settings_of(case["settings"])
    if case["mode"] == "export":
        path = tmp_path / "test_g_agent.pt"
        torch.save({"samples": [tensor_record(r) for r in case["records"]]}, path)
        out, total = bc.export_bfs_chain_cache(g_agent_path=path, output_dir=tmp_path / "eval_bfs", split="test", settings=settings,
                                               drop_unreachable=case["drop_unreachable"])
        got = out.read_text().splitlines()
        assert total == len(case["lines"])
        manifest = json.loads((tmp_path / "eval_bfs" / "test.manifest.json").read_text())
        want = dict(case["manifest"])
        assert re.fullmatch(r"\d{4}-\d\d-\d\dT\d\d:\d\d:\d\dZ", manifest.pop("created_at"))
        want.pop("created_at")
        assert manifest == want and list(manifest) == [k for k in case["manifest"] if k != "created_at"]
    else:
        samples = [as_sample(r) for r in case["records"]]
        got = lines_of(samples, bc.build_bfs_candidate_chains_batch(samples, settings=settings))
    assert len(got) == len(case["lines"])
    for i, (a, b) in enumerate(zip(got, case["lines"])):
        assert a == b, f"{case['name']} line {i}"


def random_record(rng, sid, n, e, *, seeds=2, hub=False):
    heads = rng.integers(0, n, e)
    tails = rng.integers(0, n, e)
    if hub:  # power-law-ish: a third of the edges touch node 0
        heads[: e // 3] = 0
    scores = (rng.integers(0, 7, e) / 7).astype(np.float32) if rng.random() < 0.5 else rng.standard_normal(e).astype(np.float32)
    return {"sample_id": sid, "question": f"q {sid}", "question_emb": [0.0], "node_entity_ids": (rng.permutation(5 * n)[:n] + 7).tolist(),
            "node_embedding_ids": list(range(n)), "edge_head_locals": heads.tolist(), "edge_tail_locals": tails.tolist(),
            "edge_relations": rng.integers(0, 3, e).tolist(), "edge_scores": scores.tolist(), "edge_labels": [0.0] * e,
            "start_entity_ids": [7], "answer_entity_ids": [7], "gt_path_edge_local_ids": [],
            "start_node_locals": ([0] if hub else []) + rng.integers(-1, n + 1, seeds).tolist()}


def test_random_settings_grid_against_restatement():
    from evi_rag_amd import bfs_chains as bc

    rng = np.random.default_rng(11)
    for trial in range(24):
        recs = [random_record(rng, f"r{trial}_{i}", int(rng.integers(3, 25)), int(rng.integers(1, 60)), seeds=int(rng.integers(0, 4)))
                for i in range(5)]
        d = {"max_chain_length": int(rng.integers(1, 5)), "min_chain_length": int(rng.integers(0, 4)),
             "max_chains_per_sample": int(rng.choice([-1, 0, 3, 100])), "max_total_chains": int(rng.choice([0, 1, 17, 300, 5000])),
             "allow_backward": bool(rng.integers(2)), "max_branch_per_node": [None, -1, 0, 1, 3][int(rng.integers(5))],
             "forbid_edge_revisit": bool(rng.integers(2)), "forbid_node_revisit": bool(rng.integers(2))}
        if d["max_total_chains"] == 0 and not (d["forbid_node_revisit"] or d["max_chain_length"] <= 3):
            d["max_chain_length"] = 3  # keeps the unbounded enumerations small for the restatement
        samples = [as_sample(r) for r in recs]
        got = lines_of(samples, bc.build_bfs_candidate_chains_batch(samples, settings=settings_of(d)))
        want = oracle.jsonl_lines([oracle.sample_as_lists(s) for s in samples], d)
        assert got == want, d


def test_hub_sample_takes_the_global_memory_path():
    from evi_rag_amd import bfs_chains as bc

    rng = np.random.default_rng(3)
    rec = random_record(rng, "hub", 400, 900, seeds=1, hub=True)
    s = as_sample(rec)
    # 20 000 chains of records are more than an LDS holds (8 140): the expansion runs in global memory
    d = {"max_chain_length": 3, "min_chain_length": 1, "max_chains_per_sample": 100, "max_total_chains": 20000,
         "allow_backward": True, "max_branch_per_node": None, "forbid_edge_revisit": True, "forbid_node_revisit": False}
    stats = {}
    got = lines_of([s], bc.build_bfs_candidate_chains_batch([s], settings=settings_of(d), stats=stats))
    assert stats["raw_chains"] == 20000
    assert got == oracle.jsonl_lines([oracle.sample_as_lists(s)], d)
    # an unbounded enumeration (max_total_chains = 0) sizes the sample again from what the device reports
    d2 = dict(d, max_total_chains=0)
    stats2 = {}
    got2 = lines_of([s], bc.build_bfs_candidate_chains_batch([s], settings=settings_of(d2), stats=stats2))
    assert stats2["raw_chains"] > 2 * 4096 and stats2["launches"] >= 2
    assert got2 == oracle.jsonl_lines([oracle.sample_as_lists(s)], d2)


def test_batch_equals_single_calls_and_knobs_do_not_matter():
    from evi_rag_amd import bfs_chains as bc

    rng = np.random.default_rng(5)
    recs = [random_record(rng, f"b{i}", int(rng.integers(5, 60)), int(rng.integers(0, 150)), seeds=int(rng.integers(0, 4)))
            for i in range(150)]
    samples = [as_sample(r) for r in recs]
    settings = settings_of({"max_chain_length": 3, "min_chain_length": 1, "max_chains_per_sample": 50, "max_total_chains": 700,
                            "allow_backward": True, "max_branch_per_node": None, "forbid_edge_revisit": True,
                            "forbid_node_revisit": False})
    ref = bc.build_bfs_candidate_chains_batch(samples, settings=settings)
    for s, c in zip(samples[:12], ref[:12]):
        assert bc.build_bfs_candidate_chains(s, settings=settings) == c
    assert bc.build_bfs_candidate_chains_batch(samples, settings=settings, chunk_size=7) == ref
    assert bc.build_bfs_candidate_chains_batch(samples, settings=settings, chunk_size=1000, use_lds=False) == ref
    # a 2-bit signature hash: nearly every pair of signatures collides, and the full comparison keeps them apart
    assert bc.build_bfs_candidate_chains_batch(samples, settings=settings, hash_bits=2) == ref
    assert bc.build_bfs_candidate_chains_batch(samples, settings=settings, hash_bits=1, use_lds=False) == ref


def test_export_files_append_and_return_value(tmp_path):
    from evi_rag_amd import bfs_chains as bc

    rng = np.random.default_rng(9)
    recs = []
    for i in range(4):
        r = random_record(rng, f"e{i}", 12, 30, seeds=2)
        r["start_node_locals"] = [v for v in r["start_node_locals"] if 0 <= v < 12] or [0]
        r.update(answer_node_locals=[1] if i % 2 == 0 else [], pair_start_node_locals=[], pair_answer_node_locals=[],
                 pair_edge_local_ids=[], pair_edge_counts=[], pair_shortest_lengths=[], gt_path_exists=False,
                 is_answer_reachable=i % 2 == 0)
        recs.append(r)
    path = tmp_path / "g.pt"
    torch.save({"samples": [tensor_record(r) for r in recs]}, path)
    settings = bc.BFSChainSettings(max_chain_length=2)
    out, n = bc.export_bfs_chain_cache(g_agent_path=path, output_dir=tmp_path / "o", split="val", settings=settings,
                                       artifact_name=" art ", schema_version=3)
    assert (out, n) == ((tmp_path / "o" / "val.jsonl").resolve(), 4)
    first = out.read_text().splitlines()
    out2, n2 = bc.export_bfs_chain_cache(g_agent_path=path, output_dir=tmp_path / "o", split="val", settings=settings,
                                         overwrite=False, drop_unreachable=True)
    assert n2 == 2 and out2 == out
    both = out.read_text().splitlines()
    assert both[:4] == first and both[4:] == [first[0], first[2]]
    m = json.loads((tmp_path / "o" / "val.manifest.json").read_text())
    assert list(m) == ["artifact", "schema_version", "file", "created_at", "producer", "settings"]
    assert m["file"] == "val.jsonl" and m["producer"] == "bfs_chain_builder" and m["artifact"] == "eval_bfs"
    assert m["settings"] == {"max_chain_length": 2, "min_chain_length": 1, "max_chains_per_sample": 100, "max_total_chains": 5000,
                             "allow_backward": True, "max_branch_per_node": None, "forbid_edge_revisit": True,
                             "forbid_node_revisit": False}
    samples = [as_sample(r) for r in recs]
    assert first == oracle.jsonl_lines([oracle.sample_as_lists(s) for s in samples], oracle_settings(settings))


def oracle_settings(s):
    return {k: getattr(s, k) for k in ("max_chain_length", "min_chain_length", "max_chains_per_sample", "max_total_chains",
                                       "allow_backward", "max_branch_per_node", "forbid_edge_revisit", "forbid_node_revisit")}


def test_eval_entry_writes_chains_from_its_own_g_agent_cache(dev, tmp_path, monkeypatch):
    from evi_rag_amd import eval as ev
    from evi_rag_amd import packed_dataset as pd, synthetic
    from evi_rag_amd.g_agent import load_g_agent_samples
    from evi_rag_amd.retriever import Retriever
    from tests.config_tree import write_tree

    data_dir = tmp_path / "data"
    monkeypatch.setenv("EVI_TEST_PROJECT_ROOT", str(tmp_path / "proj"))
    cfg_dir = write_tree(tmp_path, data_dir)
    rng = np.random.default_rng(5)
    emb = data_dir / "toyqa" / "materialized" / "embeddings"
    emb.mkdir(parents=True)
    torch.save(torch.from_numpy(rng.standard_normal((2000, 16)).astype(np.float32)), emb / "entity_embeddings.pt")
    torch.save(torch.from_numpy(rng.standard_normal((9, 16)).astype(np.float32)), emb / "relation_embeddings.pt")
    base = synthetic.make_batch(9, nodes_per_graph=40, edges_per_graph=150, emb_dim=16, num_relations=9, seed=19)
    pd.write_packed(emb / "test.packed", pd.samples_from_flat_batch(base))
    torch.manual_seed(3)
    torch.save({"state_dict": {f"model.{k}": v for k, v in Retriever(emb_dim=16, hidden_dim=16).state_dict().items()}},
               tmp_path / "retriever.ckpt")
    common = ["experiment=eval_retriever", "dataset=toyqa", f"ckpt.retriever={tmp_path / 'retriever.ckpt'}",
              "run.dataset_variants=null", "run.require_dual_datasets=false", "run.run_all_splits=false", "run.split=test",
              "run.build_g_agent=true", "run.allow_empty_answer=true"]
    art = data_dir / "toyqa" / "artifacts" / "toyqa"
    out_dir = tmp_path / "proj" / "logs" / "eval_retriever_toyqa" / "runs" / "fixed"

    (_, _, plain), = ev.run(cfg_dir, common, device=str(dev))
    assert not (art / "eval_bfs").exists() and "bfs_chain/total" not in plain
    assert json.loads((out_dir / "metrics.json").read_text()) == plain

    (_, _, metrics), = ev.run(cfg_dir, common + ["+bfs_chain_eval.enabled=true", "+bfs_chain_eval.max_chain_length=3"], device=str(dev))
    samples = load_g_agent_samples(art / "g_agent" / "test_g_agent.pt")
    assert metrics["bfs_chain/total"] == float(len(samples)) and len(samples) > 0
    assert json.loads((out_dir / "metrics.json").read_text()) == metrics
    assert {k: v for k, v in metrics.items() if k != "bfs_chain/total"} == plain
    got = (art / "eval_bfs" / "test.jsonl").read_text().splitlines()
    d = {"max_chain_length": 3, "min_chain_length": 1, "max_chains_per_sample": 100, "max_total_chains": 5000,
         "allow_backward": True, "max_branch_per_node": None, "forbid_edge_revisit": True, "forbid_node_revisit": False}
    assert got == oracle.jsonl_lines([oracle.sample_as_lists(s) for s in samples], d)
    assert (art / "eval_bfs" / "test.manifest.json").exists()
