#!/usr/bin/env python3
"""Generates tests/golden/bfs_chains.json.gz by RUNNING THE REFERENCE'S OWN CHAIN BUILDER (build container only).

For every case: synthetic g_agent records, one BFSChainSettings, and the exact JSONL lines (and, for cases that go through
the cache, the manifest) that the reference's `export_bfs_chain_cache` / `build_bfs_candidate_chains` produce.  Cases
whose samples the reference's cache loader refuses (out-of-range seeds, no edges) are run through
`build_bfs_candidate_chains` directly and recorded as the lines the export would write for them.

Usage:  EVI_REFERENCE_ROOT=/path/to/EVI-RAG python tests/golden/make_golden_chains.py
"""
from __future__ import annotations

import gzip
import importlib.abc
import importlib.machinery
import json
import os
import sys
import tempfile
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.environ.get("EVI_REFERENCE_ROOT", os.path.join(os.path.dirname(os.path.dirname(os.path.dirname(HERE))), "EVI-RAG"))
sys.path.insert(0, REF)

_STUB_ROOTS = ("lmdb", "torch_geometric", "torchmetrics", "lightning", "lightning_utilities", "wandb")


class _StubModule(types.ModuleType):
    __path__: list = []

    def __getattr__(self, name):
        if name.startswith("__"):
            raise AttributeError(name)
        cls = type(name, (object,), {"__init__": lambda self, *a, **k: None, "__module__": self.__name__})
        setattr(self, name, cls)
        return cls


class _StubFinder(importlib.abc.MetaPathFinder, importlib.abc.Loader):
    def find_spec(self, fullname, path=None, target=None):
        if fullname.split(".")[0] in _STUB_ROOTS:
            return importlib.machinery.ModuleSpec(fullname, self, is_package=True)
        return None

    def create_module(self, spec):
        return _StubModule(spec.name)

    def exec_module(self, module):
        return None


sys.meta_path.append(_StubFinder())

from src.data.components import bfs_chain_builder as ref  # noqa: E402


def graph(rng, sid, n, e, *, n_rel=4, score_levels=None, seeds=2, self_loops=0, parallel=0, neg_zero=False, reachable=True):
    heads = rng.integers(0, n, e)
    tails = rng.integers(0, n, e)
    rels = rng.integers(0, n_rel, e)
    if score_levels:
        scores = (rng.integers(0, score_levels, e) / score_levels).astype(np.float32)  # many ties
    else:
        scores = rng.standard_normal(e).astype(np.float32)
    for i in range(min(self_loops, e)):
        tails[i] = heads[i]
    for i in range(min(parallel, e // 2)):  # edge 2i+1 parallels edge 2i: same endpoints, relation (so signature), new score
        heads[2 * i + 1], tails[2 * i + 1], rels[2 * i + 1] = heads[2 * i], tails[2 * i], rels[2 * i]
    scores = scores.tolist()
    if neg_zero:
        for i in range(0, e, 3):
            scores[i] = -0.0 if i % 2 else 0.0
    ent = (rng.permutation(10 * n)[:n] + 1000).tolist()
    starts = rng.integers(0, n, seeds).tolist() if seeds else []
    answers = rng.integers(0, n, 1).tolist() if reachable else []
    return {
        "sample_id": sid, "question": f"question {sid}?", "question_emb": [0.5, -0.25],
        "edge_relations": rels.tolist(), "edge_scores": scores, "edge_labels": [0.0] * e,
        "edge_head_locals": heads.tolist(), "edge_tail_locals": tails.tolist(), "node_entity_ids": ent,
        "node_embedding_ids": list(range(n)), "start_entity_ids": [ent[s] for s in starts] or [ent[0]],
        "start_node_locals": starts, "answer_entity_ids": [ent[a] for a in answers], "answer_node_locals": answers,
        "pair_start_node_locals": [], "pair_answer_node_locals": [], "pair_edge_local_ids": [], "pair_edge_counts": [],
        "pair_shortest_lengths": [], "gt_path_edge_local_ids": [], "gt_path_exists": False,
        "is_answer_reachable": bool(starts) and reachable,
    }


def as_tensors(rec):
    out = dict(rec)
    for k, v in rec.items():
        if isinstance(v, list):
            out[k] = torch.tensor(v, dtype=torch.float32 if k in ("edge_scores", "edge_labels", "question_emb") else torch.long)
    return out


def run_export(records, settings, drop_unreachable=False):
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "test_g_agent.pt")
        torch.save({"samples": [as_tensors(r) for r in records]}, path)
        out_path, total = ref.export_bfs_chain_cache(g_agent_path=path, output_dir=os.path.join(tmp, "eval_bfs"), split="test",
                                                     settings=settings, drop_unreachable=drop_unreachable)
        lines = out_path.read_text().splitlines()
        manifest = json.loads((out_path.parent / "test.manifest.json").read_text())
    assert total == len(lines)
    return lines, manifest


def run_build(records, settings):
    lines = []
    for rec in records:
        sample = _parse_sample_loose(rec)
        chains = ref.build_bfs_candidate_chains(sample, settings=settings)
        lines.append(json.dumps({"sample_id": str(rec["sample_id"]), "question": str(rec["question"]), "candidate_chains": chains}))
    return lines


def _parse_sample_loose(rec):
    """A GAgentSample for records the reference's loader refuses (the chain builder itself accepts them)."""
    t = as_tensors(rec)
    return types.SimpleNamespace(**{k: (v.view(-1) if isinstance(v, torch.Tensor) else v) for k, v in t.items()})


def settings_dict(s):
    return {k: getattr(s, k) for k in ("max_chain_length", "min_chain_length", "max_chains_per_sample", "max_total_chains",
                                       "allow_backward", "max_branch_per_node", "forbid_edge_revisit", "forbid_node_revisit")}


def main():
    rng = np.random.default_rng(20261016)
    S = ref.BFSChainSettings
    base = [graph(rng, f"g{i}", 30 + 5 * i, 60 + 20 * i, seeds=2) for i in range(3)]
    small = [graph(rng, f"s{i}", 8, 12, seeds=2) for i in range(3)]
    special = [
        graph(rng, "loops", 12, 30, self_loops=6, seeds=2),
        graph(rng, "parallel", 12, 30, parallel=10, seeds=2),
        graph(rng, "ties", 15, 40, score_levels=3, seeds=3),
        graph(rng, "zeros", 15, 40, score_levels=2, neg_zero=True, seeds=2),
    ]
    special[0]["start_node_locals"] = [special[0]["edge_head_locals"][0]] * 2  # duplicate seed at a self-loop
    special[0]["start_entity_ids"] = [special[0]["node_entity_ids"][special[0]["edge_head_locals"][0]]]
    cases = []

    def add(name, settings, records, mode="export", drop_unreachable=False):
        case = {"name": name, "settings": settings_dict(settings), "mode": mode, "drop_unreachable": drop_unreachable,
                "records": records}
        if mode == "export":
            case["lines"], case["manifest"] = run_export(records, settings, drop_unreachable)
        else:
            case["lines"] = run_build(records, settings)
        cases.append(case)
        print(f"{name}: {sum(len(x) for x in case['lines'])} bytes of lines")

    add("default", S(max_chain_length=3), base)
    add("default_len2", S(max_chain_length=2), base)
    add("no_backward", S(max_chain_length=3, allow_backward=False), base)
    add("edge_revisit_allowed", S(max_chain_length=3, forbid_edge_revisit=False, max_chains_per_sample=30), base[:2])
    add("node_revisit_forbidden", S(max_chain_length=3, forbid_node_revisit=True, max_chains_per_sample=30), base[:2])
    add("node_revisit_forbidden_no_edge", S(max_chain_length=3, forbid_node_revisit=True, forbid_edge_revisit=False,
                                            max_chains_per_sample=30), small)
    add("branch_none", S(max_chain_length=3, max_branch_per_node=None, max_chains_per_sample=30), base[:2])
    add("branch_0", S(max_chain_length=3, max_branch_per_node=0), base[:2])
    add("branch_2", S(max_chain_length=4, max_branch_per_node=2, max_chains_per_sample=30), base)
    add("branch_neg", S(max_chain_length=3, max_branch_per_node=-1, max_chains_per_sample=30), base[:2])
    add("min_len_0", S(max_chain_length=2, min_chain_length=0, max_chains_per_sample=30), base[:2])
    add("min_len_2", S(max_chain_length=3, min_chain_length=2, max_chains_per_sample=30), base)
    add("min_len_2_cap", S(max_chain_length=3, min_chain_length=2, max_total_chains=40, max_chains_per_sample=30), base)
    add("min_len_above_max", S(max_chain_length=2, min_chain_length=3), base[:2])
    add("cap_0_small", S(max_chain_length=3, max_total_chains=0, max_chains_per_sample=30), small)
    add("cap_1", S(max_chain_length=3, max_total_chains=1), base)
    add("cap_37", S(max_chain_length=3, max_total_chains=37), base)
    add("cap_default_reached", S(max_chain_length=4, max_chains_per_sample=20), base[2:])
    add("per_sample_0", S(max_chain_length=2, max_chains_per_sample=0), base[:2])
    add("per_sample_neg", S(max_chain_length=2, max_chains_per_sample=-1), base[:2])
    add("special", S(max_chain_length=3), special)
    add("special_no_edge_revisit", S(max_chain_length=3, forbid_edge_revisit=False, max_chains_per_sample=40), special)
    unreach = [graph(rng, f"u{i}", 10, 20, seeds=2, reachable=(i % 2 == 0)) for i in range(4)]
    add("drop_unreachable", S(max_chain_length=2), unreach, drop_unreachable=True)
    add("keep_unreachable", S(max_chain_length=2), unreach)
    no_seeds = graph(rng, "noseeds", 10, 20, seeds=0)
    add("no_seeds", S(max_chain_length=2), [no_seeds, small[0]])
    oor = graph(rng, "oor", 10, 20, seeds=2)
    oor["start_node_locals"] = [-1, 3, 10, 99, 3]
    empty = graph(rng, "noedges", 5, 0, seeds=2)
    add("direct_out_of_range_seeds_and_no_edges", S(max_chain_length=3), [oor, empty, small[1]], mode="build")

    out = os.path.join(HERE, "bfs_chains.json.gz")
    with open(out, "wb") as raw, gzip.GzipFile(filename="", mode="wb", fileobj=raw, mtime=0) as fh:  # reproducible bytes
        fh.write(json.dumps({"cases": cases}).encode("utf-8"))
    print(f"wrote {out}: {os.path.getsize(out)} bytes, {len(cases)} cases")


if __name__ == "__main__":
    main()
