#!/usr/bin/env python3
"""Times the BFS chain export (evi_rag_amd.bfs_chains) on a synthetic WebQSP-shaped g_agent cache.

1 628 samples (the WebQSP test split), each about 500 edges (the retriever's top edges united with the seeds' own edges)
over ~300 nodes, 1-3 seeds whose degree follows a power law.  Prints one JSON line: device milliseconds for the split,
host formatting milliseconds, the whole export in seconds (and the part of it spent reading the cache with torch.load),
the CPU restatement's samples/s on a subset, and chain-count statistics (levels reached, samples that hit
max_total_chains).

Usage:  python tools/bfs_chain_bench.py [--samples 1628] [--max-chain-length 3] [--cpu-subset 16]
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def make_cache(path: str, samples: int, seed: int) -> None:
    rng = np.random.default_rng(seed)
    recs = []
    for i in range(samples):
        n = int(rng.integers(200, 400))
        n_seeds = int(rng.integers(1, 4))
        seeds = rng.choice(n, n_seeds, replace=False)
        seed_deg = np.minimum((rng.pareto(1.2, n_seeds) * 8 + 1).astype(np.int64), 250)  # power-law seed degree
        e_top = 500 - int(seed_deg.sum()) if int(seed_deg.sum()) < 450 else 50
        heads = [rng.integers(0, n, e_top)]
        tails = [rng.integers(0, n, e_top)]
        for s, d in zip(seeds, seed_deg):
            other = rng.integers(0, n, int(d))
            out = rng.random(int(d)) < 0.5
            heads.append(np.where(out, s, other))
            tails.append(np.where(out, other, s))
        h, t = np.concatenate(heads), np.concatenate(tails)
        e = h.shape[0]
        ent = np.sort(rng.choice(2_000_000, n, replace=False))
        recs.append({
            "sample_id": f"WebQTest-{i}", "question": f"synthetic question {i}", "question_emb": torch.zeros(1, 4),
            "edge_relations": torch.from_numpy(rng.integers(0, 6000, e)), "edge_scores": torch.from_numpy(rng.random(e).astype(np.float32)),
            "edge_labels": torch.zeros(e), "edge_head_locals": torch.from_numpy(h), "edge_tail_locals": torch.from_numpy(t),
            "node_entity_ids": torch.from_numpy(ent), "node_embedding_ids": torch.from_numpy(ent),
            "start_entity_ids": torch.from_numpy(ent[seeds]), "start_node_locals": torch.from_numpy(seeds.astype(np.int64)),
            "answer_entity_ids": torch.from_numpy(ent[:1]), "answer_node_locals": torch.zeros(1, dtype=torch.long),
            "pair_start_node_locals": torch.zeros(0, dtype=torch.long), "pair_answer_node_locals": torch.zeros(0, dtype=torch.long),
            "pair_edge_local_ids": torch.zeros(0, dtype=torch.long), "pair_edge_counts": torch.zeros(0, dtype=torch.long),
            "pair_shortest_lengths": torch.zeros(0, dtype=torch.long), "gt_path_edge_local_ids": torch.zeros(0, dtype=torch.long),
            "gt_path_exists": False, "is_answer_reachable": True, "is_dummy_agent": False})
    torch.save({"samples": recs}, path)


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=1628)
    ap.add_argument("--max-chain-length", type=int, default=3)
    ap.add_argument("--cpu-subset", type=int, default=16)
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()

    from evi_rag_amd import bfs_chains as bc
    from evi_rag_amd.g_agent import load_g_agent_samples
    from tests import bfs_chain_oracle as oracle

    settings = bc.BFSChainSettings(max_chain_length=args.max_chain_length)
    with tempfile.TemporaryDirectory() as tmp:
        cache = os.path.join(tmp, "test_g_agent.pt")
        make_cache(cache, args.samples, args.seed)
        # warm-up: library load, context, first-launch costs
        bc.export_bfs_chain_cache(g_agent_path=cache, output_dir=os.path.join(tmp, "warm"), split="test", settings=settings)
        stats: dict = {}
        t0 = time.perf_counter()
        out, total = bc.export_bfs_chain_cache(g_agent_path=cache, output_dir=os.path.join(tmp, "eval_bfs"), split="test",
                                               settings=settings, stats=stats)
        export_s = time.perf_counter() - t0
        lines = out.read_text().splitlines()
        samples = load_g_agent_samples(cache)[: args.cpu_subset]
        sdict = {k: getattr(settings, k) for k in ("max_chain_length", "min_chain_length", "max_chains_per_sample",
                                                   "max_total_chains", "allow_backward", "max_branch_per_node",
                                                   "forbid_edge_revisit", "forbid_node_revisit")}
        plain = [oracle.sample_as_lists(s) for s in samples]
        t0 = time.perf_counter()
        cpu_lines = oracle.jsonl_lines(plain, sdict)
        cpu_s = time.perf_counter() - t0
    cpu_rate = len(samples) / cpu_s if cpu_s > 0 else float("inf")
    print(json.dumps({
        "bench": "bfs_chain_export", "samples": total, "max_chain_length": args.max_chain_length,
        "device_ms": round(stats["device_ms"], 3), "launches": stats["launches"], "host_format_ms": round(1e3 * stats["format_s"], 1),
        "export_s": round(export_s, 3), "cache_load_s": round(stats["load_s"], 3),
        "format_share": round(stats["format_s"] / export_s, 3),
        "chain_stage_s": round(export_s - stats["load_s"], 3),
        "cpu_restatement_samples_per_s": round(cpu_rate, 2), "cpu_subset": len(samples),
        "cpu_split_estimate_s": round(total / cpu_rate, 1), "speedup_vs_cpu": round(total / cpu_rate / export_s, 1),
        "chain_stage_speedup_vs_cpu": round(total / cpu_rate / (export_s - stats["load_s"]), 1),
        "subset_lines_equal": cpu_lines == lines[: len(samples)], "levels_reached": stats["levels_reached"],
        "samples_at_cap": stats["samples_at_cap"], "raw_chains_mean": round(stats["raw_chains"] / max(total, 1), 1)}))
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
