"""CPU restatement of the BFS candidate-chain builder (src/data/components/bfs_chain_builder.py:49-311), written from its
documented contract rather than its code: level-by-level enumeration over an oriented, ranked adjacency, signature
de-duplication, a stable (frequency, length, score) ranking.  It is the independent check the device path is tested
against; it is not used by the package."""
from __future__ import annotations

import json
from typing import Any, Dict, List, Mapping, Optional, Sequence


def _adjacency(num_nodes: int, heads: Sequence[int], tails: Sequence[int], scores: Sequence[float], allow_backward: bool,
               max_branch: Optional[int]) -> List[List[tuple]]:
    """Per node: (edge, direction, src, dst, score) entries, best score first, then edge id, then direction."""
    out: List[List[tuple]] = [[] for _ in range(num_nodes)]
    for e in range(len(heads)):
        h, t, sc = int(heads[e]), int(tails[e]), float(scores[e])
        out[h].append((e, 0, h, t, sc))
        if allow_backward:
            out[t].append((e, 1, t, h, sc))
    for lst in out:
        lst.sort(key=lambda x: (-(x[4] + 0.0), x[0], x[1]))  # + 0.0 folds -0.0 into +0.0
        if max_branch is not None and int(max_branch) >= 0:
            del lst[int(max_branch):]
    return out


def enumerate_chains(sample: Mapping[str, Any], settings: Mapping[str, Any]) -> List[dict]:
    """Chains of length >= min_chain_length in breadth-first order: [{'steps': [entry, ...], 'score': float}]."""
    seeds = [int(s) for s in sample["start_node_locals"]]
    n = len(sample["node_entity_ids"])
    adj = _adjacency(n, sample["edge_head_locals"], sample["edge_tail_locals"], sample["edge_scores"],
                     bool(settings["allow_backward"]), settings["max_branch_per_node"])
    max_len, min_len = int(settings["max_chain_length"]), int(settings["min_chain_length"])
    cap = int(settings["max_total_chains"])
    no_edge, no_node = bool(settings["forbid_edge_revisit"]), bool(settings["forbid_node_revisit"])
    level = []
    for s in seeds:
        if 0 <= s < n:
            level.extend({"steps": [x], "score": x[4], "seed": s} for x in adj[s])
    out: List[dict] = []
    depth = 1
    while level:
        nxt = []
        for ch in level:
            if depth >= min_len:
                out.append(ch)
                if cap > 0 and len(out) >= cap:
                    return out
            if depth >= max_len:
                continue
            edges = {x[0] for x in ch["steps"]}
            nodes = {ch["seed"]} | {x[3] for x in ch["steps"]}
            for x in adj[ch["steps"][-1][3]]:
                if no_edge and x[0] in edges:
                    continue
                if no_node and x[3] in nodes:
                    continue
                nxt.append({"steps": ch["steps"] + [x], "score": ch["score"] + x[4], "seed": ch["seed"]})
        level = nxt
        depth += 1
    return out


def candidate_chains(sample: Mapping[str, Any], settings: Mapping[str, Any]) -> List[Dict[str, Any]]:
    """The reference's candidate list for one sample (dicts in its key order)."""
    if len(sample["start_node_locals"]) == 0:
        return []
    if int(settings["max_chain_length"]) <= 0:
        raise ValueError("max_chain_length must be a positive integer.")
    ent = [int(v) for v in sample["node_entity_ids"]]
    rel = [int(v) for v in sample["edge_relations"]]
    heads, tails = sample["edge_head_locals"], sample["edge_tail_locals"]
    groups: Dict[tuple, dict] = {}
    order: List[tuple] = []
    for ch in enumerate_chains(sample, settings):
        sig = tuple((ent[x[2]], rel[x[0]], ent[x[3]]) for x in ch["steps"])
        g = groups.get(sig)
        if g is None:
            groups[sig] = {"freq": 1, "best": ch}
            order.append(sig)
        else:
            g["freq"] += 1
            if ch["score"] > g["best"]["score"]:
                g["best"] = ch
    cands = []
    for first, sig in enumerate(order):
        g = groups[sig]
        cands.append((-g["freq"], -len(sig), -g["best"]["score"], first, sig, g))
    cands.sort(key=lambda c: c[:4])
    limit = settings.get("max_chains_per_sample")
    if limit is not None:
        cands = cands[:max(int(limit), 0)]
    result = []
    for rank, (_, _, _, _, sig, g) in enumerate(cands, 1):
        steps = g["best"]["steps"]
        result.append({
            "signature": [list(t) for t in sig],
            "length": len(steps),
            "frequency": g["freq"],
            "score": float(g["best"]["score"]),
            "edge_local_ids": [x[0] for x in steps],
            "chain_edges": [{"edge_id": x[0], "head_entity_id": ent[int(heads[x[0]])], "tail_entity_id": ent[int(tails[x[0]])],
                             "relation_id": rel[x[0]], "src_entity_id": ent[x[2]], "dst_entity_id": ent[x[3]],
                             "src_node_local": x[2], "dst_node_local": x[3], "direction": x[1]} for x in steps],
            "rank": rank,
        })
    return result


def jsonl_lines(samples: Sequence[Mapping[str, Any]], settings: Mapping[str, Any]) -> List[str]:
    """One JSON line per sample, as export_bfs_chain_cache writes them."""
    return [json.dumps({"sample_id": str(s["sample_id"]), "question": str(s["question"]),
                        "candidate_chains": candidate_chains(s, settings)}) for s in samples]


def sample_as_lists(sample) -> Dict[str, Any]:
    """A GAgentSample (tensor fields) or a record dict -> the plain-list view the functions above read."""
    get = (lambda k: sample[k]) if isinstance(sample, Mapping) else (lambda k: getattr(sample, k))

    def flat(v):
        return v.reshape(-1).tolist() if hasattr(v, "reshape") else list(v)

    out = {k: flat(get(k)) for k in ("node_entity_ids", "edge_head_locals", "edge_tail_locals", "edge_relations",
                                     "edge_scores", "start_node_locals")}
    out["edge_scores"] = [float(v) for v in out["edge_scores"]]
    out["sample_id"], out["question"] = get("sample_id"), get("question")
    return out
