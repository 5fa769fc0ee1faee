"""CPU restatement of the retriever-oracle run (reference: src/models/reasoner_module.py:17-68, 190-273) and the recipes
that turn the compact cases of tests/golden/reasoner_oracle.json.gz into eval_retriever caches.  Shared by the fixture's
generator and the tests, so both build the same files."""
from __future__ import annotations

import json
from pathlib import Path
from typing import Any, Callable, Dict, List, Sequence, Tuple

import torch


# ---- the oracle, rank by rank ------------------------------------------------------------------------------------------
def sample_oracle(heads: Sequence[int], tails: Sequence[int], answers: Sequence[int], ks: Sequence[int]) -> Dict[str, float]:
    """_oracle_metrics_for_sample with Python sets: the found set after each rank, read at every k."""
    uniq = set(int(a) for a in answers)
    if not uniq or not heads:
        out = {f"answer_hit@{k}": 0.0 for k in ks}
        out.update({f"answer_recall@{k}": 0.0 for k in ks})
        return out
    found: set = set()
    state = []  # found-set size after ranks 1..r
    for h, t in zip(heads[:max(ks)], tails[:max(ks)]):
        if h in uniq:
            found.add(h)
        if t in uniq:
            found.add(t)
        state.append(len(found))
    out = {}
    for k in ks:
        n = state[min(k, len(state)) - 1]
        out[f"answer_hit@{k}"] = 1.0 if n else 0.0
        out[f"answer_recall@{k}"] = float(n / len(uniq))
    return out


def counts(heads: Sequence[int], tails: Sequence[int], answers: Sequence[int], ks: Sequence[int],
           max_scan_k: int) -> Tuple[int, List[int]]:
    """(distinct answers, distinct answers among ranks 1..min(E, max_scan_k, k) per k): the kernel's contract."""
    uniq = set(int(a) for a in answers)
    out = []
    for k in ks:
        m = min(len(heads), max_scan_k, k)
        out.append(len(uniq & (set(heads[:m]) | set(tails[:m]))))
    return len(uniq), out


def rows(samples: Sequence[Dict[str, Any]], ks: Sequence[int]) -> List[Dict[str, Any]]:
    return [{"id": s["id"], "question": s["question"], "answer_entity_ids": s["answer_entity_ids"],
             "oracle": sample_oracle(s["head_entity_ids"], s["tail_entity_ids"], s["answer_entity_ids"], ks)} for s in samples]


def files(samples: Sequence[Dict[str, Any]], ks: Sequence[int]) -> Tuple[str, str]:
    """(JSONL text, .metrics.json text) of the oracle run over `samples` (the datamodule's sample dicts)."""
    rs = rows(samples, ks)
    sums = {f"answer_hit@{k}": 0.0 for k in ks}
    sums.update({f"answer_recall@{k}": 0.0 for k in ks})
    for r in rs:
        for key in sums:
            sums[key] += float(r["oracle"][key])
    n = float(max(len(rs), 1))
    metrics = {"oracle/total": float(len(rs))}
    for k in ks:
        metrics[f"oracle/answer_hit@{k}"] = sums[f"answer_hit@{k}"] / n
        metrics[f"oracle/answer_recall@{k}"] = sums[f"answer_recall@{k}"] / n
    return "".join(json.dumps(r) + "\n" for r in rs), json.dumps(metrics, indent=2)


def samples_from_cache(payload: Dict[str, Any], max_k: int) -> List[Dict[str, Any]]:
    """The datamodule's sample dicts from a loaded eval_retriever payload (no checks)."""
    out = []
    for rec in payload["samples"]:
        tbk = rec["triplets_by_k"]
        edges = tbk[max_k] if max_k in tbk else tbk[str(max_k)]
        out.append({"id": str(rec["sample_id"]), "question": str(rec["question"]),
                    "answer_entity_ids": [int(a) for a in rec["answer_entity_ids"]],
                    "head_entity_ids": [int(e["head_entity_id"]) for e in edges],
                    "tail_entity_ids": [int(e["tail_entity_id"]) for e in edges]})
    return out


# ---- compact case -> cache ---------------------------------------------------------------------------------------------
def expand_record(spec: Dict[str, Any], cache_ks: Sequence[int], str_keys: bool) -> Dict[str, Any]:
    """One compact sample ({id, question, answers, heads, tails}) -> the record RetrieverTopKEdgeWriter writes: edge i has
    relation i % 7, score 1 - i / 1024, label 0, rank i + 1; triplets_by_k[k] holds the first min(k, E) edges."""
    heads, tails = spec["heads"], spec["tails"]
    tbk = {}
    for k in cache_ks:
        rows_k = [{"head_entity_id": int(heads[i]), "relation_id": i % 7, "tail_entity_id": int(tails[i]), "head_text": None,
                   "relation_text": None, "tail_text": None, "score": 1.0 - i / 1024.0, "label": 0.0, "rank": i + 1}
                  for i in range(min(int(k), len(heads)))]
        tbk[str(k) if str_keys else int(k)] = rows_k
    return {"sample_id": spec["id"], "question": spec["question"], "triplets_by_k": tbk, "answer_entity_ids": list(spec["answers"])}


def write_cache(out_dir: Path, split: str, payload: Any, manifest: Any = "default") -> Path:
    out_dir = Path(out_dir)
    out_dir.mkdir(parents=True, exist_ok=True)
    path = out_dir / f"{split}.pt"
    torch.save(payload, path)
    if manifest == "default":
        manifest = {"artifact": "eval_retriever", "schema_version": 1, "file": path.name, "created_at": "2026-01-01T00:00:00Z",
                    "producer": "retriever_topk_edge_writer"}
    if manifest is not None:
        (out_dir / f"{split}.manifest.json").write_text(json.dumps(manifest, indent=2), encoding="utf-8")
    return path


def write_case(out_dir: Path, case: Dict[str, Any]) -> Path:
    records = [expand_record(s, case["cache_ks"], case["str_keys"]) for s in case["samples"]]
    return write_cache(out_dir, "test", {"settings": {"split": "test", "topk_values": list(case["cache_ks"])}, "samples": records})


# ---- refusals: name -> writes the files, returns the eval_retriever_path the datamodule is given --------------------------
def _good(**over) -> Dict[str, Any]:
    rec = expand_record({"id": "q0", "question": "who?", "answers": [3], "heads": [1, 2], "tails": [3, 4]}, [1, 5], False)
    rec.update(over)
    return rec


def _payload(*records) -> Dict[str, Any]:
    return {"settings": {"split": "test", "topk_values": [1, 5]}, "samples": list(records)}


def _manifest(**over) -> Dict[str, Any]:
    m = {"artifact": "eval_retriever", "schema_version": 1, "file": "test.pt"}
    m.update(over)
    return {k: v for k, v in m.items() if v is not None}


def _legacy(d: Path) -> Path:
    d.mkdir(parents=True, exist_ok=True)
    torch.save(_payload(_good()), d / "test_eval_retriever.pt")
    return d / "test.pt"


REFUSALS: Dict[str, Callable[[Path], Path]] = {
    "missing_file": lambda d: d / "test.pt",
    "legacy_name": _legacy,
    "missing_manifest": lambda d: write_cache(d, "test", _payload(_good()), manifest=None),
    "manifest_no_artifact": lambda d: write_cache(d, "test", _payload(_good()), _manifest(artifact=None)),
    "manifest_artifact_mismatch": lambda d: write_cache(d, "test", _payload(_good()), _manifest(artifact="eval_bfs")),
    "manifest_no_schema": lambda d: write_cache(d, "test", _payload(_good()), _manifest(schema_version=None)),
    "manifest_schema_mismatch": lambda d: write_cache(d, "test", _payload(_good()), _manifest(schema_version=2)),
    "manifest_no_file": lambda d: write_cache(d, "test", _payload(_good()), _manifest(file=None)),
    "manifest_file_mismatch": lambda d: write_cache(d, "test", _payload(_good()), _manifest(file="other.pt")),
    "payload_list": lambda d: write_cache(d, "test", [_good()]),
    "payload_no_samples": lambda d: write_cache(d, "test", {"settings": {}}),
    "samples_empty": lambda d: write_cache(d, "test", _payload()),
    "sample_not_dict": lambda d: write_cache(d, "test", _payload(_good(), [1, 2])),
    "sample_id_empty": lambda d: write_cache(d, "test", _payload(_good(sample_id=""))),
    "answers_empty": lambda d: write_cache(d, "test", _payload(_good(), _good(sample_id="q7", answer_entity_ids=[]))),
    "triplets_by_k_missing": lambda d: write_cache(d, "test", _payload(_good(triplets_by_k=None))),
    "triplets_by_k_missing_k": lambda d: write_cache(d, "test", _payload(_good(triplets_by_k={1: [], "5": [], 50: [], "10": []}))),
    "triplets_by_k_not_list": lambda d: write_cache(d, "test", _payload(_good(triplets_by_k={5: {"a": 1}}))),
}
REFUSAL_K_VALUES = {"triplets_by_k_missing_k": [1, 20]}  # the k list the datamodule is given (default [1, 5])
