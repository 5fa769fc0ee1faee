"""Retriever-oracle upper bound from the persisted eval_retriever cache: `experiment=reasoner_oracle` without an LLM.

reference: ReasonerOracleDataModule (src/data/reasoner_oracle_datamodule.py) and ReasonerModule in mode="oracle"
(src/models/reasoner_module.py:17-68, 132-151, 190-285).  The datamodule reads `eval_retriever/<split>.pt` (written by
`topk_writer.RetrieverTopKEdgeWriter`) and keeps each sample's ranked heads and tails at its max k; the module reports,
per sample and k, whether any answer entity appears among the first k ranked triplets (`answer_hit@k`) and which share
of the distinct answers does (`answer_recall@k`), writes `<dataset>-<prompt_tag>-<split>.jsonl` and its
`.metrics.json`, and keeps the aggregate in `predict_metrics`.

The reference walks every rank of every sample in Python.  Here a chunk of samples is packed into flat arrays once,
copied to the device once, `evi_oracle_answer_hits` (csrc/oracle.hip) counts the distinct answers found at each k with
one workgroup per sample, and one device -> host copy returns the counts.  The files are byte-identical to the
reference's.

One difference: the cache is read with `torch.load(weights_only=True)` (the writer stores plain containers), and a file
that needs unpickling is refused with a ValueError instead of being executed.  The LLM reasoner runs (mode="llm") are
not part of this backend.
"""
from __future__ import annotations

import ctypes
import itertools
import json
import logging
import time
from operator import itemgetter
from pathlib import Path
from typing import Any, Dict, Iterator, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib
from .metrics import normalize_k_values

log = logging.getLogger(__name__)

DEFAULT_CHUNK_SAMPLES = 2048
MAX_LDS_ANSWERS = 4096  # csrc/oracle.hip kMaxLdsAnswers
_I32_MAX = 2**31 - 1
_HEAD = itemgetter("head_entity_id")
_TAIL = itemgetter("tail_entity_id")


# ---- the datamodule ----------------------------------------------------------------------------------------------------
class ReasonerOracleDataModule:
    """reference: ReasonerOracleDataModule (same constructor kwargs, checks and sample dicts; no Lightning)."""

    def __init__(self, *, dataset: str, split: str, eval_retriever_path: str, k_values: Sequence[int],
                 artifact_name: str = "eval_retriever", schema_version: int = 1, num_workers: int = 0,
                 prompt_tag: str = "oracle") -> None:
        self.dataset = dataset
        self.split = split
        self.eval_retriever_path = Path(eval_retriever_path).expanduser().resolve()
        self.artifact_name = str(artifact_name).strip()
        if not self.artifact_name:
            raise ValueError("artifact_name must be a non-empty string.")
        self.schema_version = int(schema_version)
        if self.schema_version <= 0:
            raise ValueError("schema_version must be a positive integer.")
        self.k_values = normalize_k_values(k_values)
        if not self.k_values:
            raise ValueError("k_values must be a non-empty list of positive integers.")
        self.max_k = int(max(self.k_values))
        self.num_workers = int(num_workers)
        self.prompt_tag = prompt_tag
        self.data: List[Dict[str, Any]] = []
        self.load_s = 0.0
        self.flatten_s = 0.0

    def setup(self, stage: Optional[str] = None) -> None:
        self.data = self._build_samples()

    def predict_dataloader(self) -> Iterator[List[Dict[str, Any]]]:
        """Batches of one sample, in order (the reference's DataLoader with batch_size=1 and a list collate)."""
        return ([s] for s in self.data)

    def _torch_load(self, path: Path) -> Any:
        try:
            return torch.load(str(path), map_location="cpu", weights_only=True)
        except Exception as exc:  # noqa: BLE001 - torch raises several types for unsafe pickles
            raise ValueError(f"{path} cannot be loaded with weights_only=True ({exc}); an eval_retriever cache holds plain "
                             "containers, and a file that needs unpickling is refused") from exc

    @staticmethod
    def _select_triplets_by_k(triplets_by_k: Dict[Any, Any], k: int) -> List[Dict[str, Any]]:
        if k in triplets_by_k:
            key: Any = k
        elif str(k) in triplets_by_k:
            key = str(k)
        else:
            available = sorted(str(raw_key) for raw_key in triplets_by_k.keys())
            raise ValueError(f"triplets_by_k missing k={k} (available={available})")
        edges = triplets_by_k[key]
        if not isinstance(edges, list):
            raise ValueError(f"triplets_by_k[{k}] must be a list, got {type(edges)}")
        return edges

    def _build_samples(self) -> List[Dict[str, Any]]:
        if not self.eval_retriever_path.exists():
            self._raise_missing_eval_retriever()
        self._validate_manifest(self.eval_retriever_path)
        t0 = time.perf_counter()
        payload = self._torch_load(self.eval_retriever_path)
        t1 = time.perf_counter()
        self.load_s = t1 - t0
        if not isinstance(payload, dict) or "samples" not in payload:
            raise ValueError(f"Unrecognized eval_retriever payload format at {self.eval_retriever_path}")
        raw_samples = payload["samples"]
        if not isinstance(raw_samples, list) or not raw_samples:
            raise ValueError(f"Empty eval_retriever samples in {self.eval_retriever_path}")

        samples: List[Dict[str, Any]] = []
        for record in raw_samples:
            if not isinstance(record, dict):
                raise ValueError("eval_retriever samples must be dicts.")
            sample_id = record["sample_id"]
            if sample_id in (None, ""):
                raise ValueError("sample_id is empty.")
            answers = record["answer_entity_ids"]
            if not answers:
                raise ValueError(f"answer_entity_ids empty for sample_id={sample_id}")
            triplets_by_k = record["triplets_by_k"]
            if not isinstance(triplets_by_k, dict):
                raise ValueError(f"Sample {sample_id} missing triplets_by_k dict.")
            edges = self._select_triplets_by_k(triplets_by_k, self.max_k)
            samples.append({
                "id": str(sample_id),
                "question": str(record["question"]),
                "answer_entity_ids": [int(x) for x in answers],
                "head_entity_ids": list(map(int, map(_HEAD, edges))),
                "tail_entity_ids": list(map(int, map(_TAIL, edges))),
            })
        self.flatten_s = time.perf_counter() - t1
        log.info("Prepared %d samples for %s/%s from %s (max_k=%d).", len(samples), self.dataset, self.split,
                 self.eval_retriever_path, self.max_k)
        return samples

    def _validate_manifest(self, data_path: Path) -> None:
        manifest_path = data_path.with_suffix(".manifest.json")
        if not manifest_path.exists():
            raise FileNotFoundError(f"Missing eval_retriever manifest: {manifest_path}")
        manifest = json.loads(manifest_path.read_text(encoding="utf-8"))
        if "artifact" not in manifest:
            raise ValueError("eval_retriever manifest missing artifact.")
        if manifest["artifact"] != self.artifact_name:
            raise ValueError(f"eval_retriever manifest artifact mismatch: expected '{self.artifact_name}', "
                             f"got '{manifest['artifact']}'.")
        if "schema_version" not in manifest:
            raise ValueError("eval_retriever manifest missing schema_version.")
        if int(manifest["schema_version"]) != self.schema_version:
            raise ValueError(f"eval_retriever manifest schema_version mismatch: expected {self.schema_version}, "
                             f"got {manifest['schema_version']}.")
        if "file" not in manifest:
            raise ValueError("eval_retriever manifest missing file.")
        if manifest["file"] != data_path.name:
            raise ValueError(f"eval_retriever manifest file mismatch: expected '{data_path.name}', "
                             f"got '{manifest['file']}'.")

    def _raise_missing_eval_retriever(self) -> None:
        split = str(self.split)
        base_dir = self.eval_retriever_path.parent
        legacy_candidates = [base_dir / f"{split}_eval_retriever.pt", base_dir / f"{split}_retriever_eval.pt"]
        existing = [str(p) for p in legacy_candidates if p.exists()]
        if existing:
            raise FileNotFoundError(
                "eval_retriever artifact naming mismatch. "
                f"Expected {self.eval_retriever_path} but found legacy file(s): {existing}. "
                "Rename them to '<split>.pt' or re-run eval_retriever.")
        raise FileNotFoundError(f"eval_retriever_path not found: {self.eval_retriever_path}")


# ---- the device pass ---------------------------------------------------------------------------------------------------
def workspace_bytes(total_answers: int) -> int:
    return int(_lib.load().evi_oracle_answer_hits_workspace_bytes(int(total_answers)))


def answer_hits(edge_ptr: torch.Tensor, head_ids: torch.Tensor, tail_ids: torch.Tensor, answer_ptr: torch.Tensor,
                answer_ids: torch.Tensor, ks: Sequence[int], max_scan_k: int, *, uniq: torch.Tensor, found: torch.Tensor,
                workspace: Optional[torch.Tensor] = None, lds_answers: int = MAX_LDS_ANSWERS) -> None:
    """`evi_oracle_answer_hits` on device tensors (int64 inputs, int32 outputs uniq [S] and found [S, len(ks)]), enqueued on
    the current stream: no synchronisation, allocation or copy, so it can be captured into a graph.  `ks`: at most
    EVI_ORACLE_MAX_KS strictly ascending positive values.  `lds_answers` is a test knob (0: every sample sorts its
    answers in the workspace); the results do not depend on it."""
    for name, t in (("edge_ptr", edge_ptr), ("head_ids", head_ids), ("tail_ids", tail_ids), ("answer_ptr", answer_ptr),
                    ("answer_ids", answer_ids)):
        if not t.is_cuda or t.dtype != torch.int64 or not t.is_contiguous():
            raise ValueError(f"{name} must be a contiguous int64 tensor on the GPU (there is no CPU fallback)")
    S = int(edge_ptr.numel()) - 1
    if S < 0 or int(answer_ptr.numel()) != S + 1:
        raise ValueError("edge_ptr and answer_ptr must both hold S + 1 offsets")
    nk = len(ks)
    if uniq.dtype != torch.int32 or found.dtype != torch.int32 or uniq.numel() != S or found.numel() != S * nk:
        raise ValueError("uniq must be int32 [S] and found int32 [S, len(ks)]")
    total = int(answer_ids.numel())  # sizes the workspace: a list longer than answer_ptr[S] is fine
    ws_bytes = workspace_bytes(total)
    if ws_bytes and (workspace is None or workspace.numel() * workspace.element_size() < ws_bytes):
        raise ValueError(f"the workspace must hold {ws_bytes} bytes")
    ks_host = (ctypes.c_int64 * max(nk, 1))(*[int(k) for k in ks])
    stream = torch.cuda.current_stream(edge_ptr.device)
    _lib.check(_lib.load().evi_oracle_answer_hits(
        S, edge_ptr.data_ptr(), head_ids.data_ptr(), tail_ids.data_ptr(), answer_ptr.data_ptr(), answer_ids.data_ptr(), total,
        ks_host, nk, min(int(max_scan_k), _I32_MAX), int(lds_answers), uniq.data_ptr(), found.data_ptr(),
        workspace.data_ptr() if ws_bytes else None, ctypes.c_size_t(ws_bytes), ctypes.c_void_p(stream.cuda_stream)))


def _pow2(n: int) -> int:
    return 1 << max(0, int(n) - 1).bit_length()


def _device() -> torch.device:
    if not torch.cuda.is_available():
        raise RuntimeError("the retriever oracle runs on the GPU (evi_oracle_answer_hits); no device is available")
    return torch.device("cuda", torch.cuda.current_device())


def _cat(lists: List[List[int]]) -> Tuple[np.ndarray, np.ndarray]:
    sizes = np.fromiter((len(x) for x in lists), np.int64, len(lists))
    ptr = np.zeros(len(lists) + 1, np.int64)
    np.cumsum(sizes, out=ptr[1:])
    flat = np.fromiter(itertools.chain.from_iterable(lists), np.int64, int(ptr[-1]))
    return ptr, flat


def oracle_counts(samples: Sequence[Dict[str, Any]], k_values: Sequence[int], *, max_scan_k: Optional[int] = None,
                  chunk_size: int = DEFAULT_CHUNK_SAMPLES, use_lds: bool = True,
                  stats: Optional[Dict[str, Any]] = None) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """(uniq [S], found [S, len(k_values)], num_edges [S]) for samples with `head_entity_ids`, `tail_entity_ids` and
    `answer_entity_ids` lists; `k_values` normalised, scanned up to `max_scan_k` (default: the largest k).  Per chunk of
    `chunk_size` samples: one host -> device copy, one launch per group of EVI_ORACLE_MAX_KS k values, one device -> host
    copy.  The results do not depend on `chunk_size` or `use_lds`."""
    ks = [int(k) for k in k_values]
    if not ks or ks != normalize_k_values(ks):
        raise ValueError(f"k_values must be a non-empty ascending list of distinct positive integers, got {ks}")
    scan = max(ks) if max_scan_k is None else int(max_scan_k)
    S, nk = len(samples), len(ks)
    uniq = np.zeros(S, np.int32)
    found = np.zeros((S, nk), np.int32)
    num_edges = np.zeros(S, np.int64)
    device_ms, launches = 0.0, 0
    if S:
        dev = _device()
        lib_groups = [ks[g:g + _lib.EVI_ORACLE_MAX_KS] for g in range(0, nk, _lib.EVI_ORACLE_MAX_KS)]
        chunk_size = max(1, int(chunk_size))
        for c0 in range(0, S, chunk_size):
            chunk = samples[c0:c0 + chunk_size]
            n = len(chunk)
            heads = [s.get("head_entity_ids", []) for s in chunk]
            tails = [s.get("tail_entity_ids", []) for s in chunk]
            edge_ptr, head = _cat(heads)
            _, tail = _cat(tails)
            if tail.shape[0] != head.shape[0] or any(len(h) != len(t) for h, t in zip(heads, tails)):
                raise ValueError("head_entity_ids and tail_entity_ids differ in length")
            answer_ptr, ans = _cat([s.get("answer_entity_ids", []) for s in chunk])
            counts = np.diff(answer_ptr)
            fits = [_pow2(c) for c in counts.tolist() if 0 < c and _pow2(c) <= MAX_LDS_ANSWERS]
            lds = (max(fits) if fits else 0) if use_lds else 0
            num_edges[c0:c0 + n] = np.diff(edge_ptr)

            # inputs: one host buffer, one copy (an empty id list keeps one unread slot: its view has a real address)
            parts = [edge_ptr, answer_ptr, head, tail, ans]
            offs, total = [], 0
            for a in parts:
                offs.append(total)
                total += max(a.shape[0], 1)
            host = np.zeros(total, np.int64)
            for a, o in zip(parts, offs):
                host[o:o + a.shape[0]] = a
            dbuf = torch.from_numpy(host).to(dev)
            views = [dbuf[o:o + max(a.shape[0], 1)] for a, o in zip(parts, offs)]
            # outputs: one device buffer, one copy back
            obuf = torch.empty(n * (1 + nk), dtype=torch.int32, device=dev)
            ws_bytes = workspace_bytes(int(views[4].numel()))
            ws = torch.empty(max(ws_bytes, 1), dtype=torch.uint8, device=dev)
            stream = torch.cuda.current_stream(dev)
            start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            start.record(stream)
            q0 = n
            for group in lib_groups:
                answer_hits(views[0], views[2], views[3], views[1], views[4], group, scan, uniq=obuf[:n],
                            found=obuf[q0:q0 + n * len(group)], workspace=ws, lds_answers=lds)
                q0 += n * len(group)
                launches += 1
            stop.record(stream)
            out = obuf.cpu().numpy()
            device_ms += start.elapsed_time(stop)
            uniq[c0:c0 + n] = out[:n]
            q0, g0 = n, 0
            for group in lib_groups:
                found[c0:c0 + n, g0:g0 + len(group)] = out[q0:q0 + n * len(group)].reshape(n, len(group))
                q0 += n * len(group)
                g0 += len(group)
    if stats is not None:
        stats.update(device_ms=device_ms, launches=launches)
    return uniq, found, num_edges


# ---- the module --------------------------------------------------------------------------------------------------------
def _oracle_rows_metrics(uniq: np.ndarray, found: np.ndarray, num_edges: np.ndarray,
                         k_values: Sequence[int]) -> List[Dict[str, float]]:
    """Per-sample `oracle` dicts with the reference's key order: interleaved per k, or all hits then all recalls for a
    sample without answers or without edges (_oracle_metrics_for_sample's early returns)."""
    hit_keys = [f"answer_hit@{k}" for k in k_values]
    rec_keys = [f"answer_recall@{k}" for k in k_values]
    empty = dict.fromkeys(hit_keys, 0.0)
    empty.update(dict.fromkeys(rec_keys, 0.0))
    recall = (found.astype(np.float64) / np.maximum(uniq, 1).astype(np.float64)[:, None]).tolist()  # found / uniq, one f64 division
    hits = (found > 0).tolist()
    out: List[Dict[str, float]] = []
    for u, e, h_row, r_row in zip(uniq.tolist(), num_edges.tolist(), hits, recall):
        if u == 0 or e == 0:
            out.append(dict(empty))
            continue
        row: Dict[str, float] = {}
        for hk, rk, h, r in zip(hit_keys, rec_keys, h_row, r_row):
            row[hk] = 1.0 if h else 0.0
            row[rk] = r
        out.append(row)
    return out


class ReasonerModule:
    """reference: ReasonerModule (same constructor kwargs; mode="oracle" only).  `chunk_size` (not in the reference) is
    the number of samples per device launch; the results do not depend on it."""

    def __init__(self, *, mode: str = "llm", model_name: Optional[str] = None, tensor_parallel_size: int = 1,
                 temperature: float = 0.0, frequency_penalty: float = 0.0, max_seq_len: int = 4096, max_tokens: int = 1024,
                 seed: int = 0, output_dir: str, dataset: str, split: str, prompt_tag: str = "triplet", backend: str = "auto",
                 ollama_base_url: str = "http://localhost:11434", ollama_timeout: float = 120.0,
                 k_values: Optional[Sequence[int]] = None, chunk_size: int = DEFAULT_CHUNK_SAMPLES) -> None:
        self.mode = str(mode).strip().lower()
        if self.mode not in {"llm", "oracle"}:
            raise ValueError(f"mode must be 'llm' or 'oracle', got {mode!r}")
        if self.mode == "llm":
            raise NotImplementedError("ReasonerModule(mode='llm'): the LLM reasoner runs (reasoner_triplet, reasoner_paths, "
                                      "reasoner_bfs_paths) are not part of this backend; only mode='oracle' is")
        self.output_dir = Path(output_dir).expanduser().resolve()
        self.dataset = dataset
        self.split = split
        self.prompt_tag = prompt_tag
        self.predict_metrics: Dict[str, Any] = {}
        self.model_name = None
        self.k_values = normalize_k_values(k_values)
        if not self.k_values:
            raise ValueError("k_values must be a non-empty list of positive integers for mode='oracle'.")
        self.chunk_size = int(chunk_size)
        self.stats: Dict[str, Any] = {}

    def oracle_rows(self, samples: Sequence[Dict[str, Any]], *, stats: Optional[Dict[str, Any]] = None) -> List[Dict[str, Any]]:
        """The prediction rows of `predict_step` for every sample, from one batched device pass."""
        uniq, found, num_edges = oracle_counts(samples, self.k_values, chunk_size=self.chunk_size, stats=stats)
        oracles = _oracle_rows_metrics(uniq, found, num_edges, self.k_values)
        return [{"id": s["id"], "question": s["question"], "answer_entity_ids": s["answer_entity_ids"], "oracle": o}
                for s, o in zip(samples, oracles)]

    def predict_step(self, batch: List[Dict[str, Any]], batch_idx: int = 0) -> List[Dict[str, Any]]:
        return self.oracle_rows(batch)

    def run(self, samples: Sequence[Dict[str, Any]]) -> Dict[str, float]:
        """predict_step over every sample and on_predict_epoch_end: the JSONL and metrics files; returns the metrics."""
        stats: Dict[str, Any] = {}
        rows = self.oracle_rows(list(samples), stats=stats)
        t0 = time.perf_counter()
        metrics = self.on_predict_epoch_end([rows])
        stats["write_s"] = time.perf_counter() - t0
        self.stats = stats
        return metrics

    @staticmethod
    def _aggregate_oracle_metrics(rows: List[Dict[str, Any]], k_values: Sequence[int]) -> Dict[str, float]:
        """reference :190-214: sequential f64 sums in row order over max(n, 1)."""
        total = 0
        sums: Dict[str, float] = {f"answer_hit@{k}": 0.0 for k in k_values}
        sums.update({f"answer_recall@{k}": 0.0 for k in k_values})
        for row in rows:
            if "oracle" not in row:
                raise ValueError("oracle metrics missing from prediction row.")
            oracle = row["oracle"]
            if not isinstance(oracle, dict):
                raise ValueError("oracle metrics must be a dict.")
            total += 1
            for k in k_values:
                hit_key = f"answer_hit@{k}"
                rec_key = f"answer_recall@{k}"
                if hit_key not in oracle or rec_key not in oracle:
                    raise ValueError("oracle metrics missing required keys.")
                sums[hit_key] += float(oracle[hit_key])
                sums[rec_key] += float(oracle[rec_key])
        denom = float(max(total, 1))
        metrics: Dict[str, float] = {"oracle/total": float(total)}
        for k in k_values:
            metrics[f"oracle/answer_hit@{k}"] = sums[f"answer_hit@{k}"] / denom
            metrics[f"oracle/answer_recall@{k}"] = sums[f"answer_recall@{k}"] / denom
        return metrics

    def on_predict_epoch_end(self, results: Optional[List[List[Dict[str, Any]]]] = None) -> Dict[str, float]:
        """reference :216-273 (one process): the rows in order to the JSONL, the aggregate to `.metrics.json`."""
        merged: List[Dict[str, Any]] = []
        for batch in results or []:
            if isinstance(batch, list):
                merged.extend(batch)
            elif batch is not None:
                merged.append(batch)
        self.output_dir.mkdir(parents=True, exist_ok=True)
        pred_path = self._prediction_path()
        with pred_path.open("w") as f:
            f.write("".join(json.dumps(row) + "\n" for row in merged))
        metrics = self._aggregate_oracle_metrics(merged, k_values=self.k_values)
        self.predict_metrics = metrics
        metrics_path = pred_path.with_suffix(".metrics.json")
        metrics_path.write_text(json.dumps(metrics, indent=2))
        log.info("Predictions saved to %s", pred_path)
        log.info("Metrics saved to %s", metrics_path)
        return metrics

    def _prediction_path(self) -> Path:
        return self.output_dir / f"{self.dataset}-{self.prompt_tag}-{self.split}.jsonl"


def run_oracle_eval(cfg: Dict[str, Any]) -> Dict[str, float]:
    """One (variant, split) of `experiment=reasoner_oracle` (src/eval.py:311-372 with a ReasonerModule): the datamodule
    and the module from the composed config, no checkpoint, and the module's `predict_metrics`."""
    from . import hydra_lite as hl

    datamodule = hl.instantiate(cfg["data"])
    model = hl.instantiate(cfg["model"])
    datamodule.setup("predict")
    return dict(model.run(datamodule.data))


__all__ = ["ReasonerOracleDataModule", "ReasonerModule", "answer_hits", "oracle_counts", "run_oracle_eval", "workspace_bytes"]
