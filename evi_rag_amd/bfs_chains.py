"""BFS candidate reasoning chains from a g_agent cache (reference: src/data/components/bfs_chain_builder.py:49-311).

For every sample, the reference enumerates the chains that start at a seed node and follow its oriented, score-ranked
adjacency breadth first, de-duplicates them by their (head entity, relation, tail entity) signature and ranks the
signatures by (frequency, length, best score).  It does so in Python, one sample at a time.  Here a chunk of samples is
packed into flat arrays once, `evi_bfs_chains` (csrc/chains.hip) runs all three stages with one workgroup per sample,
and one device -> host copy per chunk returns the ranked chains as flat arrays; the JSON records are built from whole-array
`tolist()` results.  The output equals the reference's, byte for byte once serialised.

Refusals the reference does not make: a non-finite edge score (Python's sort order is undefined for NaN), a
max_chain_length above EVI_BFS_CHAIN_MAX_LENGTH, and a sample that needs more than MAX_RECORDS_PER_SAMPLE chain records
(only possible with max_total_chains <= 0 or min_chain_length > 1).
"""
from __future__ import annotations

import ctypes
import json
import logging
import time
from dataclasses import dataclass
from datetime import datetime, timezone
from pathlib import Path
from typing import Any, Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib
from .g_agent import GAgentSample, load_g_agent_samples

log = logging.getLogger(__name__)

DIRECTION_FORWARD = 0
DIRECTION_BACKWARD = 1
MAX_RECORDS_PER_SAMPLE = 1 << 22
DEFAULT_CHUNK_SAMPLES = 1024
_FIRST_ROOM = 4096  # record room a sample starts with when its chain count is not bounded by max_total_chains
_BOUNDED_ROOM = 65536  # ... and the most it starts with when it is (max(max_total_chains, seeds) records always suffice)
_LDS_RECORDS = 8140  # csrc/chains.hip kMaxLdsRecords
_LDS_SORT_SLOTS = 32768
_I32_MAX = 2**31 - 1


@dataclass
class BFSChainSettings:
    """reference: BFSChainSettings, bfs_chain_builder.py:37-46 (same fields, same defaults)."""

    max_chain_length: int
    min_chain_length: int = 1
    max_chains_per_sample: int = 100
    max_total_chains: int = 5000
    allow_backward: bool = True
    max_branch_per_node: Optional[int] = None
    forbid_edge_revisit: bool = True
    forbid_node_revisit: bool = False


def _clamp_i32(v: int) -> int:
    return max(-_I32_MAX - 1, min(_I32_MAX, int(v)))


def _pow2(n: int) -> int:
    return 1 << max(0, int(n) - 1).bit_length()


@dataclass
class _Packed:
    """One chunk's inputs on the host (numpy) — what is copied to the device in one go."""

    node_ptr: np.ndarray
    edge_ptr: np.ndarray
    seed_ptr: np.ndarray
    head: np.ndarray
    tail: np.ndarray
    score: np.ndarray
    rel: np.ndarray
    ent: np.ndarray
    seeds: np.ndarray


def _pack(samples: Sequence[GAgentSample]) -> _Packed:
    def cat(arrays, dtype):
        return np.concatenate(arrays).astype(dtype, copy=False) if arrays else np.zeros(0, dtype)

    def ptr(sizes):
        out = np.zeros(len(sizes) + 1, np.int64)
        np.cumsum(sizes, out=out[1:])
        return out

    ents = [s.node_entity_ids.reshape(-1).numpy() for s in samples]
    heads = [s.edge_head_locals.reshape(-1).numpy() for s in samples]
    tails = [s.edge_tail_locals.reshape(-1).numpy() for s in samples]
    seeds = []
    for s, e in zip(samples, ents):
        q = s.start_node_locals.reshape(-1).numpy().astype(np.int64)
        seeds.append(np.where((q >= 0) & (q < e.shape[0]), q, -1).astype(np.int32))  # out of range: skipped
    return _Packed(node_ptr=ptr([e.shape[0] for e in ents]), edge_ptr=ptr([h.shape[0] for h in heads]),
                   seed_ptr=ptr([q.shape[0] for q in seeds]), head=cat(heads, np.int32), tail=cat(tails, np.int32),
                   score=cat([s.edge_scores.reshape(-1).numpy() for s in samples], np.float32),
                   rel=cat([s.edge_relations.reshape(-1).numpy() for s in samples], np.int64), ent=cat(ents, np.int64),
                   seeds=cat(seeds, np.int32))


def _validate(sample: GAgentSample, max_len: int) -> None:
    if max_len <= 0:
        raise ValueError("max_chain_length must be a positive integer.")
    if max_len > _lib.EVI_BFS_CHAIN_MAX_LENGTH:
        raise ValueError(f"max_chain_length {max_len} exceeds the bound of {_lib.EVI_BFS_CHAIN_MAX_LENGTH} hops of the device "
                         "chain builder")
    n = int(sample.node_entity_ids.numel())
    e = int(sample.edge_head_locals.numel())
    if int(sample.edge_tail_locals.numel()) != e or int(sample.edge_relations.numel()) != e or int(sample.edge_scores.numel()) != e:
        raise ValueError(f"sample {sample.sample_id!r}: edge arrays differ in length")
    if e:
        if not bool(torch.isfinite(sample.edge_scores).all()):
            raise ValueError(f"sample {sample.sample_id!r}: non-finite edge score (the reference's ranking is undefined for NaN)")
        for name, t in (("edge_head_locals", sample.edge_head_locals), ("edge_tail_locals", sample.edge_tail_locals)):
            if bool((t < 0).any()) or bool((t >= n).any()):
                raise ValueError(f"sample {sample.sample_id!r}: {name} out of range")


class _ChainRun:
    """The settings of one batched call, mapped to the C-ABI's integers."""

    def __init__(self, settings: BFSChainSettings, *, hash_bits: int = 64, use_lds: bool = True):
        self.max_len = int(settings.max_chain_length)
        self.min_len = _clamp_i32(settings.min_chain_length)
        self.cap = _clamp_i32(settings.max_total_chains)
        mb = settings.max_branch_per_node
        self.max_branch = -1 if mb is None else _clamp_i32(mb)
        self.allow_backward = bool(settings.allow_backward)
        self.forbid_edge = bool(settings.forbid_edge_revisit)
        self.forbid_node = bool(settings.forbid_node_revisit)
        lim = settings.max_chains_per_sample
        self.limit = None if lim is None else max(int(lim), 0)
        self.hash_bits = int(hash_bits)
        self.use_lds = bool(use_lds)
        self.bounded = self.cap > 0 and self.min_len <= 1  # every level fits in max(cap, seeds) records
        self.device_ms = 0.0
        self.launches = 0

    def first_room(self, seeds: int) -> int:
        """Record room a sample starts with; a sample that needs more is sized again from what the device reports."""
        if self.bounded:
            return max(min(self.cap, _BOUNDED_ROOM), seeds, 1)
        return max(min(self.cap, _BOUNDED_ROOM) if self.cap > 0 else 0, seeds, _FIRST_ROOM)

    def launch(self, samples: Sequence[GAgentSample], rooms: Sequence[int], dev: torch.device) -> Dict[str, np.ndarray]:
        """One chunk: pack, copy in, three kernels, one copy out."""
        lib = _lib.load()
        pk = _pack(samples)
        S = len(samples)
        rec_ptr = np.zeros(S + 1, np.int64)
        np.cumsum(rooms, out=rec_ptr[1:])
        slots = [_pow2(r) for r in rooms]
        sort_ptr = np.zeros(S + 1, np.int64)
        np.cumsum(slots, out=sort_ptr[1:])
        max_room = max(rooms) if rooms else 1
        M = max_room if self.limit is None else min(self.limit, max_room)
        TN, TE, R, P = int(pk.node_ptr[-1]), int(pk.edge_ptr[-1]), int(rec_ptr[-1]), int(sort_ptr[-1])
        lds_records = min(max_room, _LDS_RECORDS) if self.use_lds else 0
        lds_slots = min(max(slots), _LDS_SORT_SLOTS) if self.use_lds else 0

        # inputs: one host buffer, one copy
        parts = [pk.node_ptr, pk.edge_ptr, pk.seed_ptr, rec_ptr, sort_ptr, pk.rel, pk.ent, pk.score, pk.head, pk.tail, pk.seeds]
        offs, total = [], 0
        for a in parts:
            offs.append(total)
            total += (a.nbytes + 15) // 16 * 16
        host = np.zeros(max(total, 16), np.uint8)
        for a, o in zip(parts, offs):
            host[o:o + a.nbytes] = a.view(np.uint8)
        dbuf = torch.from_numpy(host).to(dev)
        base = dbuf.data_ptr()
        ptrs = [base + o for o in offs]

        # outputs: one device buffer, one copy back
        out_parts = [("stats", np.int64, 4 * S), ("score", np.float64, S * M), ("count", np.int32, S), ("len", np.int32, S * M),
                     ("freq", np.int32, S * M), ("steps", np.int32, S * M * self.max_len)]
        oofs, ototal = {}, 0
        for name, dt, n in out_parts:
            oofs[name] = ototal
            ototal += (n * np.dtype(dt).itemsize + 15) // 16 * 16
        obuf = torch.empty(max(ototal, 16), dtype=torch.uint8, device=dev)
        ob = obuf.data_ptr()
        ws_bytes = int(lib.evi_bfs_chains_workspace_bytes(TN, TE, R, P))
        ws = torch.empty(max(ws_bytes, 16), dtype=torch.uint8, device=dev)
        stream = torch.cuda.current_stream(dev)
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record(stream)
        _lib.check(lib.evi_bfs_chains(
            S, ptrs[0], ptrs[1], ptrs[2], ptrs[3], ptrs[4], TN, TE, R, P, ptrs[8], ptrs[9], ptrs[7], ptrs[5], ptrs[6], ptrs[10],
            self.max_len, self.min_len, self.cap, int(self.allow_backward), self.max_branch, int(self.forbid_edge),
            int(self.forbid_node), M, lds_records, lds_slots, self.hash_bits, ob + oofs["count"], ob + oofs["len"],
            ob + oofs["freq"], ob + oofs["score"], ob + oofs["steps"], ob + oofs["stats"], ws.data_ptr(), ctypes.c_size_t(ws_bytes),
            ctypes.c_void_p(stream.cuda_stream)))
        stop.record(stream)
        out_host = obuf.cpu().numpy()
        self.device_ms += start.elapsed_time(stop)
        self.launches += 1
        res = {}
        for name, dt, n in out_parts:
            res[name] = out_host[oofs[name]:oofs[name] + n * np.dtype(dt).itemsize].view(dt)
        res["stats"] = res["stats"].reshape(S, 4)
        res["M"] = M
        res["pack"] = pk
        return res


def _gather(res: Dict[str, Any], S: int, max_len: int):
    """Flat device results -> whole-array gathers, as Python lists: the nine step columns of every emitted chain (in
    rank order, steps in path order) and each candidate's length, frequency and score."""
    pk: _Packed = res["pack"]
    M = int(res["M"])
    count = res["count"].astype(np.int64)
    lens = res["len"].reshape(S, M)
    valid_c = np.arange(M)[None, :] < count[:, None]
    steps = res["steps"].reshape(S, M, max_len)
    valid_s = valid_c[:, :, None] & (np.arange(max_len)[None, None, :] < lens[:, :, None])
    sample_of = np.broadcast_to(np.arange(S)[:, None, None], steps.shape)[valid_s]
    x = steps[valid_s].astype(np.int64)
    eid, direction = x >> 1, x & 1
    g_edge = pk.edge_ptr[sample_of] + eid
    n0 = pk.node_ptr[sample_of]
    h_loc, t_loc = pk.head[g_edge].astype(np.int64), pk.tail[g_edge].astype(np.int64)
    s_loc = np.where(direction == 1, t_loc, h_loc)
    d_loc = np.where(direction == 1, h_loc, t_loc)
    cols = [eid, pk.ent[n0 + h_loc], pk.ent[n0 + t_loc], pk.rel[g_edge], pk.ent[n0 + s_loc], pk.ent[n0 + d_loc], s_loc, d_loc,
            direction]
    return ([c.tolist() for c in cols], lens[valid_c].tolist(), res["freq"].reshape(S, M)[valid_c].tolist(),
            res["score"].reshape(S, M)[valid_c].tolist(), count.tolist())


def _empty(res: Dict[str, Any], S: int) -> bool:
    return S == 0 or int(res["M"]) == 0 or int(res["count"].sum()) == 0


def _format(samples: Sequence[GAgentSample], res: Dict[str, Any], max_len: int) -> List[List[Dict[str, Any]]]:
    """Flat device results -> the reference's candidate dicts (key order included)."""
    S = len(samples)
    if _empty(res, S):
        return [[] for _ in range(S)]
    (eid_l, he_l, te_l, rel_l, se_l, de_l, sl_l, dl_l, dir_l), len_l, freq_l, score_l, count = _gather(res, S, max_len)
    out: List[List[Dict[str, Any]]] = []
    c = t = 0
    for s in range(S):
        cands = []
        for rank in range(1, count[s] + 1):
            L = len_l[c]
            sl = slice(t, t + L)
            cands.append({
                "signature": [[a, b, d] for a, b, d in zip(se_l[sl], rel_l[sl], de_l[sl])],
                "length": L,
                "frequency": freq_l[c],
                "score": score_l[c],
                "edge_local_ids": eid_l[sl],
                "chain_edges": [{"edge_id": k[0], "head_entity_id": k[1], "tail_entity_id": k[2], "relation_id": k[3],
                                 "src_entity_id": k[4], "dst_entity_id": k[5], "src_node_local": k[6], "dst_node_local": k[7],
                                 "direction": k[8]}
                                for k in zip(eid_l[sl], he_l[sl], te_l[sl], rel_l[sl], se_l[sl], de_l[sl], sl_l[sl], dl_l[sl],
                                             dir_l[sl])],
                "rank": rank,
            })
            c += 1
            t += L
        out.append(cands)
    return out


_STEP = ('{"edge_id": %d, "head_entity_id": %d, "tail_entity_id": %d, "relation_id": %d, "src_entity_id": %d, '
         '"dst_entity_id": %d, "src_node_local": %d, "dst_node_local": %d, "direction": %d}')


def _format_text(samples: Sequence[GAgentSample], res: Dict[str, Any], max_len: int) -> List[str]:
    """The same candidates as `_format`, directly as the text `json.dumps` gives their list (default separators; ints
    print as %d, finite floats as repr): the export writes this without building the dicts."""
    S = len(samples)
    if _empty(res, S):
        return ["[]"] * S
    cols, len_l, freq_l, score_l, count = _gather(res, S, max_len)
    eid_l, _, _, rel_l, se_l, de_l = cols[:6]
    steps = [_STEP % k for k in zip(*cols)]
    sigs = ["[%d, %d, %d]" % k for k in zip(se_l, rel_l, de_l)]
    out: List[str] = []
    c = t = 0
    for s in range(S):
        cands = []
        for rank in range(1, count[s] + 1):
            L = len_l[c]
            e = t + L
            cands.append('{"signature": [%s], "length": %d, "frequency": %d, "score": %s, "edge_local_ids": [%s], '
                         '"chain_edges": [%s], "rank": %d}' % (", ".join(sigs[t:e]), L, freq_l[c], float.__repr__(score_l[c]),
                                                                ", ".join(map(str, eid_l[t:e])), ", ".join(steps[t:e]), rank))
            c += 1
            t = e
        out.append("[" + ", ".join(cands) + "]")
    return out


def _device() -> torch.device:
    if not torch.cuda.is_available():
        raise RuntimeError("the BFS chain builder runs on the GPU (evi_bfs_chains); no device is available")
    return torch.device("cuda", torch.cuda.current_device())


def _build_batch(samples: Sequence[GAgentSample], settings: BFSChainSettings, *, chunk_size: int, hash_bits: int, use_lds: bool,
                 stats: Optional[Dict[str, Any]], as_text: bool = False) -> List[Any]:
    samples = list(samples)
    formatter = _format_text if as_text else _format
    results: List[Any] = [("[]" if as_text else []) for _ in samples]
    work = [i for i, s in enumerate(samples) if int(s.start_node_locals.numel()) > 0]  # no seeds: [] (reference :50-52)
    max_len = int(settings.max_chain_length)
    for i in work:
        _validate(samples[i], max_len)
    run = _ChainRun(settings, hash_bits=hash_bits, use_lds=use_lds)
    level_hist: Dict[int, int] = {}
    raw_total = capped = 0
    format_s = 0.0
    if work and run.min_len <= max_len:  # otherwise no chain is long enough: every list is empty
        dev = _device()
        chunk_size = max(1, int(chunk_size))
        for c0 in range(0, len(work), chunk_size):
            idx = work[c0:c0 + chunk_size]
            rooms = {i: run.first_room(int(samples[i].start_node_locals.numel())) for i in idx}
            while idx:
                chunk = [samples[i] for i in idx]
                res = run.launch(chunk, [rooms[i] for i in idx], dev)
                t0 = time.perf_counter()
                formatted = formatter(chunk, res, max_len)
                format_s += time.perf_counter() - t0
                again = []
                for j, i in enumerate(idx):
                    need = int(res["stats"][j, 0])
                    if need:
                        if need > MAX_RECORDS_PER_SAMPLE:
                            raise ValueError(f"sample {samples[i].sample_id!r} needs at least {need} chain records, more than the "
                                             f"bound of {MAX_RECORDS_PER_SAMPLE}; lower max_chain_length or set max_total_chains > 0")
                        rooms[i] = min(max(need, 2 * rooms[i]), MAX_RECORDS_PER_SAMPLE)
                        again.append(i)
                        continue
                    results[i] = formatted[j]
                    levels, raw = int(res["stats"][j, 1]), int(res["stats"][j, 2])
                    level_hist[levels] = level_hist.get(levels, 0) + 1
                    raw_total += raw
                    capped += int(run.cap > 0 and raw >= run.cap)
                idx = again
    if stats is not None:
        stats.update(device_ms=run.device_ms, launches=run.launches, format_s=format_s, levels_reached=dict(sorted(level_hist.items())),
                     samples_at_cap=capped, raw_chains=raw_total)
    return results


def build_bfs_candidate_chains_batch(samples: Sequence[GAgentSample], *, settings: BFSChainSettings,
                                     chunk_size: int = DEFAULT_CHUNK_SAMPLES, hash_bits: int = 64, use_lds: bool = True,
                                     stats: Optional[Dict[str, Any]] = None) -> List[List[Dict[str, Any]]]:
    """build_bfs_candidate_chains for every sample: one launch and one read-back per chunk of `chunk_size` samples.
    `hash_bits` and `use_lds` are test knobs (a narrowed signature hash; global memory only): the results never depend on
    them, nor on `chunk_size`.  `stats`, if given, receives device milliseconds, host formatting seconds and chain counts."""
    return _build_batch(samples, settings, chunk_size=chunk_size, hash_bits=hash_bits, use_lds=use_lds, stats=stats)


def build_bfs_candidate_chains(sample: GAgentSample, *, settings: BFSChainSettings) -> List[Dict[str, Any]]:
    """reference: build_bfs_candidate_chains, bfs_chain_builder.py:49-91."""
    return _build_batch([sample], settings, chunk_size=1, hash_bits=64, use_lds=True, stats=None)[0]


def export_bfs_chain_cache(*, g_agent_path, output_dir, split: str, settings: BFSChainSettings, artifact_name: str = "eval_bfs",
                           schema_version: int = 1, overwrite: bool = True, drop_unreachable: bool = False,
                           chunk_size: int = DEFAULT_CHUNK_SAMPLES, stats: Optional[Dict[str, Any]] = None) -> Tuple[Path, int]:
    """reference: export_bfs_chain_cache, bfs_chain_builder.py:94-146: `<output_dir>/<split>.jsonl` (one record per sample,
    appended to when overwrite=False) and `<split>.manifest.json`; returns (jsonl path, samples written)."""
    t_start = time.perf_counter()
    g_agent_path = Path(g_agent_path).expanduser().resolve()
    if not g_agent_path.exists():
        raise FileNotFoundError(f"g_agent_path not found: {g_agent_path}")
    output_dir = Path(output_dir).expanduser().resolve()
    output_dir.mkdir(parents=True, exist_ok=True)
    output_path = output_dir / f"{split}.jsonl"
    manifest_path = output_dir / f"{split}.manifest.json"
    if overwrite:
        output_path.write_text("", encoding="utf-8")
    t_load = time.perf_counter()
    samples = load_g_agent_samples(g_agent_path, drop_unreachable=drop_unreachable)
    run_stats: Dict[str, Any] = {"load_s": time.perf_counter() - t_load}
    chains = _build_batch(samples, settings, chunk_size=chunk_size, hash_bits=64, use_lds=True, stats=run_stats, as_text=True)
    t0 = time.perf_counter()
    with output_path.open("a", encoding="utf-8") as f:  # json.dumps of {"sample_id", "question", "candidate_chains"}
        f.write("".join('{"sample_id": %s, "question": %s, "candidate_chains": %s}\n'
                        % (json.dumps(str(s.sample_id)), json.dumps(str(s.question)), c) for s, c in zip(samples, chains)))
    run_stats["format_s"] = run_stats.get("format_s", 0.0) + time.perf_counter() - t0
    manifest = {
        "artifact": str(artifact_name).strip(),
        "schema_version": int(schema_version),
        "file": output_path.name,
        "created_at": datetime.now(timezone.utc).replace(tzinfo=None).isoformat(timespec="seconds") + "Z",
        "producer": "bfs_chain_builder",
        "settings": {
            "max_chain_length": int(settings.max_chain_length),
            "min_chain_length": int(settings.min_chain_length),
            "max_chains_per_sample": int(settings.max_chains_per_sample),
            "max_total_chains": int(settings.max_total_chains),
            "allow_backward": bool(settings.allow_backward),
            "max_branch_per_node": settings.max_branch_per_node,
            "forbid_edge_revisit": bool(settings.forbid_edge_revisit),
            "forbid_node_revisit": bool(settings.forbid_node_revisit),
        },
    }
    manifest_path.write_text(json.dumps(manifest, indent=2), encoding="utf-8")
    run_stats["total_s"] = time.perf_counter() - t_start
    if stats is not None:
        stats.update(run_stats)
    return output_path, len(samples)


def settings_from_config(bfs_cfg: Dict[str, Any]) -> Tuple[BFSChainSettings, int]:
    """The `bfs_chain_eval` block -> (settings, schema_version), with the reference's checks (src/eval.py:200-223)."""
    schema_version = int(bfs_cfg.get("schema_version", 1))
    if schema_version <= 0:
        raise ValueError("bfs_chain_eval.schema_version must be a positive integer.")
    max_chain_length = int(bfs_cfg.get("max_chain_length", 0))
    if max_chain_length <= 0:
        raise ValueError("bfs_chain_eval.max_chain_length must be a positive integer.")
    settings = BFSChainSettings(
        max_chain_length=max_chain_length,
        min_chain_length=int(bfs_cfg.get("min_chain_length", 1)),
        max_chains_per_sample=int(bfs_cfg.get("max_chains_per_sample", 100)),
        max_total_chains=int(bfs_cfg.get("max_total_chains", 5000)),
        allow_backward=bool(bfs_cfg.get("allow_backward", True)),
        max_branch_per_node=bfs_cfg.get("max_branch_per_node"),
        forbid_edge_revisit=bool(bfs_cfg.get("forbid_edge_revisit", True)),
        forbid_node_revisit=bool(bfs_cfg.get("forbid_node_revisit", False)),
    )
    return settings, schema_version


def maybe_build_bfs_chains(cfg: Dict[str, Any]) -> Dict[str, float]:
    """reference: _maybe_build_bfs_chains, src/eval.py:186-229.  {} when the block is absent or disabled."""
    bfs_cfg = cfg.get("bfs_chain_eval") or {}
    if not bool(bfs_cfg.get("enabled", False)):
        return {}
    dataset_cfg = cfg.get("dataset") or {}
    run_cfg = cfg.get("run") or {}
    split = str(run_cfg.get("split", "test"))
    artifact_root = Path(dataset_cfg.get("artifact_dir") or dataset_cfg.get("materialized_dir") or ".")
    g_agent_path = bfs_cfg.get("g_agent_path") or str(artifact_root / "g_agent" / f"{split}_g_agent.pt")
    output_dir = bfs_cfg.get("output_dir") or str(artifact_root / "eval_bfs")
    artifact_name = str(bfs_cfg.get("artifact_name", "eval_bfs")).strip()
    settings, schema_version = settings_from_config(bfs_cfg)
    output_path, total = export_bfs_chain_cache(
        g_agent_path=str(g_agent_path), output_dir=str(output_dir), split=split, settings=settings, artifact_name=artifact_name,
        schema_version=schema_version, overwrite=bool(bfs_cfg.get("overwrite", True)),
        drop_unreachable=bool(bfs_cfg.get("drop_unreachable", False)))
    log.info("BFS chains saved to %s (samples=%d).", output_path, total)
    return {"bfs_chain/total": float(total)}


__all__ = ["BFSChainSettings", "build_bfs_candidate_chains", "build_bfs_candidate_chains_batch", "export_bfs_chain_cache",
           "maybe_build_bfs_chains", "MAX_RECORDS_PER_SAMPLE"]
