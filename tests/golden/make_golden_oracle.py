#!/usr/bin/env python3
"""Generates tests/golden/reasoner_oracle.json.gz by RUNNING THE REFERENCE'S OWN ORACLE RUN (build container only).

For every case: compact samples (ids, question, raw answers, ranked heads and tails; tests/answer_hits_oracle.py expands
them into eval_retriever records), the datamodule's and the module's k lists, and what the reference's
`ReasonerOracleDataModule._build_samples`, `ReasonerModule.predict_step` and `on_predict_epoch_end` write for them: the
JSONL text, the `.metrics.json` text, and per sample the distinct answer count and the distinct answers found at each k
(recall x distinct answers).  For every refusal recipe of tests/answer_hits_oracle.py: the exception type and message
the reference's datamodule raises, with the case directory written as {dir}.

Usage:  EVI_REFERENCE_ROOT=/path/to/EVI-RAG python tests/golden/make_golden_oracle.py
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
from pathlib import Path

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
REF = os.environ.get("EVI_REFERENCE_ROOT", os.path.join(os.path.dirname(REPO), "EVI-RAG"))
sys.path.insert(0, REF)
sys.path.insert(1, REPO)

_STUB_ROOTS = ("lightning", "lightning_utilities", "openai", "vllm", "wandb")


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


sys.meta_path.insert(0, _StubFinder())

from src.data.reasoner_oracle_datamodule import ReasonerOracleDataModule  # noqa: E402
from src.models.reasoner_module import ReasonerModule  # noqa: E402
from tests import answer_hits_oracle as aho  # noqa: E402

WINDOW = [1, 10, 25, 50, 100, 200, 300, 400, 500]


def sample(rng, sid, *, n_answers, n_edges, ent_range=60, dup=0, absent=0, head_is_tail_answer=False):
    answers = rng.integers(0, ent_range, n_answers).tolist()
    answers += [answers[i % len(answers)] for i in range(dup)] if answers else []
    answers += [10**9 + i for i in range(absent)]  # never found
    rng.shuffle(answers)
    heads = rng.integers(0, ent_range, n_edges).tolist()
    tails = rng.integers(0, ent_range, n_edges).tolist()
    if head_is_tail_answer and n_edges and answers:
        p = int(rng.integers(0, n_edges))
        heads[p] = tails[p] = int(answers[0])
    return {"id": f"s{sid}", "question": f"question {sid}: what é \"x\"?", "answers": [int(a) for a in answers],
            "heads": heads, "tails": tails}


def cases():
    rng = np.random.default_rng(2026)
    out = []
    basic = []
    for i in range(48):
        n_edges = int(rng.choice([1, 5, 9, 30, 99, 250, 500, 600]))
        basic.append(sample(rng, i, n_answers=int(rng.integers(1, 9)), n_edges=n_edges, ent_range=int(rng.choice([20, 200, 2000])),
                            dup=int(rng.integers(0, 3)), absent=int(rng.integers(0, 2)), head_is_tail_answer=bool(i % 5 == 0)))
    basic.append(sample(rng, 48, n_answers=3, n_edges=0))  # empty triplet list: hits-then-recalls key order
    basic.append({"id": "s49", "question": "only the head-and-tail edge", "answers": [7, 7, 8], "heads": [7], "tails": [7]})
    basic.append({"id": "s50", "question": "never found", "answers": [5, 6], "heads": [1, 2, 3], "tails": [4, 4, 4]})
    out.append({"name": "window", "data_k_values": WINDOW, "model_k_values": WINDOW, "cache_ks": WINDOW, "str_keys": False,
                "samples": basic})
    few = [sample(rng, 100 + i, n_answers=int(rng.integers(1, 5)), n_edges=int(rng.integers(0, 40)), ent_range=30, dup=1)
           for i in range(12)]
    out.append({"name": "k_lists_unsorted", "data_k_values": [25, 10, "3", 0, -4, 10, 1], "model_k_values": [7, 2, 2, 0, 25, -1],
                "cache_ks": [1, 3, 10, 25], "str_keys": False, "samples": few})
    out.append({"name": "module_k_past_data_k", "data_k_values": [10, 3], "model_k_values": [1, 5, 10, 40, 1000],
                "cache_ks": [3, 10, 50], "str_keys": True, "samples": few})
    out.append({"name": "module_k_below_data_k", "data_k_values": [50], "model_k_values": [2, 4], "cache_ks": [50],
                "str_keys": True, "samples": few})
    hub = sample(rng, 200, n_answers=4000, n_edges=500, ent_range=6000, dup=700, absent=3)
    small = sample(rng, 201, n_answers=2, n_edges=500, ent_range=50)
    out.append({"name": "several_thousand_answers", "data_k_values": WINDOW, "model_k_values": WINDOW, "cache_ks": [100, 500],
                "str_keys": False, "samples": [small, hub, small | {"id": "s202"}]})
    return out


def run_case(case, tmp: Path):
    d = tmp / case["name"]
    path = aho.write_case(d, case)
    dm = ReasonerOracleDataModule(dataset="toyqa", split="test", eval_retriever_path=str(path), k_values=case["data_k_values"])
    dm.setup()
    module = ReasonerModule(mode="oracle", output_dir=str(d / "out"), dataset="toyqa", split="test", prompt_tag="oracle",
                            k_values=case["model_k_values"])
    module.trainer = None
    results = [module.predict_step(batch, i) for i, batch in enumerate(dm.predict_dataloader())]
    module.on_predict_epoch_end(results)
    pred = d / "out" / "toyqa-oracle-test.jsonl"
    jsonl = pred.read_text()
    metrics = pred.with_suffix(".metrics.json").read_text()
    uniq, found = [], []
    for s, row in zip(dm.data, (r for b in results for r in b)):
        u = len(set(s["answer_entity_ids"]))
        uniq.append(u)
        found.append([int(round(row["oracle"][f"answer_recall@{k}"] * u)) for k in module.k_values])
    return dict(case, jsonl=jsonl, metrics=metrics, uniq=uniq, found=found, model_ks=list(module.k_values), data_max_k=dm.max_k)


def refusals(tmp: Path):
    out = []
    for name, recipe in aho.REFUSALS.items():
        d = tmp / "refusal" / name
        d.mkdir(parents=True, exist_ok=True)
        path = recipe(d)
        ks = aho.REFUSAL_K_VALUES.get(name, [1, 5])
        try:
            dm = ReasonerOracleDataModule(dataset="toyqa", split="test", eval_retriever_path=str(path), k_values=ks)
            dm.setup()
        except Exception as exc:  # noqa: BLE001 - recorded
            out.append({"name": name, "type": type(exc).__name__, "message": str(exc).replace(str(d.resolve()), "{dir}")})
            continue
        raise SystemExit(f"refusal {name}: the reference accepted it")
    return out


def main():
    with tempfile.TemporaryDirectory() as t:
        tmp = Path(t)
        payload = {"cases": [run_case(c, tmp) for c in cases()], "refusals": refusals(tmp)}
    out = os.path.join(HERE, "reasoner_oracle.json.gz")
    with gzip.open(out, "wt", encoding="utf-8", compresslevel=9) as fh:
        json.dump(payload, fh, separators=(",", ":"))
    print(out, os.path.getsize(out), "bytes;", len(payload["cases"]), "cases,", len(payload["refusals"]), "refusals")


if __name__ == "__main__":
    main()
