"""Retriever oracle, host side: the CPU restatement against the reference's recorded run, the datamodule's refusals (all
before any device work), the C-ABI's argument checks, and `experiment=reasoner_oracle` composing on a miniature tree."""
import ctypes
import gzip
import json
import os
import pickle

import pytest
import torch

from tests import answer_hits_oracle as aho
from tests.config_tree import _dump, write_tree

GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "reasoner_oracle.json.gz")


def golden():
    with gzip.open(GOLDEN, "rt", encoding="utf-8") as fh:
        return json.load(fh)


def _datamodule(path, k_values):
    from evi_rag_amd.reasoner_oracle import ReasonerOracleDataModule

    return ReasonerOracleDataModule(dataset="toyqa", split="test", eval_retriever_path=str(path), k_values=k_values)


@pytest.mark.parametrize("case", golden()["cases"], ids=lambda c: c["name"])
def test_restatement_matches_reference_files(case, tmp_path):
    dm = _datamodule(aho.write_case(tmp_path, case), case["data_k_values"])
    dm.setup()
    assert dm.max_k == case["data_max_k"]
    jsonl, metrics = aho.files(dm.data, case["model_ks"])
    assert jsonl == case["jsonl"]
    assert metrics == case["metrics"]
    for s, u, f in zip(dm.data, case["uniq"], case["found"]):
        assert aho.counts(s["head_entity_ids"], s["tail_entity_ids"], s["answer_entity_ids"], case["model_ks"],
                          max(case["model_ks"])) == (u, f)


def test_golden_covers_the_cases():
    g = golden()
    cases = {c["name"]: c for c in g["cases"]}
    samples = [s for c in g["cases"] for s in c["samples"]]
    assert any(len(s["answers"]) != len(set(s["answers"])) for s in samples)  # duplicated answers
    assert any(h == t and h in s["answers"] for s in samples for h, t in zip(s["heads"], s["tails"]))
    assert any(0 < len(s["heads"]) < 500 for s in cases["window"]["samples"])  # fewer edges than max k
    assert any(not s["heads"] for s in samples)
    assert max(len(s["answers"]) for s in samples) > 4096  # past the LDS budget
    assert cases["module_k_past_data_k"]["str_keys"]
    assert any(u and not any(f) for c in g["cases"] for u, f in zip(c["uniq"], c["found"]))  # answers never found
    # the early return lists all hits, then all recalls
    empty = next(json.loads(line) for line in cases["window"]["jsonl"].splitlines() if json.loads(line)["id"] == "s48")
    ks = cases["window"]["model_ks"]
    assert list(empty["oracle"]) == [f"answer_hit@{k}" for k in ks] + [f"answer_recall@{k}" for k in ks]


@pytest.mark.parametrize("refusal", golden()["refusals"], ids=lambda r: r["name"])
def test_datamodule_refusals_match_reference(refusal, tmp_path):
    d = tmp_path / refusal["name"]
    d.mkdir()
    path = aho.REFUSALS[refusal["name"]](d)
    dm = _datamodule(path, aho.REFUSAL_K_VALUES.get(refusal["name"], [1, 5]))
    with pytest.raises(Exception) as info:
        dm.setup()
    assert type(info.value).__name__ == refusal["type"]
    assert str(info.value) == refusal["message"].replace("{dir}", str(d.resolve()))


class _Opaque:
    def __reduce__(self):
        return (dict, ())


def test_cache_that_needs_unpickling_is_refused(tmp_path):
    payload = {"settings": {}, "samples": [{"sample_id": "a", "question": "q", "answer_entity_ids": [1],
                                            "triplets_by_k": {1: []}, "extra": _Opaque()}]}
    path = tmp_path / "test.pt"
    torch.save(payload, path, pickle_module=pickle)
    (tmp_path / "test.manifest.json").write_text(json.dumps({"artifact": "eval_retriever", "schema_version": 1, "file": "test.pt"}))
    with pytest.raises(ValueError, match="weights_only=True"):
        _datamodule(path, [1]).setup()


def test_constructor_refusals(tmp_path):
    from evi_rag_amd.reasoner_oracle import ReasonerModule

    with pytest.raises(ValueError, match="k_values must be a non-empty list"):
        _datamodule(tmp_path / "test.pt", [0, -1, "x"])
    with pytest.raises(ValueError, match="mode must be 'llm' or 'oracle'"):
        ReasonerModule(mode="chat", output_dir=str(tmp_path), dataset="d", split="test", k_values=[1])
    with pytest.raises(NotImplementedError, match="LLM reasoner runs .* are not part of this backend"):
        ReasonerModule(mode="llm", model_name="m", output_dir=str(tmp_path), dataset="d", split="test")
    with pytest.raises(ValueError, match="non-empty list of positive integers for mode='oracle'"):
        ReasonerModule(mode="oracle", output_dir=str(tmp_path), dataset="d", split="test", k_values=None)
    m = ReasonerModule(mode=" Oracle ", output_dir=str(tmp_path), dataset="d", split="test", prompt_tag="oracle", k_values=[5, 1, 5])
    assert m.k_values == [1, 5] and m._prediction_path() == tmp_path.resolve() / "d-oracle-test.jsonl"


def test_abi_argument_refusals():
    from evi_rag_amd import _lib

    lib = _lib.load()
    ks = (ctypes.c_int64 * 3)(1, 5, 10)

    def call(S=1, ks_host=ks, nk=3, max_scan_k=10, lds=64, total=0):
        return lib.evi_oracle_answer_hits(S, None, None, None, None, None, total, ks_host, nk, max_scan_k, lds, None, None, None,
                                          ctypes.c_size_t(0), None)

    for kwargs, text in (({"S": -1}, "num_samples must be >= 0"), ({"ks_host": None}, "null ks_host"), ({"nk": 0}, "nk must be in"),
                         ({"nk": 65}, "nk must be in"), ({"ks_host": (ctypes.c_int64 * 3)(1, 0, 10)}, "ks must be positive"),
                         ({"ks_host": (ctypes.c_int64 * 3)(1, 5, 5)}, "strictly ascending"),
                         ({"ks_host": (ctypes.c_int64 * 3)(10, 5, 1)}, "strictly ascending"),
                         ({"max_scan_k": -1}, "max_scan_k must be >= 0"), ({"lds": 4097}, "lds_answers must be in"),
                         ({"total": -1}, "total_answers must be in"), ({}, "null offset, id or output pointer")):
        rc = call(**kwargs)
        assert rc == _lib.EVI_ERR_INVALID, kwargs
        assert text in _lib.last_error(), (kwargs, _lib.last_error())
    assert call(S=0) == _lib.EVI_OK  # nothing to do, nothing launched
    assert lib.evi_oracle_answer_hits_workspace_bytes(0) == 0
    assert lib.evi_oracle_answer_hits_workspace_bytes(1000) >= 1000 * 2 * 12
    with pytest.raises(ValueError):
        _lib.check(call(nk=0))


def test_oracle_counts_refuse_without_device_or_with_bad_k(monkeypatch):
    from evi_rag_amd import reasoner_oracle as ro

    s = [{"head_entity_ids": [1], "tail_entity_ids": [2], "answer_entity_ids": [2]}]
    with pytest.raises(ValueError, match="ascending list"):
        ro.oracle_counts(s, [5, 1])
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    with pytest.raises(RuntimeError, match="runs on the GPU"):
        ro.oracle_counts(s, [1, 5])


def write_oracle_overlay(cfg_dir):
    """data/reasoner_oracle.yaml, model/reasoner/oracle.yaml, experiment/reasoner_oracle.yaml (and the empty callbacks
    group they select) on top of tests/config_tree.write_tree, in the reference's shape."""
    _dump(cfg_dir / "data" / "reasoner_oracle.yaml", {
        "_target_": "src.data.reasoner_oracle_datamodule.ReasonerOracleDataModule", "dataset": "${dataset.name}",
        "split": "${run.split}", "prompt_tag": "oracle",
        "eval_retriever_path": "${dataset.artifact_dir}/eval_retriever/${data.split}.pt", "artifact_name": "eval_retriever",
        "schema_version": 1, "k_values": "${window.k_values}", "num_workers": 0})
    _dump(cfg_dir / "model" / "reasoner" / "oracle.yaml", {
        "_target_": "src.models.reasoner_module.ReasonerModule", "mode": "oracle", "dataset": "${data.dataset}",
        "split": "${data.split}", "output_dir": "${paths.output_dir}", "k_values": "${data.k_values}",
        "prompt_tag": "${data.prompt_tag}"})
    _dump(cfg_dir / "callbacks" / "none.yaml", {})
    _dump(cfg_dir / "experiment" / "reasoner_oracle.yaml", {
        "defaults": [{"override /data": "reasoner_oracle"}, {"override /model": "reasoner/oracle"}, {"override /callbacks": "none"},
                     {"override /logger": "none"}, {"override /trainer": "predict"}],
        "run": {"name": "reasoner_oracle", "task_name": "reasoner/oracle", "tags": ["eval", "reasoner", "oracle"], "split": "test",
                "ckpt_path": None, "dataset_variants": ["${dataset.dataset_family}", "${dataset.dataset_family}-sub"],
                "require_dual_datasets": True}},
        header="# @package _global_\n#\n# Experiment: retriever-oracle upper bound (no LLM).\n\n")


def test_reasoner_oracle_composes_on_a_miniature_tree(tmp_path, monkeypatch):
    from evi_rag_amd import eval as ev
    from evi_rag_amd import hydra_lite as hl
    from evi_rag_amd.reasoner_oracle import ReasonerModule, ReasonerOracleDataModule

    monkeypatch.setenv("EVI_TEST_PROJECT_ROOT", str(tmp_path / "proj"))
    cfg_dir = write_tree(tmp_path, tmp_path / "data")
    write_oracle_overlay(cfg_dir)
    raw, hydra_node = hl.compose_raw(cfg_dir, "eval", ["experiment=reasoner_oracle", "dataset=toyqa"])
    cfg = hl.resolve_config(raw, hydra_node)
    ev.preflight_validate(cfg)
    assert ev.is_reasoner_run(cfg) and cfg["ckpt_path"] is None
    assert cfg["data"]["eval_retriever_path"] == str(tmp_path / "data" / "toyqa" / "artifacts" / "toyqa" / "eval_retriever" / "test.pt")
    assert cfg["model"]["k_values"] == [1, 5, 20] and cfg["model"]["dataset"] == "toyqa" and cfg["model"]["prompt_tag"] == "oracle"
    assert cfg["run"]["dataset_variants"] == ["toyqa", "toyqa-sub"] and cfg["callbacks"] == {}
    assert cfg["model"]["output_dir"].endswith("reasoner_oracle_toyqa/runs/fixed")
    assert isinstance(hl.instantiate(cfg["data"]), ReasonerOracleDataModule)
    assert isinstance(hl.instantiate(cfg["model"]), ReasonerModule)
    # each dataset variant resolves data.dataset (and so the output file names) to its own name
    variants = ev._variants(raw, hydra_node, cfg_dir)
    assert [label for label, _ in variants] == ["toyqa", "toyqa-sub"]
    raw["dataset"] = variants[1][1]
    sub = hl.resolve_config(raw, hydra_node)
    assert sub["model"]["dataset"] == "toyqa-sub" and ev.dataset_scope(sub["dataset"]) == "sub"
    assert sub["data"]["eval_retriever_path"].endswith("toyqa/artifacts/toyqa-sub/eval_retriever/test.pt")
    # a retriever run is not a reasoner run
    raw_r, hn_r = hl.compose_raw(cfg_dir, "eval", ["experiment=eval_retriever", "dataset=toyqa"])
    assert not ev.is_reasoner_run(hl.resolve_config(raw_r, hn_r))
