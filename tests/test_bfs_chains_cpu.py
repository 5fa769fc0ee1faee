"""BFS candidate chains, host side: the CPU restatement against the reference's recorded output, the cache loader's and
the eval hook's refusals (all before any device work), and the C-ABI's argument checks."""
import ctypes
import gzip
import json
import os

import pytest
import torch

from tests import bfs_chain_oracle as oracle

GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "bfs_chains.json.gz")


def golden_cases():
    with gzip.open(GOLDEN, "rt", encoding="utf-8") as fh:
        return json.load(fh)["cases"]


def kept_records(case):
    return [r for r in case["records"] if not case["drop_unreachable"] or r["is_answer_reachable"]]


@pytest.mark.parametrize("case", golden_cases(), ids=lambda c: c["name"])
def test_restatement_matches_reference_lines(case):
    got = oracle.jsonl_lines(kept_records(case), case["settings"])
    assert len(got) == len(case["lines"])
    for i, (a, b) in enumerate(zip(got, case["lines"])):
        assert a == b, f"{case['name']} line {i}"


def test_golden_covers_the_settings_grid():
    cases = golden_cases()
    seen = {k: {json.dumps(c["settings"][k]) for c in cases} for k in cases[0]["settings"]}
    assert {"true", "false"} <= seen["allow_backward"] and {"true", "false"} <= seen["forbid_edge_revisit"]
    assert {"true", "false"} <= seen["forbid_node_revisit"]
    assert {"null", "0", "2", "-1"} <= seen["max_branch_per_node"]
    assert {"0", "2"} <= seen["min_chain_length"] and {"0", "1", "5000"} <= seen["max_total_chains"]
    assert {"0", "-1"} <= seen["max_chains_per_sample"]
    assert any(c["drop_unreachable"] for c in cases)
    # the manifest the reference wrote: its keys, in order
    m = next(c for c in cases if c["mode"] == "export")["manifest"]
    assert list(m) == ["artifact", "schema_version", "file", "created_at", "producer", "settings"]


class _Opaque:
    pass


def _record(**over):
    rec = {"sample_id": "a", "question": "q?", "question_emb": torch.zeros(2), "edge_relations": torch.tensor([0, 1]),
           "edge_scores": torch.tensor([0.5, 0.25]), "edge_labels": torch.zeros(2), "edge_head_locals": torch.tensor([0, 1]),
           "edge_tail_locals": torch.tensor([1, 2]), "node_entity_ids": torch.tensor([10, 11, 12]),
           "node_embedding_ids": torch.tensor([0, 1, 2]), "start_entity_ids": torch.tensor([10]),
           "start_node_locals": torch.tensor([0]), "answer_entity_ids": torch.tensor([12]), "answer_node_locals": torch.tensor([2]),
           "pair_start_node_locals": torch.zeros(0, dtype=torch.long), "pair_answer_node_locals": torch.zeros(0, dtype=torch.long),
           "pair_edge_local_ids": torch.zeros(0, dtype=torch.long), "pair_edge_counts": torch.zeros(0, dtype=torch.long),
           "pair_shortest_lengths": torch.zeros(0, dtype=torch.long), "gt_path_edge_local_ids": torch.zeros(0, dtype=torch.long),
           "gt_path_exists": False, "is_answer_reachable": True}
    rec.update(over)
    return rec


def test_loader_refusals(tmp_path):
    from evi_rag_amd.g_agent import load_g_agent_samples

    with pytest.raises(FileNotFoundError, match="g_agent cache not found"):
        load_g_agent_samples(tmp_path / "missing.pt")
    p = tmp_path / "c.pt"
    torch.save({"samples": []}, p)
    with pytest.raises(ValueError, match="No samples found"):
        load_g_agent_samples(p)
    bad = _record()
    del bad["edge_scores"]
    torch.save({"samples": [bad]}, p)
    with pytest.raises(ValueError, match=r"missing keys: \['edge_scores'\]"):
        load_g_agent_samples(p)
    torch.save({"samples": [_record(is_answer_reachable=False, answer_node_locals=torch.zeros(0, dtype=torch.long))]}, p)
    assert len(load_g_agent_samples(p)) == 1
    with pytest.raises(ValueError, match="No usable samples"):
        load_g_agent_samples(p, drop_unreachable=True)
    torch.save({"samples": [_record(edge_head_locals=torch.tensor([0, 3]))]}, p)
    with pytest.raises(ValueError, match="edge_head_locals out of range"):
        load_g_agent_samples(p)

    torch.save({"samples": [_record(extra=_Opaque())]}, p)  # a pickled object: refused, not unpickled
    with pytest.raises(ValueError, match="weights_only=True"):
        load_g_agent_samples(p)
    torch.save({"samples": [_record()]}, p)
    (s,) = load_g_agent_samples(p)
    assert s.sample_id == "a" and s.edge_scores.dtype == torch.float32 and s.start_node_locals.tolist() == [0]


def test_hook_refusals_and_disabled_block(tmp_path):
    from evi_rag_amd.bfs_chains import maybe_build_bfs_chains

    assert maybe_build_bfs_chains({}) == {}
    assert maybe_build_bfs_chains({"bfs_chain_eval": {"enabled": False, "max_chain_length": 0}}) == {}
    base = {"dataset": {"artifact_dir": str(tmp_path)}, "run": {"split": "test"}}
    with pytest.raises(ValueError, match="schema_version must be a positive integer"):
        maybe_build_bfs_chains({**base, "bfs_chain_eval": {"enabled": True, "schema_version": 0, "max_chain_length": 2}})
    with pytest.raises(ValueError, match="max_chain_length must be a positive integer"):
        maybe_build_bfs_chains({**base, "bfs_chain_eval": {"enabled": True, "max_chain_length": 0}})
    with pytest.raises(FileNotFoundError, match="g_agent_path not found"):
        maybe_build_bfs_chains({**base, "bfs_chain_eval": {"enabled": True, "max_chain_length": 2}})
    assert not (tmp_path / "eval_bfs").exists()


def test_builder_refusals_before_device_work():
    from evi_rag_amd import bfs_chains as bc
    from evi_rag_amd.g_agent import GAgentSample

    def sample(scores, starts=(0,)):
        return GAgentSample(sample_id="x", question="q", question_emb=torch.zeros(1, 2), node_entity_ids=torch.tensor([1, 2]),
                            node_embedding_ids=torch.tensor([0, 1]), edge_head_locals=torch.tensor([0]),
                            edge_tail_locals=torch.tensor([1]), edge_relations=torch.tensor([0]),
                            edge_scores=torch.tensor(scores, dtype=torch.float32), edge_labels=torch.zeros(1),
                            start_entity_ids=torch.tensor([1]), answer_entity_ids=torch.tensor([2]),
                            gt_path_edge_local_ids=torch.zeros(0, dtype=torch.long),
                            start_node_locals=torch.tensor(list(starts), dtype=torch.long))

    with pytest.raises(ValueError, match="non-finite edge score"):
        bc.build_bfs_candidate_chains(sample([float("nan")]), settings=bc.BFSChainSettings(max_chain_length=2))
    with pytest.raises(ValueError, match="max_chain_length must be a positive integer"):
        bc.build_bfs_candidate_chains(sample([0.5]), settings=bc.BFSChainSettings(max_chain_length=0))
    with pytest.raises(ValueError, match="exceeds the bound"):
        bc.build_bfs_candidate_chains(sample([0.5]), settings=bc.BFSChainSettings(max_chain_length=33))
    # no seeds: [] before anything is checked, as in the reference
    assert bc.build_bfs_candidate_chains(sample([float("nan")], starts=()), settings=bc.BFSChainSettings(max_chain_length=0)) == []


def test_c_abi_rejects_bad_arguments_on_the_host():
    from evi_rag_amd import _lib

    lib = _lib.load()
    assert lib.evi_bfs_chains_workspace_bytes(10, 20, 100, 128) > 0
    assert lib.evi_bfs_chains_workspace_bytes(-1, 20, 100, 128) == 0
    one = (ctypes.c_int64 * 8)()
    p = ctypes.addressof(one)

    def call(**kw):
        args = dict(S=1, max_len=3, min_len=1, cap=5000, max_out=10, lds=0, slots=0, bits=64, ws=1 << 20, wsp=p)
        args.update(kw)
        return lib.evi_bfs_chains(args["S"], p, p, p, p, p, 2, 1, 8, 8, p, p, p, p, p, p, args["max_len"], args["min_len"],
                                  args["cap"], 1, -1, 1, 0, args["max_out"], args["lds"], args["slots"], args["bits"], p, p, p, p,
                                  p, p, args["wsp"], args["ws"], None)

    for kw, text in ((dict(S=-1), "num_samples"), (dict(max_len=0), "max_chain_length"), (dict(max_len=33), "max_chain_length"),
                     (dict(max_out=-1), "max_out"), (dict(lds=100000), "lds_records"), (dict(slots=1 << 20), "lds_sort_slots"),
                     (dict(bits=0), "hash_bits"), (dict(bits=65), "hash_bits"), (dict(ws=16), "workspace"),
                     (dict(wsp=None), "workspace")):
        assert lib.evi_bfs_chains and call(**kw) == _lib.EVI_ERR_INVALID, kw
        assert text in _lib.last_error(), (kw, _lib.last_error())
