"""Writes tests/golden/optim_groups.json.gz: the parameter groups the reference's own `_build_param_groups`
(src/utils/optimization.py:82-131) forms for a set of `param_groups` configurations, over a module whose `named_parameters()`
are the 25 names and shapes of `Retriever`.  Run where the reference checkout is available:

    python tests/golden/make_golden_optim.py /path/to/reference

The fixture holds names and numbers only: per configuration the `param_groups` value, and either the groups as lists of
parameter names plus overrides or the type of the exception raised.  tests/test_optim_cfg_cpu.py compares
`evi_rag_amd.train.build_param_groups` with it.
"""
import gzip
import importlib.util
import json
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

CONFIGS = {
    # a mapping of named groups: a bare suffix, then a module prefix
    "mapping_of_groups": {"no_decay": {"params": ["bias"], "weight_decay": 0.0},
                          "state": {"params": ["state_net"], "lr": 5.0e-4}},
    # one group given directly
    "single_group": {"params": ["bias"], "weight_decay": 0.0},
    # a sequence of groups, `names` instead of `params`, a string instead of a list
    "sequence": [{"names": "score_head", "lr": 1.0e-4}, {"params": ["entity_proj", "relation_proj", "query_proj"], "lr": 2.0e-3}],
    "glob": [{"params": ["*_proj.network.0.*"], "lr": 2.0e-3}, {"params": ["state_net.[14].*"], "weight_decay": 0.0}],
    "bare_suffix": [{"params": ["bias"], "weight_decay": 0.0}],
    "prefix": [{"params": ["state_net"], "lr": 1.0e-4}],
    # `struct_proj` is no prefix of `struct_gate_net.*`; `proj` is neither a prefix nor a suffix of anything
    "prefix_is_whole_components": [{"params": ["struct_proj", "proj"], "lr": 1.0e-4}],
    "exact_name": [{"params": ["non_text_entity_emb.weight", " score_head.bias "], "weight_decay": 0.0}],
    # first match wins: the biases of state_net stay in the first group
    "overlap_first_wins": [{"params": ["bias", "struct_proj.1.weight", "state_net.1.weight"], "weight_decay": 0.0},
                           {"params": ["state_net", "*.bias"], "lr": 1.0e-4}],
    "group_matching_nothing": [{"params": ["*norm*"], "weight_decay": 0.0}, {"params": ["bias"], "weight_decay": 0.0, "lr": 3.0e-3}],
    "group_without_patterns": [{"lr": 1.0}, {"params": [], "lr": 2.0}, {"params": ["q_gate"], "lr": 3.0}],
    "everything_in_one_group": [{"params": ["*"], "lr": 1.0e-4}],
    "matches_nothing_at_all": [{"params": ["*norm*"], "weight_decay": 0.0}, {"params": ["decoder"], "lr": 1.0}],
    "not_a_group_container": "bias",
    "patterns_not_a_sequence": [{"params": 7}],
}


class Named(torch.nn.Module):
    """A module whose `named_parameters()` are the given names (dots included) and shapes."""

    def __init__(self, names_shapes):
        super().__init__()
        self._named = [(n, torch.nn.Parameter(torch.zeros(*s))) for n, s in names_shapes]

    def named_parameters(self, prefix="", recurse=True, remove_duplicate=True):
        return iter(self._named)


def record(build, module, cfg):
    names = {id(p): n for n, p in module.named_parameters()}
    try:
        groups = build(module, cfg)
    except Exception as exc:  # the type is the contract
        return {"raises": type(exc).__name__}
    if groups and not isinstance(groups[0], dict):
        return {"params": [names[id(p)] for p in groups]}
    return {"groups": [{"names": [names[id(p)] for p in g["params"]], "overrides": {k: v for k, v in g.items() if k != "params"}}
                       for g in groups]}


def main(reference_root):
    from evi_rag_amd.retriever import Retriever

    spec = importlib.util.spec_from_file_location("reference_optimization", os.path.join(reference_root, "src", "utils", "optimization.py"))
    ref = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ref)
    names_shapes = [(n, list(p.shape)) for n, p in Retriever(emb_dim=64, hidden_dim=64).named_parameters()]
    assert len(names_shapes) == 25
    module = Named(names_shapes)
    cases = {"no_param_groups": {"param_groups": None, **record(ref._build_param_groups, module, None)}}
    for key, cfg in CONFIGS.items():
        cases[key] = {"param_groups": cfg, **record(ref._build_param_groups, module, cfg)}
    cases["empty_module"] = {"param_groups": None, "module": [], **record(ref._build_param_groups, Named([]), None)}
    out = os.path.join(HERE, "optim_groups.json.gz")
    with gzip.GzipFile(out, "wb", mtime=0) as fh:
        fh.write(json.dumps({"parameters": names_shapes, "cases": cases}, indent=1, sort_keys=True).encode("utf-8"))
    print(f"wrote {out}: {len(cases)} configurations")
    for key, c in cases.items():
        print(" ", key, c.get("raises") or [len(g["names"]) for g in c.get("groups", [])] or len(c.get("params", [])))


if __name__ == "__main__":
    main(sys.argv[1])
