"""CPU: the host side of the reference's `optimizer_cfg` / `scheduler_cfg` contract (src/utils/optimization.py:20-170,
src/models/retriever_module.py:336-370) — group construction against a fixture recorded from the reference's own
`_build_param_groups` (tests/golden/make_golden_optim.py), the two schedules against torch's, and the refusals.
"""
import gzip
import json
import os
import types

import pytest
import torch

from evi_rag_amd import _lib
from evi_rag_amd import train as T

HERE = os.path.dirname(os.path.abspath(__file__))

with gzip.open(os.path.join(HERE, "golden", "optim_groups.json.gz"), "rt", encoding="utf-8") as _fh:
    FIXTURE = json.load(_fh)


class Named(torch.nn.Module):
    """A module whose `named_parameters()` are the given names (dots included) and shapes."""

    def __init__(self, names_shapes):
        super().__init__()
        self._named = [(n, torch.nn.Parameter(torch.zeros(*s))) for n, s in names_shapes]

    def named_parameters(self, prefix="", recurse=True, remove_duplicate=True):
        return iter(self._named)

    def parameters(self, recurse=True):
        return iter(p for _, p in self._named)


def test_fixture_covers_the_retriever_and_every_form():
    from evi_rag_amd.retriever import Retriever

    assert [(n, list(p.shape)) for n, p in Retriever(emb_dim=64, hidden_dim=64).named_parameters()] == [tuple(x) for x in FIXTURE["parameters"]]
    assert len(FIXTURE["parameters"]) == 25 and len(FIXTURE["cases"]) >= 10


@pytest.mark.parametrize("key", sorted(FIXTURE["cases"]))
def test_param_groups_equal_the_reference(key):
    case = FIXTURE["cases"][key]
    module = Named(case.get("module", FIXTURE["parameters"]))
    names = {id(p): n for n, p in module.named_parameters()}
    if "raises" in case:
        with pytest.raises(getattr(__import__("builtins"), case["raises"])):
            T.build_param_groups(module, case["param_groups"])
        return
    got = T.build_param_groups(module, case["param_groups"])
    if "params" in case:
        assert [names[id(p)] for p in got] == case["params"]
        return
    assert all(isinstance(g, dict) for g in got)
    assert [{"names": [names[id(p)] for p in g["params"]], "overrides": {k: v for k, v in g.items() if k != "params"}} for g in got] == case["groups"]


def _two_group_sgd():
    a, b = torch.nn.Parameter(torch.zeros(3)), torch.nn.Parameter(torch.zeros(2))
    return torch.optim.SGD([{"params": [a], "lr": 1e-3}, {"params": [b], "lr": 7e-2}], lr=1e-3)


def _ours_like(opt):
    # what a schedule needs of a FlatOptimizer: param_groups with lr and initial_lr
    return types.SimpleNamespace(param_groups=[{"lr": g["lr"], "initial_lr": g["lr"]} for g in opt.param_groups])


def _rel(a, b):
    return abs(a - b) / max(abs(b), 1e-300)


@pytest.mark.parametrize("eta_min", [0.0, 1e-5])
def test_cosine_schedule_equals_torch_per_group(eta_min):
    ref_opt = _two_group_sgd()
    ours_opt = _ours_like(ref_opt)
    ref = torch.optim.lr_scheduler.CosineAnnealingLR(ref_opt, T_max=10, eta_min=eta_min)
    ours = T.CosineSchedule(ours_opt, t_max=10, eta_min=eta_min)
    for epoch in range(25):  # past T_max: the curve climbs back
        ref_opt.step()
        ref.step()
        ours.step()
        for g, want in zip(ours_opt.param_groups, ref.get_last_lr()):
            assert g["lr"] == want or _rel(g["lr"], want) <= 1e-12, (epoch, g["lr"], want)
    assert ours.last_epoch == ref.last_epoch == 25


@pytest.mark.parametrize("t_mult", [1, 2])
@pytest.mark.parametrize("eta_min", [0.0, 1e-5])
def test_cosine_restart_schedule_equals_torch_per_group(t_mult, eta_min):
    ref_opt = _two_group_sgd()
    ours_opt = _ours_like(ref_opt)
    ref = torch.optim.lr_scheduler.CosineAnnealingWarmRestarts(ref_opt, T_0=4, T_mult=t_mult, eta_min=eta_min)
    ours = T.CosineRestartSchedule(ours_opt, t_0=4, t_mult=t_mult, eta_min=eta_min)
    seen = []
    for epoch in range(25):
        ref_opt.step()
        ref.step()
        ours.step()
        for g, want in zip(ours_opt.param_groups, ref.get_last_lr()):
            assert g["lr"] == want or _rel(g["lr"], want) <= 1e-12, (epoch, g["lr"], want)
        assert ours.position() == (ref.T_cur, ref.T_i)
        seen.append(ours_opt.param_groups[1]["lr"])
    assert seen.count(7e-2) == (6 if t_mult == 1 else 2)  # restarts (epochs 4, 8, .. 24 / 4 and 12): back at the group's own base rate
    # the position is a function of last_epoch alone (what a checkpoint keeps)
    again = T.CosineRestartSchedule(ours_opt, t_0=4, t_mult=t_mult, eta_min=eta_min)
    again.last_epoch = ours.last_epoch
    assert again.position() == ours.position()
    with pytest.raises(ValueError):
        T.CosineRestartSchedule(ours_opt, t_0=0)
    with pytest.raises(ValueError):
        T.CosineRestartSchedule(ours_opt, t_0=4, t_mult=0)


def test_single_rate_optimizer_keeps_its_schedule():
    # FlatAdamW's interface (one lr / initial_lr pair, no param_groups) is still served
    opt = types.SimpleNamespace(lr=1e-3, initial_lr=1e-3)
    T.CosineRestartSchedule(opt, t_0=4).step()
    assert _rel(opt.lr, 1e-3 * (1 + 2 ** -0.5) / 2) <= 1e-12


def test_refusals():
    module = Named(FIXTURE["parameters"])
    with pytest.raises(ValueError, match="closure-based.*not supported"):
        T.setup_optimizer(module, {"type": "lbfgs"})
    for name in ("muon", "SingleDeviceMuon", "muon_distributed"):
        with pytest.raises(ImportError, match="Muon optimizer requested but the 'muon-optimizer' package is not installed"):
            T.setup_optimizer(module, {"type": name})
    with pytest.raises(ValueError, match="Unsupported optimizer type 'lion'"):
        T.setup_optimizer(module, {"name": "lion"})
    with pytest.raises(TypeError, match="unexpected option 'nesterov'"):
        T.setup_optimizer(module, {"type": "adam", "nesterov": True})
    with pytest.raises(TypeError, match="unexpected option 'momentum'"):
        T.setup_optimizer(module, {"type": "adamw", "param_groups": [{"params": ["bias"], "momentum": 0.9}]})
    with pytest.raises(TypeError, match="unexpected option 'beta'"):
        T.setup_optimizer(module, {"type": "adamw", "beta": 0.9})  # the default path refuses it too
    with pytest.raises(ValueError, match="no trainable parameters"):
        T.setup_optimizer(Named([]), {"type": "sgd"})
    with pytest.raises(ValueError, match="valid nn.Module"):
        T.setup_optimizer(None, {})
    with pytest.raises(TypeError, match="must be a mapping"):
        T.setup_optimizer(module, ["adamw"])
    # accepted configurations get as far as the device check: there is no CPU fallback
    for cfg in ({"type": "sgd", "momentum": 0.9, "foreach": True}, {"type": "adamw", "amsgrad": True, "maximize": False},
                {"type": "adamw", "param_groups": [{"params": ["bias"], "weight_decay": 0.0}]}, {"type": "adamw"}):
        with pytest.raises(RuntimeError, match="MI355X only"):
            T.setup_optimizer(module, cfg)
    with pytest.raises(ValueError, match="'maximize' is not supported"):
        T.setup_optimizer(module, {"type": "sgd", "maximize": True})


def test_library_refuses_more_groups_than_the_kernel_arguments_hold():
    # argument validation happens on the host before any device work, so it is safe without a GPU
    lib = _lib.load()
    table = (_lib.EviOptimGroup * 17)()
    rc = lib.evi_optim_step(0, None, None, None, None, None, 0, table, 17, 1.0, None, 0.0, None)
    assert rc == _lib.EVI_ERR_UNSUPPORTED and "17 parameter groups" in _lib.last_error()
    with pytest.raises(NotImplementedError):
        _lib.check(rc)
    assert lib.evi_optim_step(8, None, None, None, None, None, 0, table, 1, 1.0, None, 0.0, None) == _lib.EVI_ERR_INVALID
    table[0].begin, table[0].end, table[0].step = 0, 6, 1  # not on a 16-byte boundary
    assert lib.evi_optim_step(0, None, None, None, None, None, 8, table, 1, 1.0, None, 0.0, None) == _lib.EVI_ERR_INVALID
    assert "16-byte boundaries" in _lib.last_error()


def test_group_and_restart_overrides_reach_the_config_tree(tmp_path, monkeypatch):
    """The README's grouped command line: `model.optimizer_cfg.param_groups=[...]` and the restart schedule arrive as the plain
    containers `setup_optimizer` / `RetrieverTrainer` read (the training entry point passes both nodes on as they are)."""
    from evi_rag_amd import hydra_lite as hl
    from tests.config_tree import write_tree

    monkeypatch.setenv("EVI_TEST_PROJECT_ROOT", str(tmp_path / "proj"))
    cfg = hl.compose(write_tree(tmp_path, tmp_path / "data"), "train", [
        "experiment=train_retriever", "dataset=toyqa",
        "model.optimizer_cfg.param_groups=[{params: [bias, struct_proj.1, state_net.1], weight_decay: 0.0}, {params: [entity_proj, relation_proj, query_proj], lr: 3.0e-4}]",
        "model.optimizer_cfg.type=nadam", "model.scheduler_cfg.type=cosine_restart", "+model.scheduler_cfg.t_0=20"])
    opt_cfg, sched_cfg = cfg["model"]["optimizer_cfg"], cfg["model"]["scheduler_cfg"]
    assert opt_cfg["type"] == "nadam" and sched_cfg["type"] == "cosine_restart" and sched_cfg["t_0"] == 20
    groups = T.build_param_groups(Named(FIXTURE["parameters"]), opt_cfg["param_groups"])
    assert [len(g["params"]) for g in groups] == [14, 3, 8]
    assert groups[0]["weight_decay"] == 0.0 and groups[1]["lr"] == 3.0e-4 and set(groups[2]) == {"params"}
