"""GPU: the grouped, multi-rule optimiser step (csrc/optim.hip evi_optim_step, train.FlatOptimizer) and the trainer around it.

The oracle of every rule is torch.optim.<Rule>(..., foreach=False) + torch.nn.utils.clip_grad_norm_ on clones fed the same
gradients — what the reference's setup_optimizer (src/utils/optimization.py:20-35) builds and Lightning's gradient_clip_val
clips.  Three groups whose members interleave in declaration order (so the group-ordered flat layout differs from the
parameter order), one of them a single 1-element parameter, each with its own lr and weight_decay.

Tolerance: the bound the project holds AdamW to (rtol 2e-6, atol 2e-7, elementwise against torch's f32 result).  RMSprop
misses it on a few of the 2.2 M elements of the large parameter, and not by rounding alone: the coupled weight decay feeds a
difference d in p back as lr wd d / (sqrt(square_avg) + eps), and where an element's gradients happen to be tiny (square_avg
~ 1e-10 with eps 1e-8) that factor exceeds 1, so a last-bit difference triples per step (measured: 0.06, 0.18, 0.56, 2.0 of
the bound over steps 1-4).  torch's own f32 result moves away from the f64 result in the same way, so for plain RMSprop a
parameter that misses the elementwise bound must instead lie within TWICE torch's own f32 distance from the same rule run in
f64 on the CPU (max |.| over the parameter; one extra rounding per operation — a wrong order of operations shows at ~1e-3).
Measured on the MI355X, large parameter, max over the parameter of |. - f64| after steps 0..8:
  torch f32: 8.38e-6 8.37e-6 2.87e-6 2.19e-6 3.66e-6 3.62e-6 3.08e-6 2.29e-6 1.84e-6
  ours:      8.38e-6 8.37e-6 2.87e-6 2.19e-6 3.20e-6 3.17e-6 2.70e-6 2.01e-6 1.61e-6   (0.87 - 1.00 of torch's)
  ours against torch f32, in units of the elementwise bound: 0.00 0.06 0.18 0.56 2.02 1.36 1.40 1.07 0.94
Every other case holds the elementwise bound with room (worst 0.43 of it, AdamW; centred RMSprop 0.74).
"""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))

SHAPES = [(33, 17), (5,), (1,), (64, 64), (7, 3), (1100, 2000)]  # odd counts: padded slots; the last exceeds 2048 x 256 x 4 elements
MEMBERS = [(0, 3), (2,), (1, 4, 5)]                               # group -> parameters (declaration order interleaves the groups)
GROUP_CFG = [{"lr": 3e-3, "weight_decay": 0.05}, {"lr": 1e-3, "weight_decay": 0.0}, {"lr": 5e-3, "weight_decay": 0.01}]

# rule, options of the constructor, per-group extra overrides
CASES = {
    "adamw": ("adamw", {"betas": (0.9, 0.99)}, None),
    "adamw-amsgrad-in-one-group": ("adamw", {"betas": (0.9, 0.99)}, [{"amsgrad": True}, {}, {}]),
    "adam": ("adam", {}, None),
    "adam-amsgrad": ("adam", {"amsgrad": True, "eps": 1e-6}, None),
    "sgd": ("sgd", {}, None),
    "sgd-momentum-dampening": ("sgd", {"momentum": 0.9, "dampening": 0.1}, [{}, {"momentum": 0.0}, {}]),
    "sgd-nesterov": ("sgd", {"momentum": 0.9, "nesterov": True, "dampening": 0.0}, None),
    "rmsprop": ("rmsprop", {}, None),
    "rmsprop-centered-momentum": ("rmsprop", {"centered": True, "momentum": 0.9, "alpha": 0.9}, None),
    "adagrad": ("adagrad", {}, None),
    "adagrad-lr-decay": ("adagrad", {"lr_decay": 0.1, "initial_accumulator_value": 0.5, "eps": 1e-8}, None),
    "adamax": ("adamax", {}, None),
    "adamax-betas": ("adamax", {"betas": (0.8, 0.95), "eps": 1e-6}, None),
    "nadam": ("nadam", {}, None),
    "nadam-momentum-decay": ("nadam", {"momentum_decay": 0.01, "betas": (0.8, 0.95)}, None),
    "adadelta": ("adadelta", {}, None),
    "adadelta-rho": ("adadelta", {"rho": 0.8, "eps": 1e-5}, None),
}
TORCH = {"adamw": torch.optim.AdamW, "adam": torch.optim.Adam, "sgd": torch.optim.SGD, "rmsprop": torch.optim.RMSprop,
         "adagrad": torch.optim.Adagrad, "adamax": torch.optim.Adamax, "nadam": torch.optim.NAdam, "adadelta": torch.optim.Adadelta}
RTOL, ATOL = 2e-6, 2e-7
F64_CASES = ("rmsprop",)  # see the module docstring; centred RMSprop with momentum holds the elementwise bound (0.74 of it)


def _groups(params, extra):
    return [dict(GROUP_CFG[i], **((extra or [{}] * 3)[i]), params=[params[j] for j in MEMBERS[i]]) for i in range(3)]


def _gradients(dev, steps=9):
    """The gradients of the 8 + 1 steps, made once and shared by every case (never modified)."""
    if not hasattr(_gradients, "cache"):
        gen = torch.Generator(device=dev).manual_seed(1)
        _gradients.cache = [[torch.randn(s, device=dev, generator=gen) * (10.0 if step % 2 == 0 else 0.01) for s in SHAPES]
                            for step in range(steps)]
    return _gradients.cache


def _initial(dev):
    gen = torch.Generator(device=dev).manual_seed(0)
    return [torch.randn(s, device=dev, generator=gen) for s in SHAPES]


@pytest.mark.parametrize("case", sorted(CASES))
def test_rule_equals_torch_with_groups_and_clipping(dev, case):
    from evi_rag_amd.train import FlatOptimizer

    rule, options, extra = CASES[case]
    ours = [torch.nn.Parameter(t.clone()) for t in _initial(dev)]
    theirs = [torch.nn.Parameter(t.clone()) for t in _initial(dev)]
    opt = FlatOptimizer(_groups(ours, extra), rule=rule, **options)
    ref = TORCH[rule](_groups(theirs, extra), foreach=False, **options)
    exact = ref64 = None
    if case in F64_CASES:
        exact = [torch.nn.Parameter(t.double().cpu()) for t in _initial(dev)]
        ref64 = TORCH[rule](_groups(exact, extra), foreach=False, **options)
    assert [g["lr"] for g in opt.param_groups] == [3e-3, 1e-3, 5e-3] == [g["initial_lr"] for g in opt.param_groups]
    # the layout is group by group, not in declaration order
    assert [p.data_ptr() for p in opt.params] == [ours[j].data_ptr() for m in MEMBERS for j in m]
    assert all(p.data_ptr() >= opt.flat.data_ptr() and p.grad.data_ptr() >= opt.grad.data_ptr() for p in ours)
    worst = 0.0
    for step, grads in enumerate(_gradients(dev)):
        last = step == 8  # the last step: grad_scale (the 1 / world of a summed all-reduce) is part of the clipped quantity
        opt.zero_grad()
        for p, q, g in zip(ours, theirs, grads):
            p.grad.add_(g * (2.0 if last else 1.0))
            q.grad = g.clone()
        torch.nn.utils.clip_grad_norm_(theirs, 1.0)
        ref.step()
        opt.step(grad_scale=0.5 if last else 1.0, max_norm=1.0)
        if exact is not None:
            for x, g in zip(exact, grads):
                x.grad = g.double().cpu()
            torch.nn.utils.clip_grad_norm_(exact, 1.0)
            ref64.step()
        for i, (p, q) in enumerate(zip(ours, theirs)):
            p, q = p.detach(), q.detach()
            err = float(((p - q).abs() / (ATOL + RTOL * q.abs())).max())
            worst = max(worst, err)
            print(f"{case} step {step} param {i}: max |ours - torch| / (atol + rtol |torch|) = {err:.3f}")
            if exact is not None:
                x = exact[i].detach().to(dev)
                d_ours, d_torch = float((p.double() - x).abs().max()), float((q.double() - x).abs().max())
                print(f"{case} step {step} param {i}: max |ours - f64| = {d_ours:.3e}, max |torch f32 - f64| = {d_torch:.3e}")
                assert err <= 1.0 or d_ours <= 2.0 * d_torch, (case, step, i, err, d_ours, d_torch)
            else:
                assert torch.allclose(p, q, rtol=RTOL, atol=ATOL), (case, step, i, float((p - q).abs().max()))
    print(f"{case}: worst {worst:.3f} of the bound")
    # only the state the rule's options need is held
    want = {"adamw": 2, "adamw-amsgrad-in-one-group": 3, "adam": 2, "adam-amsgrad": 3, "sgd": 0, "sgd-momentum-dampening": 1, "sgd-nesterov": 1,
            "rmsprop": 1, "rmsprop-centered-momentum": 3, "adagrad": 1, "adagrad-lr-decay": 1, "adamax": 2, "adamax-betas": 2, "nadam": 2,
            "nadam-momentum-decay": 2, "adadelta": 2, "adadelta-rho": 2}[case]
    assert len(opt.state) == want
    v0 = ours[0]._version
    opt.zero_grad()
    opt.step()
    assert ours[0]._version > v0  # the kernel's write is visible to version-keyed caches


def test_default_configuration_is_flat_adamw_bit_for_bit(dev):
    from evi_rag_amd.train import FlatAdamW, FlatOptimizer, setup_optimizer

    def module():
        torch.manual_seed(5)
        return torch.nn.Sequential(torch.nn.Linear(33, 17), torch.nn.LayerNorm(17), torch.nn.Linear(17, 1)).to(dev)

    a, b, c = module(), module(), module()
    opt_a = setup_optimizer(a, {"type": "adamw", "lr": 3e-3, "weight_decay": 1e-4})
    opt_b = FlatAdamW(b.parameters(), lr=3e-3, weight_decay=1e-4)
    opt_c = setup_optimizer(c, {"name": "AdamW", "lr": 3e-3, "weight_decay": 1e-4, "amsgrad": True})
    assert type(opt_a) is FlatAdamW and type(opt_c) is FlatOptimizer
    assert sorted(opt_a.state_dict()) == sorted(opt_b.state_dict()) == ["exp_avg", "exp_avg_sq", "initial_lr", "lr", "step"]
    gen = torch.Generator(device=dev).manual_seed(2)
    for step in range(4):
        opt_a.zero_grad()
        opt_b.zero_grad()
        for p, q in zip(a.parameters(), b.parameters()):
            g = torch.randn(p.shape, device=dev, generator=gen) * (10.0 if step % 2 == 0 else 0.01)
            p.grad.add_(g)
            q.grad.add_(g)
        opt_a.step(max_norm=1.0)
        opt_b.step(max_norm=1.0)
    for p, q in zip(a.parameters(), b.parameters()):
        assert torch.equal(p, q)
    assert torch.equal(opt_a.flat, opt_b.flat) and torch.equal(opt_a.exp_avg_sq, opt_b.exp_avg_sq)


@pytest.mark.parametrize("rule,options", [("adam", {"amsgrad": True}), ("sgd", {"momentum": 0.9}), ("nadam", {})])
def test_state_dict_round_trip_continues_bit_for_bit(dev, rule, options, tmp_path):
    from evi_rag_amd.train import FlatOptimizer

    shapes = SHAPES[:5]
    grads = [g[:5] for g in _gradients(dev)]
    members = [(0, 3), (2,), (1, 4)]

    def make(tensors):
        ps = [torch.nn.Parameter(t.clone()) for t in tensors]
        return ps, FlatOptimizer([dict(GROUP_CFG[i], params=[ps[j] for j in m]) for i, m in enumerate(members)], rule=rule, **options)

    def run(ps, opt, steps):
        for gs in steps:
            opt.zero_grad()
            for p, g in zip(ps, gs):
                p.grad.add_(g)
            opt.step(max_norm=1.0)

    ps, opt = make(_initial(dev)[:5])
    run(ps, opt, grads[:3])
    opt.param_groups[1]["lr"] = 7e-4  # a schedule's work travels with the state
    path = tmp_path / "opt.pt"
    torch.save({"optimizer": opt.state_dict(), "params": [p.detach().clone() for p in ps]}, path)
    blob = torch.load(path, map_location=dev, weights_only=True)
    ps2, opt2 = make(blob["params"])
    opt2.load_state_dict(blob["optimizer"])
    assert opt2.steps == [3, 3, 3] and opt2.param_groups[1]["lr"] == 7e-4 and opt2.param_groups[1]["initial_lr"] == 1e-3
    assert opt2.mu_products == opt.mu_products
    run(ps, opt, grads[3:6])
    run(ps2, opt2, grads[3:6])
    for p, q in zip(ps, ps2):
        assert torch.equal(p, q)
    for k in opt.state:
        assert torch.equal(opt.state[k], opt2.state[k])
    assert len(shapes) == len(ps)
    # a state that does not fit is refused
    _, other = make(_initial(dev)[:5])
    sd = opt.state_dict()
    sd["rule"] = "adagrad"
    with pytest.raises(ValueError, match="does not fit"):
        other.load_state_dict(sd)


def test_seventeen_groups_are_refused(dev):
    from evi_rag_amd.train import FlatOptimizer

    ps = [torch.nn.Parameter(torch.zeros(3, device=dev)) for _ in range(17)]
    with pytest.raises(NotImplementedError, match="17 parameter groups"):
        FlatOptimizer([{"params": [p], "lr": 1e-3 * (i + 1)} for i, p in enumerate(ps)], rule="sgd")
    before = [p.data_ptr() for p in ps]
    opt = FlatOptimizer([{"params": [p], "lr": 1e-3 * (i + 1)} for i, p in enumerate(ps[:16])], rule="sgd")  # sixteen fit
    for p in ps[:16]:
        p.grad.fill_(1.0)
    opt.step()
    torch.cuda.synchronize()
    assert [round(float(p.detach()[0]) / -1e-3) for p in ps[:16]] == list(range(1, 17)) and ps[16].data_ptr() == before[16]


# InfoNCE's logit gradients sum to zero inside every graph, so the gradients of the two biases behind the logits are pure
# rounding noise, which Adam normalises to steps of size lr (tests/test_train_gpu.py: NOISE_ONLY, _close)
NOISE_ONLY = ("state_net.4.bias", "score_head.bias")
GROUPED_CFG = {"type": "adamw", "lr": 1e-2, "weight_decay": 1e-4, "param_groups": [{"params": ["bias", "*norm*"], "weight_decay": 0.0}]}
RESTART_CFG = {"type": "cosine_restart", "t_0": 2}


def _close(name, a, b, steps, lr):
    a, b = np.asarray(a), np.asarray(b)
    if name in NOISE_ONLY:
        return bool(np.abs(a - b).max() <= 2.0 * steps * lr)
    return bool(np.allclose(a, b, rtol=1e-4, atol=2e-5))


def _manual_reference(dev, batch, epochs, lr):
    """The same loop — one optimiser step per epoch — with torch.optim.AdamW over the two groups, clip_grad_norm_ and
    CosineAnnealingWarmRestarts around the differentiable mirror."""
    sys.path.insert(0, HERE)
    import train_rank_worker as w
    from evi_rag_amd.loss import RetrieverLoss

    model = w.make_model(dev)
    model.train()
    loss_fn = RetrieverLoss(infonce_temperature=0.5)
    named = list(model.named_parameters())
    opt = torch.optim.AdamW([{"params": [p for n, p in named if n.endswith("bias")], "weight_decay": 0.0},
                             {"params": [p for n, p in named if not n.endswith("bias")]}], lr=lr, weight_decay=1e-4, foreach=False)
    sched = torch.optim.lr_scheduler.CosineAnnealingWarmRestarts(opt, T_0=2, T_mult=1, eta_min=0.0)
    losses, rates = [], []
    for _ in range(epochs):
        opt.zero_grad(set_to_none=True)
        out = model(batch)
        lo = loss_fn(out, batch.labels, edge_batch=out.query_ids, num_graphs=batch.num_graphs)
        lo.loss.backward()
        torch.nn.utils.clip_grad_norm_(model.parameters(), 1.0)
        opt.step()
        sched.step()
        losses.append(float(lo.loss.detach()))
        rates.append(sched.get_last_lr())
    return model, losses, rates


def test_trainer_with_groups_and_restarts_equals_the_torch_loop(dev, tmp_path):
    sys.path.insert(0, HERE)
    import train_rank_worker as w
    from evi_rag_amd.loss import RetrieverLoss
    from evi_rag_amd.train import CosineRestartSchedule, FlatAdamW, FlatOptimizer, RetrieverTrainer

    batch = w.make_batch(0, dev)
    model = w.make_model(dev)

    def trainer_for(m, optimizer_cfg=GROUPED_CFG, scheduler_cfg=RESTART_CFG):
        return RetrieverTrainer(m, loss=RetrieverLoss(infonce_temperature=0.5), optimizer_cfg=optimizer_cfg, scheduler_cfg=scheduler_cfg,
                                gradient_clip_val=1.0)

    trainer = trainer_for(model)
    assert type(trainer.optimizer) is FlatOptimizer and type(trainer.scheduler) is CosineRestartSchedule
    groups = trainer.optimizer.param_groups
    names = {id(p): n for n, p in model.named_parameters()}
    assert len(groups) == 2 and all(names[id(p)].endswith("bias") for p in groups[0]["params"]) and len(groups[0]["params"]) == 12
    assert (groups[0]["weight_decay"], groups[1]["weight_decay"]) == (0.0, 1e-4)
    losses, logs = [], []
    for _ in range(3):  # three epochs of one step
        losses.append(float(trainer.training_step(batch)))
        logs.append(trainer.on_train_epoch_end())
    ref_model, ref_losses, ref_rates = _manual_reference(dev, batch, 3, 1e-2)
    for a, b in zip(losses, ref_losses):
        assert abs(a - b) <= 2e-5 * max(1.0, abs(b)), (losses, ref_losses)
    for log, want in zip(logs, ref_rates):
        assert abs(log["lr"] - want[0]) <= 1e-12 * want[0]  # 5e-3, 1e-2 (restart), 5e-3: group 0's
    assert [abs(g["lr"] - r) <= 1e-12 * r for g, r in zip(groups, ref_rates[-1])] == [True, True]
    for (n, p), q in zip(model.named_parameters(), ref_model.parameters()):
        assert _close(n, p.detach().cpu().numpy(), q.detach().cpu().numpy(), 3, 1e-2), (n, float((p - q).abs().max()))
    # checkpoint round trip: rates, steps, schedule position and state come back, and the next step is the same step
    path = tmp_path / "grouped.ckpt"
    trainer.save_checkpoint(path)
    torch.load(str(path), map_location="cpu", weights_only=True)
    model2 = w.make_model(dev)
    trainer2 = trainer_for(model2)
    trainer2.load_checkpoint(path)
    assert [g["lr"] for g in trainer2.optimizer.param_groups] == [g["lr"] for g in groups]
    assert trainer2.optimizer.steps == [3, 3] and trainer2.scheduler.last_epoch == 3 and trainer2.scheduler.position() == (1, 2)
    assert (trainer2.global_step, trainer2.current_epoch) == (3, 3)
    for k, v in trainer.optimizer.state.items():
        assert torch.equal(v, trainer2.optimizer.state[k])
    l1, l2 = float(trainer.training_step(batch)), float(trainer2.training_step(batch))
    assert l1 == l2
    for p, q in zip(model.parameters(), model2.parameters()):
        assert torch.equal(p, q)
    # a checkpoint in the layout written before there were groups (FlatAdamW's flat keys, `last_epoch` only) still loads
    model3 = w.make_model(dev)
    old = trainer_for(model3, {"type": "adamw", "lr": 1e-2, "weight_decay": 1e-4}, {"type": "cosine", "t_max": 4, "eta_min": 1e-6})
    assert type(old.optimizer) is FlatAdamW
    n = old.optimizer.numel
    blob = {"state_dict": {f"model.{k}": v.detach().cpu() + 0.5 for k, v in model3.state_dict().items()}, "epoch": 2, "global_step": 7,
            "optimizer_states": [{"step": 7, "lr": 5e-3, "initial_lr": 1e-2, "exp_avg": torch.full((n,), 0.25), "exp_avg_sq": torch.full((n,), 0.5)}],
            "lr_schedulers": [{"last_epoch": 2}]}
    torch.save(blob, str(tmp_path / "old.ckpt"))
    assert old.load_checkpoint(tmp_path / "old.ckpt") == {}
    assert (old.optimizer.step_count, old.optimizer.lr, old.optimizer.initial_lr, old.scheduler.last_epoch) == (7, 5e-3, 1e-2, 2)
    assert (old.global_step, old.current_epoch) == (7, 2) and float(old.optimizer.exp_avg[0]) == 0.25 and float(old.optimizer.exp_avg_sq[-1]) == 0.5
    assert torch.equal(model3.score_head.bias.cpu(), blob["state_dict"]["model.score_head.bias"])
    with pytest.raises(ValueError, match="written by FlatAdamW"):
        trainer2.optimizer.load_state_dict(blob["optimizer_states"][0])
