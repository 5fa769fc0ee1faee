"""Times one optimiser step (gradient norm + update) on the D = H = 1024 retriever's parameters (about 9.4 M floats):

  (a) FlatAdamW (evi_adamw_step), the default configuration;
  (b) FlatOptimizer AdamW (evi_optim_step) with the two-group no-decay split (biases and LayerNorm weights: weight_decay 0).

Both move 7 floats per parameter in the update plus 1 in the norm pass, so (b) should sit close to (a); DESIGN.md §4 records both and why they differ.
The two are timed in alternating rounds inside one process (device events around `--steps` steps after `--warmup` steps);
(a)'s spread is the range of its own rounds.  Prints one JSON line.

    python tools/optim_step_probe.py [--dim 1024] [--rounds 7] [--steps 200] [--warmup 20]
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dim", type=int, default=1024)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("optim_step_probe needs the GPU: a CPU timing says nothing about it")
    from evi_rag_amd.retriever import Retriever
    from evi_rag_amd.train import FlatAdamW, FlatOptimizer, setup_optimizer

    dev = torch.device("cuda:0")

    def model():
        torch.manual_seed(0)
        return Retriever(emb_dim=args.dim, hidden_dim=args.dim).to(dev)

    split = [{"params": ["bias", "struct_proj.1", "state_net.1"], "weight_decay": 0.0}]
    opt_a = setup_optimizer(model(), {"type": "adamw", "lr": 1e-3, "weight_decay": 1e-4})
    opt_b = setup_optimizer(model(), {"type": "adamw", "lr": 1e-3, "weight_decay": 1e-4, "param_groups": split})
    assert type(opt_a) is FlatAdamW and type(opt_b) is FlatOptimizer and len(opt_b.param_groups) == 2
    for opt in (opt_a, opt_b):
        opt.grad.normal_(generator=torch.Generator(device=dev).manual_seed(1))

    def timed(opt):
        for _ in range(args.warmup):
            opt.step(max_norm=1.0)
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        for _ in range(args.steps):
            opt.step(max_norm=1.0)
        stop.record()
        stop.synchronize()
        return start.elapsed_time(stop) * 1e3 / args.steps  # microseconds per step

    a, b = [], []
    for _ in range(args.rounds):  # alternating: whatever else the host is doing falls on both
        a.append(timed(opt_a))
        b.append(timed(opt_b))
    n = opt_a.numel
    med_a, med_b = statistics.median(a), statistics.median(b)
    print(json.dumps({"parameters": n, "groups_b": [len(g["params"]) for g in opt_b.param_groups], "steps": args.steps, "rounds": args.rounds,
                      "flat_adamw_us": {"median": round(med_a, 2), "min": round(min(a), 2), "max": round(max(a), 2)},
                      "flat_optimizer_two_groups_us": {"median": round(med_b, 2), "min": round(min(b), 2), "max": round(max(b), 2)},
                      "b_inside_spread_of_a": bool(min(a) <= med_b <= max(a)),
                      "bytes_per_step": 32 * n, "flat_adamw_gbps": round(32 * n / med_a / 1e3, 1),
                      "flat_optimizer_gbps": round(32 * n / med_b / 1e3, 1)}))


if __name__ == "__main__":
    main()
