"""CPU: the float64 scorer model (tests/scorer_f64.py) pinned to the reference's own outputs and autograd.

tests/golden/retriever_{toy,mid,fwd,bwd}.npz hold the reference Retriever's f32 outputs and, for a fixed `gvec`,
d(sum_e gvec_e logit_e)/d(parameter) from its own autograd.  The float64 model must be that function to f32 rounding, so
that the GPU tests can judge the kernels by it on batches the goldens do not contain.

Bars: logits and edge embeddings within 2e-6 absolute, every `g_*` array within 1e-5 of its own max (1e-6 floor, the scale
rule of test_backward_gpu._check_grads).  Measured (worst of each golden; gradients as a fraction of the array's max):

    golden  logits   logits_fwd  logits_bwd  edge_embeddings  node_struct  worst gradient
    toy     2.0e-07  2.8e-07     2.5e-07     4.1e-07          5.2e-08      2.1e-06  (struct_gate_net.0.bias)
    mid     1.5e-07  2.2e-07     2.4e-07     6.1e-07          2.3e-07      1.4e-06  (struct_gate_net.0.weight)
    fwd     1.2e-07  1.2e-07     -           3.3e-07          7.3e-08      8.4e-07  (struct_proj.0.bias)
    bwd     1.2e-07  -           1.2e-07     3.0e-07          8.9e-08      8.9e-07  (entity_proj.network.0.bias)

The float64 loss is pinned to oracle/loss.py (f32 arithmetic, closed-form d total / d logits) on the same goldens' labels:
total within 2e-6 relative, gradient within 1e-5 of its max — both f32 rounding of the oracle (measured at most 1.2e-07 / 2.0e-07).
`edge_bias` (no golden carries one) is pinned to the f32 oracle's handling of it in the bidirectional mode, same 2e-6 bar
(measured 3.9e-07 on the logits), and to its definition in the single-direction modes: the logits move by the bias.
The training-mode dropout form (`dropout_mul`, no golden carries one either) is pinned to the f32 oracle given the same mask —
the kernel's own, p = 0.25 — on the toy golden at the same 2e-6 bar (measured 4.3e-07 on the edge embeddings, 1.5e-07 on the logits), and a mask of ones is
the eval-mode result bit for bit.
"""
import os
import types

import numpy as np
import pytest
import torch

from oracle import loss as oloss
from oracle import scorer as oscorer
from tests import scorer_f64 as f64

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
NAMES = ["retriever_toy", "retriever_mid", "retriever_fwd", "retriever_bwd"]
OUT_ATOL = 2e-6
GRAD_RTOL = 1e-5


def _load(name):
    z = np.load(os.path.join(GOLD, name + ".npz"), allow_pickle=False)
    batch = types.SimpleNamespace(**{k[2:]: z[k] for k in z.files if k.startswith("b_")})
    w = f64.leaf_weights({k[2:]: z[k] for k in z.files if k.startswith("w_")})
    rounds = z["rounds"].tolist()
    return z, batch, w, dict(num_rounds=rounds[0], num_reverse_rounds=rounds[1], direction_mode=str(z["direction"]))


@pytest.mark.parametrize("name", NAMES)
def test_float64_model_is_the_reference_to_f32_rounding(name):
    z, batch, w, kw = _load(name)
    out = f64.retriever_forward(w, batch, **kw)
    assert list(w) == [k for k in z["state_dict_keys"].tolist() if k != "parity_meta"]
    assert np.array_equal(out["query_ids"].numpy(), z["query_ids"])
    worst = {}
    for key in ("logits", "logits_fwd", "logits_bwd", "edge_embeddings", "node_struct"):
        if out[key] is None:
            assert z[key].size == 0, key  # the single-direction goldens store the other direction empty
            continue
        worst[key] = float(np.abs(out[key].detach().numpy() - z[key].astype(np.float64)).max())
    print(f"\n{name}: " + "  ".join(f"{k} {v:.1e}" for k, v in worst.items()))
    for key, err in worst.items():
        assert err <= OUT_ATOL, (key, err)

    (out["logits"] * torch.from_numpy(z["gvec"]).double()).sum().backward()
    ratios = {}
    for pname, p in w.items():
        want = z["g_" + pname]
        assert p.grad is not None and tuple(p.grad.shape) == want.shape, pname
        scale = max(float(np.abs(want).max()), 1e-6)
        ratios[pname] = float(np.abs(p.grad.numpy() - want.astype(np.float64)).max()) / scale
    assert len(ratios) == 25
    top = max(ratios, key=ratios.get)
    print(f"{name}: worst gradient {ratios[top]:.1e} of its max ({top})")
    for pname, r in ratios.items():
        assert r <= GRAD_RTOL, (pname, r)


@pytest.mark.parametrize("name", ["retriever_toy", "retriever_mid"])
@pytest.mark.parametrize("cfg", [dict(infonce_temperature=0.07), dict(infonce_temperature=0.5, bce_weight=0.3),
                                 dict(infonce_temperature=1.0, infonce_weight=0.5, bce_weight=1.0, edge_weight_near=2.0,
                                      edge_weight_bridge=0.5)], ids=["infonce", "infonce+bce", "weights"])
def test_float64_loss_is_the_loss_oracle_to_f32_rounding(name, cfg):
    z, batch, _, _ = _load(name)
    B = int(batch.ptr.shape[0] - 1)
    eb = np.searchsorted(batch.ptr[1:], batch.edge_index[0], side="right")
    near = (np.arange(eb.size) % 3 == 0)
    x = torch.from_numpy(z["logits"]).double().requires_grad_(True)
    total = f64.retriever_loss(x, batch.labels, eb, B, edge_is_near=near, **cfg)
    total.backward()
    want, _, _, want_grad = oloss.retriever_loss(z["logits"], batch.labels, eb, B, edge_is_near=near, **cfg)
    rel = abs(float(total.detach()) - want) / max(abs(want), 1e-6)
    gerr = float(np.abs(x.grad.numpy() - want_grad).max()) / max(float(np.abs(want_grad).max()), 1e-6)
    print(f"\n{name}: loss {float(total.detach()):.6f} rel {rel:.1e}  grad {gerr:.1e} of its max")
    assert want > 0
    assert rel <= 2e-6 and gerr <= 1e-5, (rel, gerr)


def test_float64_edge_bias_moves_both_directional_logits_before_the_combine():
    """The hide-and-seek penalty: added to both directional logits, then combined.  Bidirectional: against the f32 oracle given
    the same bias (the combine weights do not change, the combined logit moves by the bias); single direction: the logits are
    the unbiased ones plus the bias, the edge embeddings do not move."""
    z, batch, w, kw = _load("retriever_toy")
    rng = np.random.default_rng(0)
    bias = np.where(rng.random(z["logits"].size) < 0.5, -2.0, 0.0).astype(np.float32)
    got = f64.retriever_forward(w, batch, edge_bias=bias, **kw)
    want = oscorer.retriever_forward({k[2:]: z[k] for k in z.files if k.startswith("w_")}, batch, edge_bias=bias, **kw)
    worst = {k: float(np.abs(got[k].detach().numpy() - want[k]).max()) for k in ("logits", "logits_fwd", "logits_bwd", "edge_embeddings")}
    print("\nedge_bias vs the f32 oracle: " + "  ".join(f"{k} {v:.1e}" for k, v in worst.items()))
    assert max(worst.values()) <= OUT_ATOL, worst
    assert float(np.abs(got["logits"].detach().numpy() - bias - z["logits"]).max()) <= OUT_ATOL
    for name in ("retriever_fwd", "retriever_bwd"):
        z, batch, w, kw = _load(name)
        bias = np.linspace(-3.0, 0.0, z["logits"].size).astype(np.float32)
        plain = f64.retriever_forward(w, batch, **kw)
        moved = f64.retriever_forward(w, batch, edge_bias=bias, **kw)
        assert torch.allclose(moved["logits"], plain["logits"] + torch.from_numpy(bias).double(), rtol=0, atol=1e-12)
        assert torch.equal(moved["edge_embeddings"], plain["edge_embeddings"])


def test_float64_dropout_form_is_the_oracle_given_the_same_mask():
    """`retriever_forward(..., dropout_mul=)`: the [2, E, H] multipliers scale the GELU output of state_net per direction, where
    oracle/scorer.py: score_edges applies them.  The mask is the kernel's (p = 0.25, a quarter of the entries zero, the rest
    4 / 3); all four outputs against the f32 oracle given the same mask, at the eval-mode bar.  A mask of ones changes nothing,
    exactly; the real mask does."""
    z, batch, w, kw = _load("retriever_toy")
    E, H = int(z["logits"].size), int(z["H"])
    mul = f64._dropout_multipliers(0x1234567890ABCDEF, E, H, 0.25)
    assert mul.shape == (2, E, H) and set(np.unique(mul).tolist()) == {0.0, float(np.float32(4.0 / 3.0))}
    assert abs(float((mul > 0).mean()) - 0.75) < 0.02 and not np.array_equal(mul[0], mul[1])
    got = f64.retriever_forward(w, batch, dropout_mul=mul, **kw)
    want = oscorer.retriever_forward({k[2:]: z[k] for k in z.files if k.startswith("w_")}, batch, dropout_mul=mul, **kw)
    keys = ("logits", "logits_fwd", "logits_bwd", "edge_embeddings")
    worst = {k: float(np.abs(got[k].detach().numpy() - want[k]).max()) for k in keys}
    print("\ndropout_mul vs the f32 oracle: " + "  ".join(f"{k} {v:.1e}" for k, v in worst.items()))
    assert max(worst.values()) <= OUT_ATOL, worst
    plain = f64.retriever_forward(w, batch, **kw)
    ones = f64.retriever_forward(w, batch, dropout_mul=np.ones((2, E, H), np.float32), **kw)
    for k in keys:
        assert torch.equal(ones[k], plain[k]), k
    assert float((got["logits"] - plain["logits"]).detach().abs().max()) > 1e-3
    # a single-direction model reads the slice of its own direction: [0] forward, [1] backward
    for name, used, other in (("retriever_fwd", 0, 1), ("retriever_bwd", 1, 0)):
        z, batch, w, kw = _load(name)
        E, H = int(z["logits"].size), int(z["H"])
        mul = f64._dropout_multipliers(77, E, H, 0.25)
        got = f64.retriever_forward(w, batch, dropout_mul=mul, **kw)
        want = oscorer.retriever_forward({k[2:]: z[k] for k in z.files if k.startswith("w_")}, batch, dropout_mul=mul, **kw)
        assert float(np.abs(got["logits"].detach().numpy() - want["logits"]).max()) <= OUT_ATOL
        changed = mul.copy()
        changed[other] = 1.0
        again = f64.retriever_forward(w, batch, dropout_mul=changed, **kw)
        assert torch.equal(again["logits"], got["logits"]) and torch.equal(again["edge_embeddings"], got["edge_embeddings"])
        changed = mul.copy()
        changed[used] = 1.0
        assert not torch.equal(f64.retriever_forward(w, batch, dropout_mul=changed, **kw)["logits"], got["logits"])
