"""MXFP8 linear on the MI355X: the quantiser bit for bit, the MFMA lane maps with exact integers, the GEMM against the
dequantised-operand oracle, capture, non-finite blocks, MXLinear and the TextEncoder option end to end."""
import numpy as np
import pytest
import torch

from tests import mx_oracle as O

pytestmark = pytest.mark.gpu

DT = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}


def _special_rows(K=256):
    rng = np.random.default_rng(1)
    x = (rng.standard_normal((12, K)) * np.exp2(rng.integers(-20, 20, (12, K // 32)).repeat(32, axis=1))).astype(np.float32)
    x[0, :32] = 0.0                                            # all-zero block
    x[1, :32] = 0.5
    x[1, 5] = 448.0 * 2.0 ** -3                                # amax exactly 448 * 2^e
    x[2, :32] = 2.0 ** -9 * np.arange(32) / 4                  # e4m3 subnormals after scaling
    x[2, 31] = 448.0
    x[3, :8] = [448.0, 1.0625, 1.1875, -1.0625, 2.0 ** -9 * 1.5, 2.0 ** -9 * 2.5, 3 * 2.0 ** -10, -5 * 2.0 ** -10]  # RNE ties
    x[4, :32] = np.float32(3.0e38) * np.linspace(-1, 1, 32).astype(np.float32)  # amax near the f32 maximum
    x[5, :32] = np.arange(32, dtype=np.float32) * np.float32(1e-45)            # f32 subnormals
    x[6, 32:64] = np.float32(1.17e-38) * np.linspace(-3, 3, 32).astype(np.float32)
    return x


@pytest.mark.parametrize("dtype", ["f32", "bf16", "f16"])
def test_quantizer_bit_exact(dev, dtype):
    from evi_rag_amd import mx

    x = torch.from_numpy(_special_rows()).to(DT[dtype])
    if dtype == "f16":
        x = torch.from_numpy(_special_rows() / np.float32(1e34)).clamp(-6e4, 6e4).to(torch.float16)
        x[0, :32] = 0
    rng = np.random.default_rng(2)
    big = torch.from_numpy(rng.standard_normal((333, 512)).astype(np.float32)).to(DT[dtype])
    for t in (x, big):
        q, s = mx.mx_quantize(t.to(dev))
        q_ref, s_ref = O.quantize(t)
        assert np.array_equal(s.cpu().numpy(), s_ref)
        assert np.array_equal(q.cpu().numpy(), q_ref)
    # a strided input (ldx > K) quantises the same
    wide = torch.zeros((big.shape[0], 544), dtype=big.dtype)
    wide[:, :512] = big
    q2, s2 = mx.mx_quantize(wide.to(dev)[:, :512])
    assert np.array_equal(q2.cpu().numpy(), O.quantize(big)[0]) and np.array_equal(s2.cpu().numpy(), O.quantize(big)[1])


def test_lane_maps_exact_integers(dev):
    """Small integers with distinct power-of-two block scales, asymmetric W: the result is the exact integer product."""
    from evi_rag_amd import mx

    rng = np.random.default_rng(3)
    M, K, N = 70, 384, 200
    # integers in [-15, 15] times a power of two per block, and every block holds a +-15: its amax is 15 * 2^s, so its scale is
    # exactly 2^(s - 4) and every element is an exact e4m3 value (j * 16, four significant bits) under it
    ex = rng.integers(-2, 2, (M, K // 32)).astype(np.float64)
    ew = rng.integers(-2, 2, (N, K // 32)).astype(np.float64)
    a = rng.integers(-15, 16, (M, K)).astype(np.float64)
    w = rng.integers(-15, 16, (N, K)).astype(np.float64)
    a[:, ::32] = 15.0
    w[:, 1::32] = -15.0
    w[:N // 2, 2::32] = 0.0  # asymmetric
    x = a * np.exp2(ex).repeat(32, axis=1)
    wf = w * np.exp2(ew).repeat(32, axis=1)
    assert np.array_equal(O.fake_quant(x.astype(np.float32)), x) and np.array_equal(O.fake_quant(wf.astype(np.float32)), wf)
    assert len(np.unique(O.quantize(x.astype(np.float32))[1])) == 4
    ref = x @ wf.T
    assert (np.abs(x) @ np.abs(wf).T).max() < 2 ** 20  # every partial sum is a multiple of 2^-4 below 2^20: exact in f32
    wt = mx.MXWeight(torch.from_numpy(wf.astype(np.float32)).to(dev))
    y = mx.mx_linear(torch.from_numpy(x.astype(np.float32)).to(dev), wt, out_dtype=torch.float32)
    assert np.array_equal(y.cpu().numpy().astype(np.float64), ref)


# Accumulation bound.  The block-scaled MFMA does not add its 128 products at full f32 precision inside one instruction:
# against the f64 product of the dequantised operands it was measured (this file, K = 96 .. 4 096) up to ~3e-5 of
# sum_k |a_k w_k| — about 2^-15, where a k-ordered f32 fma chain stays near 1e-7.  The bound is 1e-4 of that sum: still
# four orders of magnitude below what a wrong lane map or a wrong scale gives (O(1) of it).
ACC_REL = 1e-4


def _check(y, y_ref, mag, out_dtype):
    y = y.float().cpu().numpy().astype(np.float64)
    tol = ACC_REL * mag + 2.0 ** -22 * np.abs(y_ref)
    if out_dtype == torch.bfloat16:
        tol = tol + 2.0 ** -8 * np.abs(y_ref)
    bad = np.abs(y - y_ref) > tol
    assert not bad.any(), f"{bad.sum()} of {bad.size} outside tolerance; worst {np.max(np.abs(y - y_ref) - tol)}"
    if out_dtype == torch.float32:
        print(f"worst |y - y_ref| / sum|a w|: {np.max(np.abs(y - y_ref) / np.maximum(mag, 1e-30)):.3e}")


@pytest.mark.parametrize("KN", [(96, 200), (128, 1), (384, 1536), (768, 3072), (1024, 1024), (1024, 4096), (4096, 1024)])
def test_linear_against_dequantized_oracle(dev, KN):
    from evi_rag_amd import mx

    K, N = KN
    rng = np.random.default_rng(K + N)
    w = (rng.standard_normal((N, K)) / np.sqrt(K)).astype(np.float32)
    bias = rng.standard_normal(N).astype(np.float32)
    wt = mx.MXWeight(torch.from_numpy(w).to(dev))
    cases = [(1, "f32", torch.float32, True), (17, "bf16", torch.bfloat16, False), (640, "f16", torch.float32, True),
             (2051, "bf16", torch.bfloat16, True)]
    for M, xd, od, with_bias in cases:
        x = torch.from_numpy(rng.standard_normal((M, K)).astype(np.float32)).to(DT[xd])
        y_ref, mag = O.linear(x, w, bias if with_bias else None)
        y = mx.mx_linear(x.to(dev), wt, torch.from_numpy(bias).to(dev) if with_bias else None, out_dtype=od)
        assert y.dtype == od and y.shape == (M, N)
        _check(y, y_ref, mag, od)
    # ldx > K and ldy > N
    M = 333
    xw = torch.from_numpy(rng.standard_normal((M, K + 64)).astype(np.float32)).to(dev)
    yw = torch.full((M, N + 24), 7.0, device=dev)
    mx.mx_linear_strided(xw[:, :K], wt, yw[:, :N], torch.from_numpy(bias).to(dev))
    y_ref, mag = O.linear(xw[:, :K].cpu(), w, bias)
    _check(yw[:, :N], y_ref, mag, torch.float32)
    assert torch.all(yw[:, N:] == 7.0)


def test_fused_equals_standalone(dev):
    from evi_rag_amd import mx

    rng = np.random.default_rng(5)
    K, N = 768, 1000
    w = torch.from_numpy(rng.standard_normal((N, K)).astype(np.float32)).to(dev)
    wt = mx.MXWeight(w)
    for dt in (torch.float32, torch.bfloat16, torch.float16):
        x = torch.from_numpy(rng.standard_normal((517, K)).astype(np.float32) * 3).to(dev).to(dt)
        q, s = mx.mx_quantize(x)
        xd = torch.from_numpy(O.dequantize(q.cpu().numpy(), s.cpu().numpy()).astype(np.float32)).to(dev)
        assert torch.equal(mx.mx_linear(x, wt, out_dtype=torch.float32), mx.mx_linear(xd, wt, out_dtype=torch.float32))


def test_determinism_capture_and_empty(dev):
    from evi_rag_amd import mx

    rng = np.random.default_rng(6)
    wt = mx.MXWeight(torch.from_numpy(rng.standard_normal((1024, 1024)).astype(np.float32)).to(dev))
    bias = torch.randn(1024, device=dev)
    x = torch.from_numpy(rng.standard_normal((1500, 1024)).astype(np.float32)).to(dev).bfloat16()
    a = mx.mx_linear(x, wt, bias)
    assert torch.equal(a, mx.mx_linear(x, wt, bias))
    static = x.clone()
    s = torch.cuda.Stream(dev)
    s.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(s):
        mx.mx_linear(static, wt, bias)
    torch.cuda.current_stream(dev).wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = mx.mx_linear(static, wt, bias)
    g.replay()
    torch.cuda.synchronize(dev)
    assert torch.equal(out, a)
    e = mx.mx_linear(torch.empty((0, 1024), device=dev), wt)
    assert e.shape == (0, 1024)
    assert mx.mx_linear(torch.empty((2, 0, 1024), device=dev), wt).shape == (2, 0, 1024)


def test_non_finite_blocks_poison_exactly_their_outputs(dev):
    from evi_rag_amd import mx

    rng = np.random.default_rng(7)
    K, N, M = 256, 300, 200
    w = rng.standard_normal((N, K)).astype(np.float32)
    w[37, 100] = np.inf
    wt = mx.MXWeight(torch.from_numpy(w).to(dev))
    x = rng.standard_normal((M, K)).astype(np.float32)
    x[5, 70] = np.nan
    x[150, 255] = -np.inf
    y = mx.mx_linear(torch.from_numpy(x).to(dev), wt, out_dtype=torch.float32).cpu().numpy()
    nan = np.isnan(y)
    expect = np.zeros_like(nan)
    expect[[5, 150], :] = True
    expect[:, 37] = True
    assert np.array_equal(nan, expect)
    clean_x, clean_w = x.copy(), w.copy()
    clean_x[[5, 150]] = 0
    clean_w[37] = 0
    y_ref, mag = O.linear(clean_x, clean_w)
    keep = ~expect
    assert np.all(np.abs(y[keep] - y_ref[keep]) <= ACC_REL * mag[keep] + 2.0 ** -22 * np.abs(y_ref[keep]))


def test_mxlinear_against_nn_linear(dev):
    from evi_rag_amd import mx

    torch.manual_seed(0)
    for K, N in ((1024, 4096), (4096, 1024)):
        lin = torch.nn.Linear(K, N).to(dev)
        m = mx.MXLinear.from_linear(lin)
        x = torch.randn(2048, K, device=dev)
        x[:, :8] *= 20  # outlier channels
        with torch.no_grad():
            y = m(x)
            ref = (x.double() @ lin.weight.double().T + lin.bias.double())
        err = float((y.double() - ref).norm() / ref.norm())
        assert err <= 0.05, err
        assert y.dtype == torch.float32
        with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
            assert m(x).dtype == torch.bfloat16 and lin(x).dtype == torch.bfloat16
        with torch.no_grad():
            assert m(x.half()).dtype == torch.float16
    xg = torch.randn(4, 1024, device=dev, requires_grad=True)
    with pytest.raises(RuntimeError, match="inference-only"):
        m = mx.MXLinear.from_linear(torch.nn.Linear(1024, 64).to(dev))
        m(xg)
    with torch.no_grad():
        m(xg)


def _bert(dev, hidden=128, layers=2):
    transformers = pytest.importorskip("transformers")
    torch.manual_seed(0)
    return transformers.BertModel(transformers.BertConfig(vocab_size=1000, hidden_size=hidden, num_hidden_layers=layers,
                                                          num_attention_heads=4, intermediate_size=4 * hidden,
                                                          max_position_embeddings=64), add_pooling_layer=False).to(dev).eval()


class _Tok:
    def __call__(self, texts, padding=True, truncation=True, return_tensors="pt"):
        lens = [3 + (len(t) * 7) % 20 for t in texts]
        L = max(lens)
        g = torch.Generator().manual_seed(sum(map(len, texts)))
        mask = (torch.arange(L).view(1, L) < torch.tensor(lens).view(-1, 1)).to(torch.int64)
        ids = torch.randint(1, 1000, (len(texts), L), generator=g) * mask
        return {"input_ids": ids, "attention_mask": mask, "token_type_ids": torch.zeros_like(ids)}


class _FakeQuantLinear(torch.nn.Module):
    def __init__(self, lin):
        super().__init__()
        self.w = O.fake_quant(lin.weight.detach().cpu())
        self.b = None if lin.bias is None else lin.bias.detach().cpu().double().numpy()

    def forward(self, x):
        x2 = x.reshape(-1, x.shape[-1])
        y = O.fake_quant(x2.float()) @ self.w.T
        if self.b is not None:
            y = y + self.b
        return torch.from_numpy(y.astype(np.float32)).reshape(*x.shape[:-1], -1)


def test_text_encoder_mxfp8_end_to_end(dev, tmp_path):
    import copy

    from evi_rag_amd import text_encode as T

    model = _bert(dev)
    texts = ["q" * (1 + (i * 5) % 23) for i in range(40)]
    plain = T.TextEncoder.from_components(_Tok(), copy.deepcopy(model), str(dev), fp16=False)
    plain.use_graphs = False
    ref32 = plain.encode_to_device(texts, 8)

    originals = [mod for mod in model.modules() if isinstance(mod, torch.nn.Linear)]
    enc = T.TextEncoder.from_components(_Tok(), model, str(dev), fp16=False, precision="mxfp8")
    assert enc.precision == "mxfp8"
    from evi_rag_amd.mx import MXLinear

    assert not any(isinstance(mod, torch.nn.Linear) for mod in model.modules())
    assert sum(isinstance(mod, MXLinear) for mod in model.modules()) == len(originals)
    enc.use_graphs = False
    eager = enc.encode_to_device(texts, 8)

    # CPU run of the same model with the oracle's fake-quant linears (f32 elsewhere, as on the device)
    cpu_model = copy.deepcopy(plain.model).cpu()
    for parent in list(cpu_model.modules()):
        for name, child in list(parent.named_children()):
            if isinstance(child, torch.nn.Linear):
                setattr(parent, name, _FakeQuantLinear(child))
    cpu_enc = T.TextEncoder.from_components(_Tok(), cpu_model, "cpu", fp16=False)
    rows = []
    for b in range(0, len(texts), 8):
        inp = _Tok()(texts[b:b + 8])
        with torch.no_grad():
            h = cpu_model(**inp).last_hidden_state
        m = inp["attention_mask"].unsqueeze(-1).float()
        rows.append((h * m).sum(1) / m.sum(1).clamp(min=1e-6))
    ref_fq = torch.cat(rows).numpy()
    got = eager.cpu().numpy()
    rel = np.linalg.norm(got - ref_fq, axis=1) / np.linalg.norm(ref_fq, axis=1)
    # Tolerance from measurement: the device and the CPU restatement quantise the same values except where upstream f32
    # arithmetic (attention, LayerNorm, GELU: different summation orders) moves an activation across an e4m3 rounding
    # boundary; each such flip changes one element by one e4m3 step (2^-3 relative) and the error it causes is diluted
    # over the rest of the network.  Measured per-row relative differences stay well below 1e-2; an error in layout or
    # scaling gives O(1).
    print(f"max per-row rel difference to the fake-quant CPU encoder: {rel.max():.3e}")
    assert rel.max() < 2e-2, rel.max()
    rel32 = np.linalg.norm(got - ref32.cpu().numpy(), axis=1) / np.linalg.norm(ref32.cpu().numpy(), axis=1)
    assert rel32.max() > 1e-3  # the swap happened

    enc.use_graphs = True
    enc.encode_to_device(texts, 8)  # captures
    replay = enc.encode_to_device(texts, 8)
    assert len(enc._graphs) > 0 and torch.equal(replay, eager)
    enc.autocast = torch.bfloat16
    bf = enc.encode_to_device(texts, 8)
    assert torch.isfinite(bf).all()
    enc.autocast = None

    ent, rel_t = T.encode_tables(enc, entity_embedding_records=[{"embedding_id": i + 1, "label": t} for i, t in enumerate(texts[:10])],
                                 entity_struct_records=[{"embedding_id": i} for i in range(12)],
                                 relation_records=[{"relation_id": i, "label": t} for i, t in enumerate(texts[:5])], batch_size=4,
                                 embeddings_out_dir=tmp_path)
    assert ent.shape == (12, 128) and rel_t.shape == (5, 128) and torch.isfinite(ent).all()

    enc.set_precision(None)
    assert enc.precision is None and not enc.__dict__.get("_graphs")
    back = [mod for mod in model.modules() if isinstance(mod, torch.nn.Linear)]
    assert len(back) == len(originals) and all(a is b for a, b in zip(back, originals))
    enc.use_graphs = False
    assert torch.equal(enc.encode_to_device(texts, 8), ref32)
