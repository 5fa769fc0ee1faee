"""MXFP8 format: self-checks of the CPU restatement (tests/mx_oracle.py) and the host-side refusals of evi_mx_*."""
import numpy as np
import pytest
import torch

from evi_rag_amd import _lib
from tests import mx_oracle as O


def _blocks(rng, M=64, K=256):
    x = rng.standard_normal((M, K)).astype(np.float32) * np.exp2(rng.integers(-40, 40, (M, 1))).astype(np.float32)
    x[3, :32] = 0.0
    return x


def test_scale_rule_puts_block_maxima_in_224_448():
    rng = np.random.default_rng(0)
    x = _blocks(rng)
    x[5, 32:64] = 448.0 * 2.0 ** 7  # amax exactly 448 * 2^e
    x[6, :32] = np.float32(3.4e38)
    q, s = O.quantize(x)
    amax = np.abs(x.reshape(64, -1, 32)).max(axis=2).astype(np.float64)
    e = s.astype(np.int64) - 127
    ratio = amax / np.ldexp(1.0, e)
    ok = (ratio > 224) & (ratio <= 448) | (e == -127)
    assert ok.all()
    assert s[3, 0] == 0 and (q[3, :32] == 0).all()
    assert s[5, 1] == 127 + 7 and ratio[5, 1] == 448.0
    assert O.e4m3_value(int(q[5, 32:64][np.argmax(np.abs(x[5, 32:64]))])) == 448.0


def test_powers_of_two_and_small_integers_are_exact():
    x = np.zeros((2, 64), np.float32)
    x[0, :32] = np.arange(-16, 16)
    x[1, :32] = np.exp2(np.arange(-16, 16))
    x[1, 32:] = -np.exp2(np.arange(0, 32) - 150).astype(np.float32)  # f32 subnormals and small normals
    assert np.array_equal(O.fake_quant(x)[0, :32], x[0, :32].astype(np.float64))
    # powers of two within e4m3's range of the block's scale (2^-6 .. 2^8 times the scale, and subnormals down to 2^-9)
    got = O.fake_quant(x)[1, :32]
    e = int(O.quantize(x)[1][1, 0]) - 127
    keep = x[1, :32] >= np.ldexp(1.0, e - 9)
    assert np.array_equal(got[keep], x[1, :32][keep].astype(np.float64))


def test_round_to_nearest_even_ties():
    # block amax 448 -> e = 0; 1 + 1/16 lies halfway between 1 and 1.125 (ties to 1, even); 1 + 3/16 ties to 1.25
    x = np.zeros((1, 32), np.float32)
    x[0, :4] = [448.0, 1.0625, 1.1875, -1.0625]
    got = O.fake_quant(x)[0, :4]
    assert list(got) == [448.0, 1.0, 1.25, -1.0]


def test_e4m3_subnormals():
    x = np.zeros((1, 32), np.float32)
    # e = 0 (amax 448): 2^-9 is the smallest subnormal; 3 * 2^-10 ties between 2^-9 and 2^-8 -> 2^-8 (code 2, even)
    x[0, :5] = [448.0, 2.0 ** -9, 3 * 2.0 ** -10, 2.0 ** -11, 5 * 2.0 ** -9]
    q, s = O.quantize(x)
    assert s[0, 0] == 127
    assert list(q[0, 1:5]) == [1, 2, 0, 5]
    assert list(O.fake_quant(x)[0, 1:5]) == [2.0 ** -9, 2.0 ** -8, 0.0, 5 * 2.0 ** -9]


def test_k_not_multiple_of_32_is_refused_with_k_in_message():
    lib = _lib.load()
    for fn, args in ((lib.evi_mx_linear, (None, 0, 4, 48, 48, None, 8, None, None, 0, 8, None)),
                     (lib.evi_mx_quantize_rows, (None, 0, 4, 48, 48, None, None, None)),
                     (lib.evi_mx_pack_weight, (None, 0, 8, 48, 48, None, None))):
        rc = fn(*args)
        assert rc == _lib.EVI_ERR_INVALID
        assert "K=48" in _lib.last_error()
    assert lib.evi_mx_pack_weight_bytes(8, 48) == 0 and lib.evi_mx_pack_weight_bytes(8, 64) > 0
    from evi_rag_amd import mx

    with pytest.raises(ValueError, match="K=48"):
        mx._check_k(48)


def test_unsupported_dtype_is_refused():
    lib = _lib.load()
    assert lib.evi_mx_linear(None, 3, 4, 64, 64, None, 8, None, None, 0, 8, None) == _lib.EVI_ERR_INVALID
    assert lib.evi_mx_linear(None, 0, 4, 64, 64, None, 8, None, None, 7, 8, None) == _lib.EVI_ERR_INVALID
    assert lib.evi_mx_quantize_rows(None, 5, 4, 64, 64, None, None, None) == _lib.EVI_ERR_INVALID
    from evi_rag_amd import mx

    with pytest.raises(ValueError, match="float32, float16 or bfloat16"):
        mx._code(torch.zeros(2, 32, dtype=torch.float64), "x")


def test_cpu_tensors_are_refused():
    from evi_rag_amd import mx

    with pytest.raises(RuntimeError, match="no CPU fallback"):
        mx.mx_quantize(torch.zeros(2, 64))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        mx.MXWeight(torch.zeros(8, 64))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        mx.MXLinear.from_linear(torch.nn.Linear(64, 8))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        mx.swap_linears(torch.nn.Sequential(torch.nn.Linear(64, 8)))
