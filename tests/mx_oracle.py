"""CPU restatement of the MXFP8 format of evi_mx_* (include/evi_hip.h): quantise, dequantise, fake-quant linear.

Blocks of 32 consecutive K elements per row.  e = max(-127, ceil(log2(amax / 448))) from the exact f32 bits (e = -127 for
an all-zero block), scale byte e + 127, elements e4m3fn(x * 2^-e) with round to nearest even (torch's cast)."""
from __future__ import annotations

import numpy as np
import torch

BLOCK = 32


def scale_exponents(amax: np.ndarray) -> np.ndarray:
    """e per block from amax (f32, >= 0, finite)."""
    bits = np.ascontiguousarray(amax, dtype=np.float32).view(np.uint32)
    biased = (bits >> 23).astype(np.int64)
    mant = bits & 0x7FFFFF
    e = np.where(mant > 0x600000, biased - 127 - 7, biased - 127 - 8)
    e = np.where(biased == 0, -127, e)
    return np.maximum(e, -127)


def quantize(x) -> tuple:
    """x [M, K] (f32 / bf16 / f16 tensor or array, finite) -> (e4m3 bytes u8 [M, K], scale bytes u8 [M, K / 32])."""
    xt = torch.as_tensor(x).to(torch.float32).cpu()
    M, K = xt.shape
    assert K % BLOCK == 0, K
    xb = xt.numpy().reshape(M, K // BLOCK, BLOCK)
    amax = np.abs(xb).max(axis=2) if M else np.zeros((0, K // BLOCK), np.float32)
    e = scale_exponents(amax.astype(np.float32))
    mul = np.ldexp(np.float32(1.0), -e).astype(np.float32)  # exact powers of two
    scaled = torch.from_numpy((xb * mul[:, :, None]).astype(np.float32).reshape(M, K))
    q = scaled.to(torch.float8_e4m3fn).view(torch.uint8).numpy()
    return q, (e + 127).astype(np.uint8)


def dequantize(q: np.ndarray, s: np.ndarray) -> np.ndarray:
    """(e4m3 bytes, scale bytes) -> f64 values."""
    M, K = q.shape
    v = torch.from_numpy(np.ascontiguousarray(q)).view(torch.float8_e4m3fn).to(torch.float64).numpy()
    scale = np.ldexp(1.0, s.astype(np.int64) - 127)
    return (v.reshape(M, K // BLOCK, BLOCK) * scale[:, :, None]).reshape(M, K)


def fake_quant(x) -> np.ndarray:
    return dequantize(*quantize(x))


def linear(x, w, bias=None) -> tuple:
    """Fake-quant linear: both operands quantised and dequantised, multiplied in f64.  Returns (y, sum_k |a_k w_k|)."""
    a, b = fake_quant(x), fake_quant(w)
    y = a @ b.T
    if bias is not None:
        y = y + np.asarray(torch.as_tensor(bias).to(torch.float64).cpu())[None, :]
    return y, np.abs(a) @ np.abs(b).T


def e4m3_value(code: int) -> float:
    return float(torch.tensor([code], dtype=torch.uint8).view(torch.float8_e4m3fn).to(torch.float64)[0])
