"""MXFP8 linear layers on gfx950's block-scaled MFMA (evi_mx_* in libevi_hip.so): the opt-in fp8 encoder linears.

Format (include/evi_hip.h, restated on the CPU in tests/mx_oracle.py): blocks of 32 consecutive elements along K, one
e8m0 scale byte per block (e = max(-127, ceil(log2(amax / 448))), stored as e + 127), elements OCP e4m3fn(x * 2^-e).
The weight is quantised once when the layer is built; the activation is quantised inside the GEMM as it is staged.
Inference only; there is no CPU fallback.
"""
from __future__ import annotations

from typing import List, Optional, Tuple

import torch

from . import _lib, ops

_DTYPE_CODE = {torch.float32: 0, torch.float16: 1, torch.bfloat16: 2}
MX_BLOCK = 32


def _code(t: torch.Tensor, name: str) -> int:
    if t.dtype not in _DTYPE_CODE:
        raise ValueError(f"{name} must be float32, float16 or bfloat16, got {t.dtype}")
    return _DTYPE_CODE[t.dtype]


def _check_k(K: int) -> None:
    if K <= 0 or K % MX_BLOCK != 0:
        raise ValueError(f"MXFP8 needs K (the reduction dimension) to be a positive multiple of {MX_BLOCK}, got K={K}")


def _rows(x: torch.Tensor) -> torch.Tensor:
    """x as a 2-D view with unit column stride (copied only when the layout needs it)."""
    x2 = x.reshape(-1, x.shape[-1])
    if x2.stride(-1) != 1 or (x2.shape[0] > 1 and x2.stride(0) < x2.shape[1]):
        x2 = x2.contiguous()
    return x2


def mx_quantize(x: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """x [M, K] (f32 / bf16 / f16, on the device) -> (e4m3 bytes u8 [M, K], scale bytes u8 [M, K / 32])."""
    dev = ops._require_gpu(x)
    code = _code(x, "x")
    if x.dim() != 2:
        raise ValueError(f"x must be 2-D [M, K], got shape {tuple(x.shape)}")
    M, K = x.shape
    _check_k(K)
    x2 = _rows(x)
    q = torch.empty((M, K), dtype=torch.uint8, device=dev)
    s = torch.empty((M, K // MX_BLOCK), dtype=torch.uint8, device=dev)
    if M == 0:
        return q, s
    lib = _lib.load()
    _lib.check(lib.evi_mx_quantize_rows(ops._ptr(x2), code, M, K, x2.stride(0), ops._ptr(q), ops._ptr(s), ops._stream(dev)))
    return q, s


class MXWeight:
    """An nn.Linear weight [N, K] quantised along K and packed in the GEMM's load order (opaque bytes on the device)."""

    def __init__(self, weight: torch.Tensor):
        dev = ops._require_gpu(weight)
        code = _code(weight, "weight")
        if weight.dim() != 2:
            raise ValueError(f"weight must be 2-D [N, K], got shape {tuple(weight.shape)}")
        N, K = weight.shape
        _check_k(K)
        if N < 1:
            raise ValueError("weight must have at least one row")
        w = _rows(weight.detach())
        lib = _lib.load()
        self.packed = torch.empty(int(lib.evi_mx_pack_weight_bytes(N, K)), dtype=torch.uint8, device=dev)
        _lib.check(lib.evi_mx_pack_weight(ops._ptr(w), code, N, K, w.stride(0), ops._ptr(self.packed), ops._stream(dev)))
        self.N, self.K, self.source_dtype = int(N), int(K), weight.dtype

    @property
    def device(self) -> torch.device:
        return self.packed.device


def _out_dtype(x: torch.Tensor) -> torch.dtype:
    """nn.Linear's result dtype: the autocast dtype inside an enabled CUDA autocast region, else the input's."""
    if torch.is_autocast_enabled():
        get = getattr(torch, "get_autocast_dtype", None)
        return get("cuda") if get is not None else torch.get_autocast_gpu_dtype()
    return x.dtype


def mx_linear(x: torch.Tensor, w: MXWeight, bias: Optional[torch.Tensor] = None,
              out_dtype: Optional[torch.dtype] = None) -> torch.Tensor:
    """y = x W^T (+ bias) on the MXFP8 GEMM; x [..., K] f32 / bf16 / f16, bias f32 [N] or None."""
    dev = ops._require_gpu(x, bias, w.packed)
    code = _code(x, "x")
    if x.shape[-1] != w.K:
        raise ValueError(f"x has {x.shape[-1]} features, the weight expects K={w.K}")
    if out_dtype is None:
        out_dtype = _out_dtype(x)
    if out_dtype not in _DTYPE_CODE:
        raise ValueError(f"out_dtype must be float32, float16 or bfloat16, got {out_dtype}")
    if bias is not None:
        if bias.shape != (w.N,):
            raise ValueError(f"bias must be [{w.N}], got {tuple(bias.shape)}")
        bias = bias.detach().to(torch.float32).contiguous()
    lead = x.shape[:-1]
    x2 = _rows(x)
    M = x2.shape[0]
    y = torch.empty((M, w.N), dtype=out_dtype, device=dev)
    if M > 0:
        lib = _lib.load()
        _lib.check(lib.evi_mx_linear(ops._ptr(x2), code, M, w.K, x2.stride(0) if M > 1 else w.K, ops._ptr(w.packed), w.N,
                                     ops._ptr(bias), ops._ptr(y), _DTYPE_CODE[out_dtype], w.N, ops._stream(dev)))
    return y.reshape(*lead, w.N)


def mx_linear_strided(x: torch.Tensor, w: MXWeight, y: torch.Tensor, bias: Optional[torch.Tensor] = None) -> torch.Tensor:
    """As mx_linear into a caller's 2-D `y` whose rows may be padded (y.stride(0) >= N, unit column stride)."""
    dev = ops._require_gpu(x, y, bias, w.packed)
    code = _code(x, "x")
    if x.dim() != 2 or y.dim() != 2 or x.shape[1] != w.K or y.shape != (x.shape[0], w.N) or y.stride(1) != 1:
        raise ValueError("x must be [M, K] and y [M, N] with unit column stride")
    if x.stride(1) != 1:
        raise ValueError("x must have unit column stride")
    b = None if bias is None else bias.detach().to(torch.float32).contiguous()
    if x.shape[0] > 0:
        lib = _lib.load()
        _lib.check(lib.evi_mx_linear(ops._ptr(x), code, x.shape[0], w.K, max(x.stride(0), w.K), ops._ptr(w.packed), w.N,
                                     ops._ptr(b), ops._ptr(y), _code(y, "y"), max(y.stride(0), w.N), ops._stream(dev)))
    return y


class MXLinear(torch.nn.Module):
    """Inference-only stand-in for nn.Linear with MXFP8 operands (weight quantised once, bias kept as f32)."""

    def __init__(self, weight: MXWeight, bias: Optional[torch.Tensor]):
        super().__init__()
        self.weight_mx = weight
        self.in_features, self.out_features = weight.K, weight.N
        self.register_buffer("bias", None if bias is None else bias.detach().to(torch.float32).clone(), persistent=False)

    @classmethod
    def from_linear(cls, linear: torch.nn.Linear) -> "MXLinear":
        return cls(MXWeight(linear.weight.detach()), linear.bias)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        if torch.is_grad_enabled() and x.requires_grad:
            raise RuntimeError("MXLinear is inference-only (there is no backward): call it under torch.no_grad() "
                               "or on a tensor that does not require grad")
        return mx_linear(x, self.weight_mx, self.bias)

    def extra_repr(self) -> str:
        return f"in_features={self.in_features}, out_features={self.out_features}, bias={self.bias is not None}, format=mxfp8"


def swap_linears(module: torch.nn.Module) -> List[Tuple[torch.nn.Module, str, torch.nn.Linear]]:
    """Replace every nn.Linear with in_features % 32 == 0 inside `module` by an MXLinear, in place.  Returns the
    (parent, attribute name, original Linear) records that `restore_linears` takes to put the same objects back."""
    swapped: List[Tuple[torch.nn.Module, str, torch.nn.Linear]] = []
    for parent in list(module.modules()):
        for name, child in list(parent.named_children()):
            if isinstance(child, torch.nn.Linear) and child.in_features % MX_BLOCK == 0:
                setattr(parent, name, MXLinear.from_linear(child))
                swapped.append((parent, name, child))
    return swapped


def restore_linears(swapped: List[Tuple[torch.nn.Module, str, torch.nn.Linear]]) -> None:
    """Undo `swap_linears`: the original nn.Linear objects go back where they were."""
    for parent, name, child in reversed(swapped):
        setattr(parent, name, child)


__all__ = ["MX_BLOCK", "MXLinear", "MXWeight", "mx_linear", "mx_linear_strided", "mx_quantize", "restore_linears",
           "swap_linears"]
