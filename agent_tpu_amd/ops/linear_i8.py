"""INT8 (W8A8) linear layer on the i8 MFMA GEMM.

Symmetric per-row quantisation, 127 levels, no zero points. Every scale operation is a single
IEEE fp32 operation, so the PyTorch twins below reproduce the kernels' ``q`` and ``scale`` bit
for bit and the int32 accumulators exactly::

    amax = max_k |x[r, k]|;  scale[r] = amax / 127;  inv = 127 / amax
    q[r, k] = clamp(rint(x[r, k] * inv), -127, 127)        (rint: half to even)
    an all-zero row: scale = 1, q = 0

    acc[m, n] = sum_k xq[m, k] * wq[n, k]                  (int32, exact for K <= 2^17)
    y = bf16(act(float(acc) * xs[m] * ws[n] + bias[n]) + residual[m, n])

Weights ``[N, K]`` are quantised by the same function over their rows (per output channel).
Native kernels: ``csrc/kernels/gemm_i8.hip``.
"""
from __future__ import annotations

from typing import Optional, Tuple

import torch
import torch.nn.functional as F

from .._native import native, ptr, launch_stream
from ._util import check, check_bf16_dev, row_stride, same_device
from .linear import EPI_BIAS, EPI_GELU, EPI_RESIDUAL
from .norm import layernorm

MAX_K = 1 << 17
_ACTS = {None: 0, "none": 0, "gelu": EPI_GELU}


def linear_i8_ok(M: int, N: int, K: int) -> bool:
    """Shapes :func:`linear_i8` takes (the kernel's ``gemm_i8_ok``): M >= 1, N % 16 == 0, K % 64 == 0."""
    return M >= 1 and N >= 16 and N % 16 == 0 and K >= 64 and K % 64 == 0 and K <= MAX_K


# ------------------------------------------------------------------ references (CPU oracle)
def quantize_rows_i8_ref(x: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """``(q int8 [rows, K], scale fp32 [rows])`` of a bf16 or fp32 ``x``; the kernel's arithmetic."""
    check(x.dim() == 2, "quantize_rows_i8: x must be 2-D")
    xf = x.float()
    amax = xf.abs().amax(dim=-1)
    any_ = amax > 0
    c127 = torch.full_like(amax, 127.0)
    safe = torch.where(any_, amax, torch.ones_like(amax))
    scale = torch.where(any_, amax / c127, torch.ones_like(amax))
    inv = torch.where(any_, c127 / safe, torch.zeros_like(amax))  # one division (never reciprocal * 127)
    q = torch.round(xf * inv.unsqueeze(-1)).clamp_(-127.0, 127.0).to(torch.int8)
    return q, scale


def linear_i8_ref(xq: torch.Tensor, xs: torch.Tensor, wq: torch.Tensor, ws: torch.Tensor,
                  bias: Optional[torch.Tensor] = None, act: Optional[str] = None,
                  residual: Optional[torch.Tensor] = None, raw: bool = False,
                  out_dtype: torch.dtype = torch.bfloat16) -> torch.Tensor:
    """int32 matmul, then the epilogue in fp32 in the kernel's order; ``raw``: the accumulators."""
    # the int32 matmul, carried in fp64 (BLAS; torch's integer matmul is a scalar loop): every partial
    # sum is an integer below 2^31 (K <= 2^17), far inside fp64's 2^53, so the result is exact
    acc = (xq.double() @ wq.double().t()).to(torch.int32)
    if raw:
        return acc
    y = acc.float() * xs.float().unsqueeze(-1)
    y = y * ws.float().unsqueeze(0)
    if bias is not None:
        y = y + bias.float()
    if act == "gelu":
        y = F.gelu(y)
    if residual is not None:
        y = y + residual.float()
    return y.to(out_dtype)


# ------------------------------------------------------------------ ops
def quantize_rows_i8(x: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """Per-row symmetric int8 quantisation: ``(q int8 [rows, K], scale fp32 [rows])``."""
    if not x.is_cuda:
        return quantize_rows_i8_ref(x)
    check_bf16_dev(x, "x")
    rows, K = x.shape
    check(rows >= 1 and K % 16 == 0 and K > 0, "quantize_rows_i8: K must be a positive multiple of 16")
    ldx = row_stride(x, "x")
    check(ldx % 8 == 0 and x.data_ptr() % 16 == 0, "quantize_rows_i8: x rows must be 16-B aligned")
    q = torch.empty((rows, K), dtype=torch.int8, device=x.device)
    scale = torch.empty((rows,), dtype=torch.float32, device=x.device)
    native().quantize_rows_i8(ptr(x), ldx, ptr(q), K, ptr(scale), rows, K, launch_stream(x))
    return q, scale


def linear_i8(xq: torch.Tensor, xs: torch.Tensor, wq: torch.Tensor, ws: torch.Tensor,
              bias: Optional[torch.Tensor] = None, act: Optional[str] = None,
              residual: Optional[torch.Tensor] = None, raw: bool = False,
              out_dtype: torch.dtype = torch.bfloat16) -> torch.Tensor:
    """``act(float(xq @ wq.T) * xs[:, None] * ws[None, :] + bias) + residual`` -> bf16 ``[M, N]``.

    ``raw=True`` returns the int32 accumulators ``[M, N]`` and applies nothing else.
    ``out_dtype`` is honoured by the CPU reference only (the fp32 oracle model); the kernel writes bf16."""
    check(act in _ACTS, f"linear_i8: unknown activation {act!r}")
    check(xq.dim() == 2 and wq.dim() == 2 and xq.dtype == torch.int8 and wq.dtype == torch.int8,
          "linear_i8: xq and wq must be 2-D int8")
    M, K = xq.shape
    N, K2 = wq.shape
    check(K == K2, f"inner dims differ: xq {tuple(xq.shape)} wq {tuple(wq.shape)}")
    check(K <= MAX_K, "linear_i8: K must be <= 2^17 (int32 accumulation)")
    check(xs.dtype == torch.float32 and xs.numel() == M and ws.dtype == torch.float32 and ws.numel() == N,
          "linear_i8: scales must be fp32 [M] and [N]")
    same_device(xq, xs, wq, ws, bias, residual)
    if not xq.is_cuda:
        return linear_i8_ref(xq, xs.reshape(-1), wq, ws.reshape(-1), bias, act, residual, raw, out_dtype)
    check(linear_i8_ok(M, N, K), f"linear_i8: unsupported shape M={M} N={N} K={K} (N % 16, K % 64)")
    check(out_dtype == torch.bfloat16, "linear_i8: the kernel writes bf16")
    lda, ldb = row_stride(xq, "xq"), row_stride(wq, "wq")
    check(lda % 16 == 0 and ldb % 16 == 0 and xq.data_ptr() % 16 == 0 and wq.data_ptr() % 16 == 0,
          "linear_i8: operand rows must be 16-B aligned")
    check(xs.is_contiguous() and ws.is_contiguous() and ws.data_ptr() % 16 == 0,
          "linear_i8: scales must be contiguous (ws 16-B aligned)")
    if raw:
        check(bias is None and residual is None and act in (None, "none"), "linear_i8: raw takes no epilogue")
        acc = torch.empty((M, N), dtype=torch.int32, device=xq.device)
        native().gemm_i8(ptr(xq), lda, ptr(xs), ptr(wq), ldb, ptr(ws), 0, 0, 0, 0, 0, M, N, K, 0, ptr(acc), N,
                         launch_stream(xq))
        return acc
    epi = _ACTS[act]
    if bias is not None:
        check(bias.dtype == torch.float32 and bias.is_contiguous() and bias.numel() == N
              and bias.data_ptr() % 16 == 0, "bias must be fp32 [N], 16-B aligned")
        epi |= EPI_BIAS
    ldr = 0
    if residual is not None:
        check_bf16_dev(residual, "residual")
        check(tuple(residual.shape) == (M, N), "residual must be [M, N]")
        ldr = row_stride(residual, "residual")
        check(ldr % 4 == 0 and residual.data_ptr() % 8 == 0, "residual rows must be 8-B aligned")
        epi |= EPI_RESIDUAL
    check(epi in (0, EPI_BIAS, EPI_BIAS | EPI_GELU, EPI_BIAS | EPI_RESIDUAL),
          "linear_i8: the kernel's epilogues are none, bias, bias + gelu, bias + residual")
    out = torch.empty((M, N), dtype=torch.bfloat16, device=xq.device)
    native().gemm_i8(ptr(xq), lda, ptr(xs), ptr(wq), ldb, ptr(ws), ptr(out), N, ptr(bias), ptr(residual), ldr, M, N, K,
                     epi, 0, 0, launch_stream(xq))
    return out


def layernorm_quant_i8(x: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, eps: float = 1e-12,
                       residual: Optional[torch.Tensor] = None
                       ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """``(y, q, scale)``: ``y = layernorm(x (+ residual))`` and ``(q, scale) = quantize_rows_i8(y)`` in one
    pass over the rows (bit for bit those two ops)."""
    if not x.is_cuda:
        y = layernorm(x, gamma, beta, eps, residual=residual)
        return (y,) + quantize_rows_i8_ref(y)
    check_bf16_dev(x, "x")
    rows, N = x.shape
    check(x.is_contiguous(), "x must be contiguous")
    check(N % 256 == 0 and N <= 2048, "row width must be a multiple of 256, <= 2048")
    for t, n in ((gamma, "gamma"), (beta, "beta")):
        check(t.dtype == torch.float32 and t.is_contiguous() and t.numel() == N, f"{n} must be fp32 [{N}]")
    if residual is not None:
        check_bf16_dev(residual, "residual")
        check(residual.is_contiguous() and residual.shape == x.shape, "residual must match x")
    same_device(x, gamma, beta, residual)
    y = torch.empty_like(x)
    q = torch.empty((rows, N), dtype=torch.int8, device=x.device)
    scale = torch.empty((rows,), dtype=torch.float32, device=x.device)
    native().layernorm_quant_i8(ptr(x), ptr(residual), ptr(gamma), ptr(beta), ptr(y), ptr(q), ptr(scale), rows, N,
                                float(eps), launch_stream(x))
    return y, q, scale
