"""Learned sparse (SPLADE) term weights. Native: ``csrc/kernels/sparse_head.hip``.

``term_max``: ``xmax[b, v] = max over i < lens[b] of t[b * S + i] . E[v]``, the vocabulary product of every
live token of every text reduced per text (``t [B*S, H]`` and ``E [V, H]`` bf16 on the GPU, fp32
accumulation in a k order that depends on ``H`` alone). ``-inf`` for an empty text. Rows of padding tokens are
never read. No ``[B*S, V]`` tensor is written.

``term_select``: ``x = xmax + bias`` (adding the bias after the maximum is exact: fp32 rounding is monotone);
the terms of a text are the entries with ``x > 0`` (NaN and ``-inf`` give none), ``nnz`` their number, and
the best ``k <= 1024`` of them come back in the total order (``x`` descending, token id ascending) as
``tok`` / ``xs`` / ``w = log1p(xs)``; slots past the list hold ``(-1, 0, 0)``.
"""
from __future__ import annotations

from typing import Tuple

import torch

from .._native import native, ptr, launch_stream
from ._util import check, check_bf16_dev, same_device

MAX_TERMS = 1024
NINF = float("-inf")


def term_max_ok(H: int, S: int, V: int, B: int) -> bool:
    """Shapes the kernel takes: H a multiple of 64 from 64 to 1024, rows of 1 to 512 tokens."""
    return H % 64 == 0 and 64 <= H <= 1024 and 1 <= S <= 512 and V >= 1 and B >= 1


def term_max_ref(t: torch.Tensor, lens: torch.Tensor, E: torch.Tensor, S: int, dtype=torch.float32) -> torch.Tensor:
    """``xmax [B, V]`` by the kernel's formula in ``dtype`` math, one text at a time; also the CPU path."""
    B, V = int(lens.numel()), int(E.shape[0])
    out = torch.full((B, V), NINF, dtype=dtype, device=t.device)
    Et = E.to(dtype).t()
    for b in range(B):
        n = min(max(int(lens[b]), 0), S)
        if n:
            out[b] = (t[b * S:b * S + n].to(dtype) @ Et).amax(0)
    return out


def term_max(t: torch.Tensor, lens: torch.Tensor, E: torch.Tensor, S: int, vocab_tile: int = 0) -> torch.Tensor:
    """``xmax [B, V]`` fp32 of the token rows ``t [B*S, H]`` (text ``b`` at rows ``b*S .. b*S+S-1``), ``lens [B]``
    int32 and the table ``E [V, H]``. ``vocab_tile``: 64 or 32 table rows per workgroup (0: the default); the
    bits do not depend on it."""
    check(t.dim() == 2 and E.dim() == 2 and E.shape[1] == t.shape[1], "term_max: t [B*S, H] and E [V, H]")
    check(isinstance(lens, torch.Tensor) and lens.dtype == torch.int32 and lens.dim() == 1 and lens.is_contiguous(),
          "term_max: lens must be a contiguous int32 [B]")
    check(isinstance(S, int) and not isinstance(S, bool), "term_max: S must be an int")
    B, H, V = int(lens.numel()), int(t.shape[1]), int(E.shape[0])
    check(term_max_ok(H, S, V, B), f"term_max: unsupported shape H={H} S={S} V={V} B={B}")
    check(t.shape[0] == B * S, "term_max: t must have B*S rows")
    check(vocab_tile in (0, 32, 64), "term_max: vocab_tile must be 0, 32 or 64")
    same_device(t, lens, E)
    if not t.is_cuda:
        return term_max_ref(t, lens, E, S).float()
    check_bf16_dev(t, "t")
    check_bf16_dev(E, "E")
    check(t.is_contiguous() and E.is_contiguous(), "term_max: t and E must be contiguous")
    xmax = torch.empty((B, V), dtype=torch.float32, device=t.device)
    native().term_max(ptr(t), ptr(lens), ptr(E), ptr(xmax), B, S, V, H, vocab_tile, launch_stream(t))
    return xmax


def term_select_ref(xmax: torch.Tensor, bias: torch.Tensor, k: int
                    ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """The kernel's selection on the CPU -> ``(tok [B, k] int32, xs [B, k], w [B, k] fp32, nnz [B] int32)``: the fp32
    add, the entries with ``x > 0``, a stable descending sort for the total order (a row already ascends by
    token, so the sort by token is the identity and only the one by ``x`` is run), ``log1p`` in fp64 rounded
    once. Also the CPU path."""
    x = xmax.detach().float().cpu() + bias.detach().float().cpu().view(1, -1)
    B, V = x.shape
    pos = x > 0  # NaN compares false
    key = torch.where(pos, x, torch.full_like(x, NINF))
    kk = min(k, V)
    order = torch.sort(key, dim=1, descending=True, stable=True).indices[:, :kk]
    val = torch.gather(key, 1, order)
    got = val > 0
    tok = torch.full((B, k), -1, dtype=torch.int32)
    xs = torch.zeros((B, k), dtype=torch.float32)
    w = torch.zeros((B, k), dtype=torch.float32)
    tok[:, :kk] = torch.where(got, order.to(torch.int32), torch.full_like(order, -1, dtype=torch.int32))
    xs[:, :kk] = torch.where(got, val, torch.zeros_like(val))
    w[:, :kk] = torch.log1p(xs[:, :kk].double()).float()
    return tok, xs, w, pos.sum(1).to(torch.int32)


def term_select(xmax: torch.Tensor, bias: torch.Tensor, k: int
                ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """``(tok [B, k] int32, xs [B, k], w [B, k] fp32, nnz [B] int32)`` of ``xmax [B, V]`` and ``bias [V]`` fp32."""
    check(isinstance(k, int) and not isinstance(k, bool) and 1 <= k <= MAX_TERMS,
          "term_select: k must be an int in [1, 1024]")
    check(xmax.dim() == 2 and xmax.shape[0] >= 1 and xmax.shape[1] >= 1, "term_select: xmax must be [B, V]")
    B, V = (int(v) for v in xmax.shape)
    check(bias.dim() == 1 and bias.numel() == V, "term_select: bias must be [V]")
    same_device(xmax, bias)
    if not xmax.is_cuda:
        return term_select_ref(xmax, bias, k)
    check(xmax.dtype == torch.float32 and xmax.is_contiguous() and bias.dtype == torch.float32
          and bias.is_contiguous(), "term_select: xmax and bias must be contiguous fp32")
    dev = xmax.device
    tok = torch.empty((B, k), dtype=torch.int32, device=dev)
    xs = torch.empty((B, k), dtype=torch.float32, device=dev)
    w = torch.empty((B, k), dtype=torch.float32, device=dev)
    nnz = torch.empty((B,), dtype=torch.int32, device=dev)
    native().term_select(ptr(xmax), ptr(bias), ptr(tok), ptr(xs), ptr(w), ptr(nnz), B, V, k, launch_stream(xmax))
    return tok, xs, w, nnz
