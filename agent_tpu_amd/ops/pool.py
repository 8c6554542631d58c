"""Sentence embedding from the encoder's hidden rows: pooling on the device.

``pool_embed`` (``csrc/kernels/pool_embed.hip``) turns the last layer's rows into one fp32 vector
per sequence: the mean over the real tokens ``j < len`` (``mode="mean"``) or row 0 (``"cls"``),
optionally divided by ``max(||e||_2, 1e-12)`` (``F.normalize``'s definition).

On the LayerNorm-folded encoder the last layer leaves raw rows ``g_j`` and their statistics
``fin = (rstd_j, rstd_j * mu_j)``. The mean commutes with the LayerNorm that would finish them:

    mean_{j<len} LN(g_j)[n] = gamma[n] * (sum_j rstd_j g_j[n] - sum_j rstd_j mu_j) / len + beta[n]

so with ``fin`` the kernel reads each real token row once and no ``[B*S, H]`` tensor is written;
without ``fin`` the rows are already normalised and ``out = sum_j x_j / len``. ``S = 1`` is how a
``[B, H]`` tensor of [CLS] states is normalised. Rows ``>= len`` contribute nothing, whatever they
hold; ``len`` is clamped to ``[1, S]``.
"""
from __future__ import annotations

from typing import Optional

import torch

from .._native import native, ptr, launch_stream
from ._util import check, check_bf16_dev, same_device

MODES = {"mean": 0, "cls": 1}
EPS = 1e-12


def pool_embed_ok(S: int, H: int) -> bool:
    """Shapes the kernel takes: 1..512 tokens, H a multiple of 64 from 64 to 1024."""
    return 1 <= S <= 512 and H % 64 == 0 and 64 <= H <= 1024


def pool_embed_ref(x: torch.Tensor, lens: torch.Tensor, B: int, fin: Optional[torch.Tensor] = None,
                   gamma: Optional[torch.Tensor] = None, beta: Optional[torch.Tensor] = None, mode: str = "mean",
                   normalize: bool = True, dtype=torch.float32) -> torch.Tensor:
    """PyTorch twin of the kernel in ``dtype`` math -> ``[B, H]`` of ``dtype`` (also the CPU path).

    Rows ``>= len`` are discarded by select (``torch.where``), never by a multiply."""
    check(mode in MODES, f"pool_embed: mode must be one of {sorted(MODES)}")
    H = x.shape[-1]
    S = x.numel() // (B * H)
    xx = x.to(dtype).view(B, S, H)
    n = (torch.ones(B, dtype=torch.int64, device=x.device) if mode == "cls"
         else lens.reshape(-1)[:B].to(device=x.device, dtype=torch.int64).clamp(1, S))
    live = (torch.arange(S, device=x.device).view(1, S) < n.view(B, 1)).view(B, S, 1)
    zero = torch.zeros((), dtype=dtype, device=x.device)
    cnt = n.to(dtype).view(B, 1)
    if fin is not None:
        check(gamma is not None and beta is not None, "pool_embed: fin needs gamma and beta")
        rstd = torch.where(live, fin[:, 0].to(dtype).view(B, S, 1), zero)
        rm = torch.where(live, fin[:, 1].to(dtype).view(B, S, 1), zero)
        a = (torch.where(live, xx, zero) * rstd).sum(1) - rm.sum(1)
        e = gamma.to(dtype).view(1, H) * a / cnt + beta.to(dtype).view(1, H)
    else:
        e = torch.where(live, xx, zero).sum(1) / cnt
    if normalize:
        e = e / e.norm(dim=1, keepdim=True).clamp_min(EPS)
    return e


def pool_embed(x: torch.Tensor, lens: torch.Tensor, B: int, fin: Optional[torch.Tensor] = None,
               gamma: Optional[torch.Tensor] = None, beta: Optional[torch.Tensor] = None, mode: str = "mean",
               normalize: bool = True, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``[B, H]`` fp32 embeddings of the hidden rows ``x [B*S, H]`` (raw rows when ``fin [B*S, 2]``,
    ``gamma`` and ``beta`` are given, else normalised rows) with lengths ``lens [B]``."""
    check(mode in MODES, f"pool_embed: mode must be one of {sorted(MODES)}")
    check(x.dim() == 2 and B > 0 and x.shape[0] % B == 0, "pool_embed: x must be [B*S, H]")
    M, H = x.shape
    S = M // B
    check(lens.numel() >= B, "pool_embed: lens must hold B lengths")
    if fin is not None:
        check(tuple(fin.shape) == (M, 2) and fin.dtype == torch.float32, "pool_embed: fin must be fp32 [M, 2]")
        check(gamma is not None and beta is not None, "pool_embed: fin needs gamma and beta")
    if not x.is_cuda:
        e = pool_embed_ref(x, lens, B, fin, gamma, beta, mode, normalize).to(torch.float32)
        return out.copy_(e) if out is not None else e
    check_bf16_dev(x, "x")
    same_device(x, fin, gamma, beta, lens, out)
    check(pool_embed_ok(S, H), f"pool_embed: unsupported shape S={S} H={H}")
    check(x.is_contiguous() and (fin is None or fin.is_contiguous()), "pool_embed: contiguous tensors")
    check(lens.dtype == torch.int32 and lens.is_contiguous(), "pool_embed: lens must be contiguous int32")
    if fin is not None:
        for t, name in ((gamma, "gamma"), (beta, "beta")):
            check(t.dtype == torch.float32 and t.numel() == H and t.is_contiguous(),
                  f"pool_embed: {name} must be contiguous fp32 [H]")
    if out is None:
        out = torch.empty((B, H), dtype=torch.float32, device=x.device)
    check(out.dtype == torch.float32 and tuple(out.shape) == (B, H) and out.is_contiguous(),
          "pool_embed: out must be contiguous fp32 [B, H]")
    native().pool_embed(ptr(x), ptr(fin) if fin is not None else 0, ptr(gamma) if fin is not None else 0,
                        ptr(beta) if fin is not None else 0, ptr(lens), ptr(out), B, S, H, MODES[mode],
                        1 if normalize else 0, launch_stream(x))
    return out
