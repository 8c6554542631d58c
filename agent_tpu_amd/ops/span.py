"""Extractive question answering head on pair rows. Native: ``csrc/kernels/span_head.hip``.

``span_topk`` turns the last layer's rows of ``[CLS] question [SEP] passage [SEP]`` rows
(``ops.pair_assemble``) into start / end logits and the ``n`` best answer spans of each passage.

On the LayerNorm-folded encoder the last layer leaves raw rows ``g_j`` and their statistics
``fin = (rstd_j, rstd_j * mu_j)``; the span head is linear, so the LayerNorm folds into it:

    logit_c[j] = rstd_j * (g_j . u_c) - (rstd_j mu_j) * su_c + c_c
    u = gamma * W,  su = the row sums of u,  c = beta . W + b

Without ``fin`` the rows are already normalised and ``logit_c[j] = x_j . u_c + c_c`` (``u = W``,
``c = b``). ``len = clamp(lens[b], 2, S)``; positions ``>= len`` have logit ``-inf``, whatever the
rows hold.

Spans: ``lo`` = the first position with ``type_ids == 1`` (``S`` when there is none), ``hi = len - 2``;
the candidates are ``(i, j)`` with ``lo <= i <= j <= hi`` and ``j - i < max_len``, valued
``logit_0[i] + logit_1[j]`` (one fp32 add; a NaN ranks as ``-inf``), in the total order of
``group_topk``: value descending, then ``i * S + j`` ascending; ``+0.0`` and ``-0.0`` tie. Spans are
passage-relative ``(i - lo, j - lo)``; exhausted slots are ``(-1, -1)`` with ``-inf``.
``null[b] = logit_0[0] + logit_1[0]`` is the score of "no answer in this passage".

``own [B, 2]`` int32, optional (the window rows of ``ops.window_assemble``): row ``b`` proposes only the
spans whose start it owns, ``lo + clamp(own[b, 0], 0, S) <= i < lo + clamp(own[b, 1], 0, S)``; ends, order
and output are unchanged. Without it the launch is the one it always was.
"""
from __future__ import annotations

from typing import Optional, Tuple

import torch

from .._native import native, ptr, launch_stream
from ._util import check, check_bf16_dev, same_device

MAX_N = 32


def span_topk_ok(S: int, H: int) -> bool:
    """Shapes the kernel takes: 4..512 tokens, H a multiple of 64 from 64 to 1024."""
    return 4 <= S <= 512 and H % 64 == 0 and 64 <= H <= 1024


def span_logits_ref(x: torch.Tensor, lens: torch.Tensor, B: int, u: torch.Tensor, su: torch.Tensor, c: torch.Tensor,
                    fin: Optional[torch.Tensor] = None, dtype=torch.float32) -> torch.Tensor:
    """``logits [B, S, 2]`` of ``dtype`` by the kernel's formula in ``dtype`` math; ``-inf`` at positions
    ``>= len`` (selected with ``torch.where``, never by a multiply)."""
    H = x.shape[-1]
    S = x.numel() // (B * H)
    xx = x.to(dtype).view(B * S, H)
    d = xx @ u.to(dtype).t()  # [B*S, 2]
    if fin is not None:
        f = fin.to(dtype)
        lg = f[:, :1] * d - f[:, 1:] * su.to(dtype).view(1, 2) + c.to(dtype).view(1, 2)
    else:
        lg = d + c.to(dtype).view(1, 2)
    n = lens.reshape(-1)[:B].to(device=x.device, dtype=torch.int64).clamp(2, S)
    live = (torch.arange(S, device=x.device).view(1, S) < n.view(B, 1)).view(B, S, 1)
    return torch.where(live, lg.view(B, S, 2), torch.full((), float("-inf"), dtype=dtype, device=x.device))


def span_select_ref(logits: torch.Tensor, type_ids: torch.Tensor, lens: torch.Tensor, max_len: int,
                    n: int, own: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """The selection of the kernel on given fp32 ``logits [B, S, 2]`` -> ``(span [B, n, 2] int32,
    score [B, n] fp32, null [B] fp32)`` on the CPU. A stable descending sort of the candidates in id
    order gives (value desc, id asc). ``own [B, 2]``: the owned window-relative starts, see the module."""
    lg = logits.detach().float().cpu()
    B, S, _ = lg.shape
    ow = None if own is None else own.detach().cpu().view(-1, 2)[:B].to(torch.int64).clamp(0, S).tolist()
    types = type_ids.detach().cpu().view(-1, S)[:B]
    ln = lens.detach().cpu().reshape(-1)[:B].to(torch.int64).clamp(2, S).tolist()
    span = torch.full((B, n, 2), -1, dtype=torch.int32)
    score = torch.full((B, n), float("-inf"), dtype=torch.float32)
    null = lg[:, 0, 0] + lg[:, 0, 1]
    ar = torch.arange(S)
    ii, jj = ar.view(S, 1), ar.view(1, S)
    ninf = torch.full((), float("-inf"))
    for b in range(B):
        one = (types[b] == 1).nonzero()
        lo = int(one[0]) if one.numel() else S
        hi = ln[b] - 2
        ok = (ii >= lo) & (jj >= ii) & (jj <= hi) & (jj - ii < max_len)
        if ow is not None:
            ok = ok & (ii >= lo + ow[b][0]) & (ii < lo + ow[b][1])
        ids = ok.view(-1).nonzero().view(-1)  # ascending i * S + j
        if not ids.numel():
            continue
        v = (lg[b, :, 0].view(S, 1) + lg[b, :, 1].view(1, S)).view(-1)[ids]
        v = torch.where(torch.isnan(v), ninf, v)  # a NaN ranks as -inf
        order = torch.sort(v + 0.0, descending=True, stable=True).indices[:n]  # -0.0 + 0.0 = +0.0: they tie
        m = order.numel()
        pick = ids[order]
        span[b, :m, 0] = (pick // S - lo).to(torch.int32)
        span[b, :m, 1] = (pick % S - lo).to(torch.int32)
        score[b, :m] = v[order]
    return span, score, null


def span_topk_ref(x: torch.Tensor, lens: torch.Tensor, type_ids: torch.Tensor, B: int, u: torch.Tensor,
                  su: torch.Tensor, c: torch.Tensor, max_len: int, n: int, fin: Optional[torch.Tensor] = None,
                  own: Optional[torch.Tensor] = None
                  ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """PyTorch twin of the kernel -> ``(span, score, null, logits)`` on the CPU (also the CPU path)."""
    lg = span_logits_ref(x, lens, B, u, su, c, fin).float().cpu()
    return span_select_ref(lg, type_ids, lens, max_len, n, own) + (lg,)


def _out(t: Optional[torch.Tensor], shape, dtype, device, name: str) -> torch.Tensor:
    if t is None:
        return torch.empty(shape, dtype=dtype, device=device)
    check(t.dtype == dtype and t.is_contiguous() and t.dim() == len(shape) and t.shape[0] >= shape[0]
          and tuple(t.shape[1:]) == tuple(shape[1:]), f"span_topk: {name} must be contiguous {dtype} {list(shape)}")
    return t


def span_topk(x: torch.Tensor, lens: torch.Tensor, type_ids: torch.Tensor, B: int, u: torch.Tensor, su: torch.Tensor,
              c: torch.Tensor, max_len: int, n: int, fin: Optional[torch.Tensor] = None,
              span: Optional[torch.Tensor] = None, score: Optional[torch.Tensor] = None,
              null: Optional[torch.Tensor] = None, logits_out: Optional[torch.Tensor] = None,
              own: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """``(span [B, n, 2] int32, score [B, n] fp32, null [B] fp32)`` of the hidden rows ``x [B*S, H]`` (raw
    rows when ``fin [B*S, 2]`` is given, else normalised rows), ``lens [B]`` and ``type_ids [B, S]`` int32,
    the head ``u [2, H]``, ``su [2]``, ``c [2]`` fp32. Given outputs may hold more than ``B`` rows; rows
    past ``B`` are not touched. ``logits_out [B, S, 2]`` fp32, when given, receives the logits. ``own
    [>=B, 2]`` int32, when given, restricts every row's span starts to the range it owns."""
    check(isinstance(B, int) and B >= 0, "span_topk: B must be an int >= 0")
    check(x.dim() == 2 and (B == 0 or x.shape[0] % B == 0), "span_topk: x must be [B*S, H]")
    H = int(x.shape[1])
    check(type_ids.dim() == 2 and type_ids.shape[0] >= B, "span_topk: type_ids must be [B, S]")
    S = int(type_ids.shape[1])
    check(x.shape[0] == B * S, "span_topk: x must be [B*S, H]")
    check(isinstance(n, int) and not isinstance(n, bool) and 1 <= n <= MAX_N, "span_topk: n must be an int in [1, 32]")
    check(isinstance(max_len, int) and not isinstance(max_len, bool) and 1 <= max_len <= S,
          "span_topk: max_len must be an int in [1, S]")
    check(span_topk_ok(S, H), f"span_topk: unsupported shape S={S} H={H}")
    check(lens.numel() >= B, "span_topk: lens must hold B lengths")
    for t, name in ((lens, "lens"), (type_ids, "type_ids")):
        check(t.dtype == torch.int32 and t.is_contiguous(), f"span_topk: {name} must be contiguous int32")
    check(tuple(u.shape) == (2, H) and su.numel() == 2 and c.numel() == 2, "span_topk: u [2, H], su [2], c [2]")
    if fin is not None:
        check(tuple(fin.shape) == (B * S, 2) and fin.dtype == torch.float32, "span_topk: fin must be fp32 [B*S, 2]")
    if own is not None:
        check(own.dtype == torch.int32 and own.is_contiguous() and own.dim() == 2 and own.shape[1] == 2
              and own.shape[0] >= B, "span_topk: own must be contiguous int32 [B, 2]")
    same_device(x, fin, u, su, c, lens, type_ids, span, score, null, logits_out, own)
    dev = x.device
    span = _out(span, (B, n, 2), torch.int32, dev, "span")
    score = _out(score, (B, n), torch.float32, dev, "score")
    null = _out(null, (B,), torch.float32, dev, "null")
    if logits_out is not None:
        _out(logits_out, (B, S, 2), torch.float32, dev, "logits_out")
    if B == 0:
        return span, score, null
    if not x.is_cuda:
        sp, sc, nl, lg = span_topk_ref(x, lens, type_ids, B, u, su, c, max_len, n, fin, own)
        span[:B].copy_(sp), score[:B].copy_(sc), null[:B].copy_(nl)
        if logits_out is not None:
            logits_out[:B].copy_(lg)
        return span, score, null
    check_bf16_dev(x, "x")
    check(x.is_contiguous() and (fin is None or fin.is_contiguous()), "span_topk: contiguous tensors")
    for t, name in ((u, "u"), (su, "su"), (c, "c")):
        check(t.dtype == torch.float32 and t.is_contiguous(), f"span_topk: {name} must be contiguous fp32")
    native().span_topk(ptr(x), ptr(fin) if fin is not None else 0, ptr(u), ptr(su), ptr(c), ptr(type_ids), ptr(lens),
                       ptr(span), ptr(score), ptr(null), ptr(logits_out) if logits_out is not None else 0, B, S, H,
                       max_len, n, launch_stream(x), ptr(own) if own is not None else 0)
    return span, score, null
