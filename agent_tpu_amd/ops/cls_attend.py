"""[CLS] attention of the last BERT layer without the all-token K / V projection.

When only the [CLS] row of the last layer is used, there is ONE query per (sequence, head),
and the K / V projection of all ``S`` keys can be moved onto the query and the result
(``x_j`` = LN2 of the previous layer, ``x_0`` its [CLS] row, head ``h``, ``scale = 1/sqrt(64)``):

* scores: ``q_h . (Wk_h x_j + bk_h) = (Wk_h^T q_h) . x_j + const``; the constant cancels in
  the softmax. With ``q_h = Wq_h x_0 + bq_h`` the projected query is linear in ``x_0``.
* context + out-projection: ``sum_h Wo[:, h] (Wv_h sum_j p_hj x_j + bv_h)`` (``sum_j p_hj = 1``).
* LayerNorm: ``x_j = gamma * (rstd_j g_j - rstd_j mu_j) + beta`` over the raw rows ``g_j``
  whose statistics the folded encoder keeps (``fin``); gamma goes into both weights, beta into
  the out bias; the ``u . beta`` score term is constant in ``j`` too.

:func:`cls_reassoc_weights` builds the two derived weights once per model,
:func:`cls_attend` is the kernel between them (``csrc/kernels/cls_attend.hip``):

    U  = linear(x_0, cls_wu, cls_bu)                       [B, heads*H]
    Z  = cls_attend(g, fin, U, lens)                       [B, heads*H]
    h1 = linear(Z, cls_wz, cls_bz, residual=x_0)           [B, H]

with ``Z[b, h] = sum_j p_hj xn_j``, ``xn_j = rstd_j g_j - rstd_j mu_j`` and ``p_h`` the softmax
over ``j < len`` of ``U_h . xn_j = rstd_j (U_h . g_j) - rstd_j mu_j sum(U_h)``.
"""
from __future__ import annotations

import math
from typing import Dict, Optional

import torch

from .._native import native, ptr, launch_stream
from ._util import check, check_bf16_dev, same_device
from .attention import HEAD_DIM

SEQ = 128


def cls_attend_ok(S: int, H: int, heads: int) -> bool:
    """Shapes the kernel takes: 128 tokens, H in {256, 512, 768, 1024}, heads of 64."""
    return S == SEQ and H % 256 == 0 and 256 <= H <= 1024 and 1 <= heads <= 16 and heads * HEAD_DIM == H


def cls_attend_ref(g: torch.Tensor, fin: torch.Tensor, U: torch.Tensor, lens: torch.Tensor, heads: int,
                   dtype=torch.float32, round_p: bool = True) -> torch.Tensor:
    """PyTorch twin of the kernel in ``dtype`` math -> ``[B, heads*H]`` of ``dtype``.

    ``round_p``: round the weights ``p_hj rstd_j`` (before normalisation) to bf16 as the
    kernel's MFMA operand is; the ``mu`` term is summed with the same rounded weights. Keys
    ``>= len`` contribute nothing, whatever their rows hold. ``lens`` is clamped to ``[1, S]``."""
    B = U.shape[0]
    H = g.shape[1]
    S = g.shape[0] // B
    gx = g.to(dtype).view(B, S, H)
    rstd = fin[:, 0].to(dtype).view(B, 1, S)
    rm = fin[:, 1].to(dtype).view(B, 1, S)
    Ux = U.to(dtype).view(B, heads, H)
    dead = (torch.arange(S, device=g.device).view(1, 1, S) >= lens.view(B, 1, 1).clamp(1, S).to(g.device))
    gx = gx.masked_fill(dead.view(B, S, 1), 0)
    sc = torch.einsum("bhn,bjn->bhj", Ux, gx) * rstd - rm * Ux.sum(-1, keepdim=True)
    sc = sc.masked_fill(dead, float("-inf"))
    e = torch.exp(sc - sc.amax(-1, keepdim=True))
    wgt = (e * rstd).masked_fill(dead, 0)
    if round_p:
        wgt = wgt.to(torch.bfloat16).to(dtype)
    mu = (rm / rstd).masked_fill(dead, 0)
    acc = torch.einsum("bhj,bjn->bhn", wgt, gx) - (wgt * mu).sum(-1, keepdim=True)
    return (acc / e.sum(-1, keepdim=True)).reshape(B, heads * H)


def cls_attend(g: torch.Tensor, fin: torch.Tensor, U: torch.Tensor, lens: torch.Tensor, heads: int,
               out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``Z [B, heads*H]`` from raw rows ``g [B*128, H]``, ``fin [B*128, 2]`` and queries ``U [B, heads*H]``."""
    check(g.dim() == 2 and U.dim() == 2, "cls_attend: g and U must be 2-D")
    M, H = g.shape
    B = U.shape[0]
    check(M == B * SEQ and U.shape[1] == heads * H, f"cls_attend: g must be [{B * SEQ}, H] and U [{B}, heads*H]")
    check(tuple(fin.shape) == (M, 2) and fin.dtype == torch.float32, "cls_attend: fin must be fp32 [M, 2]")
    check(lens.numel() >= B, "cls_attend: lens must hold B lengths")
    if not g.is_cuda:
        z = cls_attend_ref(g, fin, U, lens.reshape(-1)[:B], heads).to(g.dtype)
        return out.copy_(z) if out is not None else z
    check_bf16_dev(g, "g")
    check_bf16_dev(U, "U")
    same_device(g, fin, U, lens, out)
    check(cls_attend_ok(SEQ, H, heads), f"cls_attend: unsupported shape H={H} heads={heads}")
    check(g.is_contiguous() and U.is_contiguous() and fin.is_contiguous(), "cls_attend: contiguous tensors")
    check(lens.dtype == torch.int32 and lens.is_contiguous(), "cls_attend: lens must be contiguous int32")
    if out is None:
        out = torch.empty((B, heads * H), dtype=torch.bfloat16, device=g.device)
    check(out.dtype == torch.bfloat16 and tuple(out.shape) == (B, heads * H) and out.is_contiguous(),
          "cls_attend: out must be contiguous bf16 [B, heads*H]")
    native().cls_attend(ptr(g), ptr(fin), ptr(U), ptr(lens), ptr(out), B, SEQ, H, heads, launch_stream(g))
    return out


def cls_reassoc_weights(qkv_w: torch.Tensor, qkv_b: torch.Tensor, o_w: torch.Tensor, o_b: torch.Tensor,
                        gamma: torch.Tensor, beta: torch.Tensor, heads: int,
                        dtype=torch.bfloat16) -> Dict[str, torch.Tensor]:
    """The derived weights of the re-associated [CLS] layer (fp32 math where the inputs live).

    ``cls_wu [heads*H, H]``: rows ``h*H + n`` = ``scale * gamma_n * (Wk_h^T Wq_h)[n, :]``;
    ``cls_bu [heads*H]``     = ``scale * gamma * (Wk_h^T bq_h)``;
    ``cls_wz [H, heads*H]``: columns ``h*H + m`` = ``(Wo[:, h] Wv_h)[:, m] * gamma_m``;
    ``cls_bz [H]``           = ``bo + sum_h Wo[:, h] (Wv_h beta + bv_h)``.
    Products are broadcast-multiply + sum, not torch matmuls (no BLAS library start-up)."""
    H = o_w.shape[0]
    d = H // heads
    scale = 1.0 / math.sqrt(d)
    w, bq = qkv_w.float(), qkv_b.float()
    ga, be = gamma.float(), beta.float()
    wo = o_w.float()
    wu = torch.empty((heads * H, H), dtype=dtype, device=w.device)
    bu = torch.empty((heads * H,), dtype=torch.float32, device=w.device)
    wz = torch.empty((H, heads * H), dtype=dtype, device=w.device)
    bz = o_b.float().clone()
    for h in range(heads):
        wq, wk, wv = (w[t * H + h * d:t * H + (h + 1) * d] for t in range(3))  # [d, H] each
        bqh, bvh = bq[h * d:(h + 1) * d], bq[2 * H + h * d:2 * H + (h + 1) * d]
        woh = wo[:, h * d:(h + 1) * d]                                         # [H, d]
        kq = torch.zeros((H, H), dtype=torch.float32, device=w.device)        # [n, m] = sum_d wk[d, n] wq[d, m]
        ov = torch.zeros((H, H), dtype=torch.float32, device=w.device)        # [out, m] = sum_d wo[out, d] wv[d, m]
        for d0 in range(0, d, 8):  # 8 of the head's 64 dims at a time: [H, 8, H] fp32 temporaries
            kq += (wk[d0:d0 + 8].t().unsqueeze(2) * wq[d0:d0 + 8].unsqueeze(0)).sum(1)
            ov += (woh[:, d0:d0 + 8].unsqueeze(2) * wv[d0:d0 + 8].unsqueeze(0)).sum(1)
        wu[h * H:(h + 1) * H] = (kq * (scale * ga).unsqueeze(1)).to(dtype)
        bu[h * H:(h + 1) * H] = scale * ga * (wk * bqh.unsqueeze(1)).sum(0)
        wz[:, h * H:(h + 1) * H] = (ov * ga.unsqueeze(0)).to(dtype)
        bz += (woh * ((wv * be.unsqueeze(0)).sum(1) + bvh).unsqueeze(0)).sum(1)
    return {"cls_wu": wu, "cls_bu": bu.contiguous(), "cls_wz": wz, "cls_bz": bz.contiguous()}
