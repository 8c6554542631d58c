"""Masked-token prediction ops. Native: ``csrc/kernels/fill.hip`` and ``csrc/kernels/mlm_head.hip``.

``fill_assemble``: ``[CLS] seg_0 [MASK] seg_1 ... seg_m [SEP]`` rows and the positions of their masks from
the single-segment rows of the pieces between a text's mask tokens (spec "atpu-fill v1" and pure-Python
twin: :func:`agent_tpu_amd.tokenizer.fill_rows`).

``mask_gather``: the encoder rows of the mask slots, ``xm[r] = x[mrow[r] * S + pos[mrow[r], mord[r]]]``. With
``fin [B*S, 2] = (rstd, rstd * mu)`` the rows are raw and the last LayerNorm is applied to the gathered
rows only: ``y = (x * rstd - rstd mu) * gamma + beta`` in fp32, rounded once to the row dtype. A slot whose
``mrow`` / ``mord`` / ``pos`` is out of range is invalid: zeros, ``valid[r] = 0``.

``vocab_topk``: ``logit[r, v] = t[r] . E[v] + bias[v]`` (``t`` fp32, ``E`` bf16 widened exactly, fp32
accumulation in a k order that depends on ``H`` alone, the bias added once at the end), its log-sum-exp
``lse[r] = max + log(sum exp(logit - max))`` over all ``V`` tokens and the top ``k`` in the total order (logit
descending, token id ascending). A NaN logit ranks and returns as ``-inf`` and adds 0 to the sum.
``prob = exp(logit - lse)`` (``lse_in[r]`` instead when given: the targets path normalises a gathered
table by the full vocabulary's lse). When ``k > V`` the tail is ``(-1, -inf, 0)``; an invalid slot returns
``(-1, -inf, 0)`` everywhere and ``lse = 0``. Every output of a slot has the same bits whatever ``R``, the
slot's index and the other slots (the header of ``mlm_head.hip`` says how). No ``[R, V]`` tensor is
written unless ``logits_out`` is given.
"""
from __future__ import annotations

import math
from typing import Optional, Tuple

import torch

from .._native import native, ptr, launch_stream
from .. import tokenizer as _tok
from ._util import check, check_bf16_dev, same_device

MAX_K = 32
MAX_MASKS = _tok.MAX_MASKS
NINF = float("-inf")


def _i32(t: torch.Tensor, name: str) -> None:
    check(isinstance(t, torch.Tensor) and t.dtype == torch.int32 and t.is_contiguous(),
          f"{name} must be a contiguous int32 tensor")


def vocab_topk_ok(H: int, V: int, k: int) -> bool:
    """Shapes the kernel takes: H a multiple of 64 from 64 to 1024, at least one token, k in 1..32."""
    return H % 64 == 0 and 64 <= H <= 1024 and V >= 1 and 1 <= k <= MAX_K


# --------------------------------------------------------------------------- fill_assemble
def fill_assemble_ref(ids_s, lens_s, segoff, max_masks: int, cls_id: int, sep_id: int, pad_id: int, mask_id: int,
                      rows: int) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """CPU reference: the twin on the first ``rows`` rows."""
    i, l, p = _tok.fill_rows(ids_s.numpy(), lens_s.numpy(), segoff.numpy()[:rows + 1], max_masks, cls_id, sep_id,
                             pad_id, mask_id)
    return torch.from_numpy(i), torch.from_numpy(l), torch.from_numpy(p)


def fill_assemble(ids_s: torch.Tensor, lens_s: torch.Tensor, segoff: torch.Tensor, max_masks: int,
                  cls_id: int = _tok.CLS_ID, sep_id: int = _tok.SEP_ID, pad_id: int = _tok.PAD_ID,
                  mask_id: int = _tok.MASK_ID, ids: Optional[torch.Tensor] = None,
                  lens: Optional[torch.Tensor] = None, pos: Optional[torch.Tensor] = None,
                  rows: Optional[int] = None) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """``(ids [B, S], lens [B], pos [B, M])`` int32 of the first ``rows`` (default: ``segoff.numel() - 1``) rows
    from the segment rows ``ids_s [Ns, S]`` / ``lens_s [Ns]`` and the offsets ``segoff [>= B + 1]`` (device data:
    clamped before use). ``M = max_masks`` in ``[1, 16]``. Rows past ``rows`` of given outputs are not touched."""
    for t, name in ((ids_s, "ids_s"), (lens_s, "lens_s"), (segoff, "segoff")):
        _i32(t, "fill_assemble: " + name)
    check(ids_s.dim() == 2 and lens_s.dim() == 1 and lens_s.numel() == ids_s.shape[0] and segoff.dim() == 1
          and segoff.numel() >= 1, "fill_assemble: ids_s [Ns, S], lens_s [Ns] and segoff [B + 1]")
    Ns, S = (int(v) for v in ids_s.shape)
    M = max_masks
    check(isinstance(M, int) and not isinstance(M, bool) and 1 <= M <= MAX_MASKS,
          "fill_assemble: max_masks must be an int in [1, 16]")
    B = int(segoff.numel() - 1 if rows is None else rows)
    check(S >= 3 and 0 <= B <= segoff.numel() - 1, "fill_assemble: S >= 3 and 0 <= rows <= segoff.numel() - 1")
    check(B == 0 or Ns >= 1, "fill_assemble: Ns must be >= 1")
    same_device(ids_s, lens_s, segoff, ids, lens, pos)
    given = [o is not None for o in (ids, lens, pos)]
    check(all(given) or not any(given), "fill_assemble: give ids, lens and pos together")
    if all(given):
        _i32(ids, "ids"), _i32(lens, "lens"), _i32(pos, "pos")
        check(ids.dim() == 2 and ids.shape[1] == S and ids.shape[0] >= B and lens.numel() >= B and pos.dim() == 2
              and pos.shape[1] == M and pos.shape[0] >= B, "fill_assemble: ids/lens/pos too small")
    if not ids_s.is_cuda:
        i, l, p = fill_assemble_ref(ids_s, lens_s, segoff, M, cls_id, sep_id, pad_id, mask_id, B)
        if ids is None:
            return i, l, p
        ids[:B].copy_(i), lens[:B].copy_(l), pos[:B].copy_(p)
        return ids, lens, pos
    if ids is None:
        ids = torch.empty((B, S), dtype=torch.int32, device=ids_s.device)
        lens = torch.empty((B,), dtype=torch.int32, device=ids_s.device)
        pos = torch.empty((B, M), dtype=torch.int32, device=ids_s.device)
    if B:
        native().fill_assemble(ptr(ids_s), ptr(lens_s), ptr(segoff), ptr(ids), ptr(lens), ptr(pos), B, Ns, S, M,
                               int(cls_id), int(sep_id), int(pad_id), int(mask_id), launch_stream(ids_s))
    return ids, lens, pos


# --------------------------------------------------------------------------- mask_gather
def mask_gather_ref(x: torch.Tensor, pos: torch.Tensor, mrow: torch.Tensor, mord: torch.Tensor, B: int, S: int,
                    fin: Optional[torch.Tensor] = None, gamma: Optional[torch.Tensor] = None,
                    beta: Optional[torch.Tensor] = None, dtype=torch.float32) -> Tuple[torch.Tensor, torch.Tensor]:
    """``(xm [R, H] of x's dtype, valid [R] int32)`` by the kernel's formula in ``dtype`` math; also the CPU path."""
    M = pos.shape[1]
    b, o = mrow.long(), mord.long()
    bc, oc = b.clamp(0, B - 1), o.clamp(0, M - 1)
    p = pos.view(-1, M)[bc, oc].long()
    ok = (b == bc) & (o == oc) & (p >= 0) & (p < S)
    row = bc * S + p.clamp(0, S - 1)
    y = x[row].to(dtype)
    if fin is not None:
        f = fin[row].to(dtype)
        y = (y * f[:, :1] - f[:, 1:]) * gamma.to(dtype).view(1, -1) + beta.to(dtype).view(1, -1)
    y = torch.where(ok.view(-1, 1), y, torch.zeros((), dtype=dtype, device=y.device))
    return y.to(x.dtype), ok.to(torch.int32)


def mask_gather(x: torch.Tensor, pos: torch.Tensor, mrow: torch.Tensor, mord: torch.Tensor, B: int, S: int,
                fin: Optional[torch.Tensor] = None, gamma: Optional[torch.Tensor] = None,
                beta: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """``(xm [R, H], valid [R] int32)`` of the encoder rows ``x [B*S, H]`` (raw rows when ``fin [B*S, 2]`` is
    given, with the fp32 ``gamma [H]`` / ``beta [H]`` of the LayerNorm that finishes them), the mask positions
    ``pos [>= B, M]`` int32 and the slots' ``mrow [R]`` / ``mord [R]`` int32."""
    check(isinstance(B, int) and isinstance(S, int) and B >= 0 and S >= 1, "mask_gather: B >= 0 and S >= 1 ints")
    check(x.dim() == 2 and x.shape[0] == B * S, "mask_gather: x must be [B*S, H]")
    H = int(x.shape[1])
    check(H % 64 == 0 and 64 <= H <= 1024, f"mask_gather: unsupported H={H}")
    for t, name in ((pos, "pos"), (mrow, "mrow"), (mord, "mord")):
        _i32(t, "mask_gather: " + name)
    check(pos.dim() == 2 and pos.shape[0] >= B and 1 <= pos.shape[1] <= MAX_MASKS, "mask_gather: pos must be [B, M]")
    check(mrow.dim() == 1 and mord.shape == mrow.shape, "mask_gather: mrow [R] and mord [R]")
    M, R = int(pos.shape[1]), int(mrow.numel())
    if fin is not None:
        check(tuple(fin.shape) == (B * S, 2) and fin.dtype == torch.float32, "mask_gather: fin must be fp32 [B*S, 2]")
        check(gamma is not None and beta is not None and gamma.numel() == H and beta.numel() == H,
              "mask_gather: fin needs gamma [H] and beta [H]")
    same_device(x, pos, mrow, mord, fin, gamma, beta)
    if R == 0 or B == 0:
        return (torch.zeros((R, H), dtype=x.dtype, device=x.device),
                torch.zeros((R,), dtype=torch.int32, device=x.device))
    if not x.is_cuda:
        return mask_gather_ref(x, pos[:B], mrow, mord, B, S, fin, gamma, beta)
    check_bf16_dev(x, "x")
    check(x.is_contiguous() and (fin is None or fin.is_contiguous()), "mask_gather: contiguous tensors")
    for t, name in ((gamma, "gamma"), (beta, "beta")):
        check(fin is None or (t.dtype == torch.float32 and t.is_contiguous()),
              f"mask_gather: {name} must be contiguous fp32")
    xm = torch.empty((R, H), dtype=x.dtype, device=x.device)
    valid = torch.empty((R,), dtype=torch.int32, device=x.device)
    opt = lambda t: ptr(t) if (t is not None and fin is not None) else 0  # noqa: E731
    native().mask_gather(ptr(x), opt(fin), opt(gamma), opt(beta), ptr(pos), ptr(mrow), ptr(mord), ptr(xm), ptr(valid),
                         R, B, S, M, H, launch_stream(x))
    return xm, valid


# --------------------------------------------------------------------------- vocab_topk
def vocab_logits_ref(t: torch.Tensor, E: torch.Tensor, bias: torch.Tensor, dtype=torch.float32) -> torch.Tensor:
    """``logits [R, V]`` of ``dtype`` by the kernel's formula in ``dtype`` math."""
    return t.to(dtype) @ E.to(dtype).t() + bias.to(dtype).view(1, -1)


def vocab_select_ref(logits: torch.Tensor, k: int, valid: Optional[torch.Tensor] = None,
                     lse_in: Optional[torch.Tensor] = None
                     ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """The selection of the kernel on given ``logits [R, V]`` -> ``(tok [R, k] int32, logit [R, k] fp32, prob
    [R, k] fp32, lse [R] fp32)`` on the CPU: a NaN ranks as ``-inf``, a stable descending sort gives the
    (logit desc, token asc) order (``+0.0`` and ``-0.0`` tie), the log-sum-exp and the probabilities in
    fp64, rounded once. Also the CPU path."""
    lg = logits.detach().float().cpu()
    R, V = lg.shape
    lg = torch.where(torch.isnan(lg), torch.full_like(lg, NINF), lg)
    tok = torch.full((R, k), -1, dtype=torch.int32)
    val = torch.full((R, k), NINF, dtype=torch.float32)
    prob = torch.zeros((R, k), dtype=torch.float32)
    lse = torch.zeros((R,), dtype=torch.float32)
    kk = min(k, V)
    order = torch.sort(lg + 0.0, dim=1, descending=True, stable=True).indices[:, :kk]
    tok[:, :kk] = order.to(torch.int32)
    val[:, :kk] = torch.gather(lg, 1, order)
    d = lg.double()
    m = d.max(dim=1, keepdim=True).values
    e = torch.where(d == m, torch.ones_like(d), torch.exp(d - m))
    e = torch.where(d == NINF, torch.zeros_like(d), e)
    own = torch.where(m.view(-1) == NINF, m.view(-1), m.view(-1) + torch.log(e.sum(1)))
    norm = own.float().double() if lse_in is None else lse_in.detach().cpu().double().view(-1)  # the fp32 lse
    pr = torch.exp(val.double() - norm.view(-1, 1))
    prob.copy_(torch.where(val == NINF, torch.zeros_like(pr), pr).float())
    lse.copy_(own.float())
    if valid is not None:
        bad = valid.detach().cpu().view(-1) == 0
        tok[bad], val[bad], prob[bad], lse[bad] = -1, NINF, 0.0, 0.0
    return tok, val, prob, lse


def vocab_topk(t: torch.Tensor, E: torch.Tensor, bias: torch.Tensor, k: int, valid: Optional[torch.Tensor] = None,
               lse_in: Optional[torch.Tensor] = None, logits_out: Optional[torch.Tensor] = None
               ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """``(tok [R, k] int32, logit [R, k], prob [R, k], lse [R])`` fp32 of the fp32 rows ``t [R, H]`` against the
    table ``E [V, H]`` (bf16 on the GPU) and the fp32 ``bias [V]``. ``valid [R]`` int32 (0: an invalid slot),
    ``lse_in [R]`` fp32 and ``logits_out [R, V]`` fp32 are optional."""
    check(t.dim() == 2 and E.dim() == 2 and E.shape[1] == t.shape[1], "vocab_topk: t [R, H] and E [V, H]")
    R, H = (int(v) for v in t.shape)
    V = int(E.shape[0])
    check(isinstance(k, int) and not isinstance(k, bool) and 1 <= k <= MAX_K, "vocab_topk: k must be an int in [1, 32]")
    check(vocab_topk_ok(H, V, k), f"vocab_topk: unsupported shape H={H} V={V}")
    check(bias.dim() == 1 and bias.numel() == V, "vocab_topk: bias must be [V]")
    if valid is not None:
        _i32(valid, "vocab_topk: valid")
        check(valid.numel() == R, "vocab_topk: valid must be [R]")
    if lse_in is not None:
        check(lse_in.dtype == torch.float32 and lse_in.is_contiguous() and lse_in.numel() == R,
              "vocab_topk: lse_in must be contiguous fp32 [R]")
    if logits_out is not None:
        check(logits_out.dtype == torch.float32 and logits_out.is_contiguous() and tuple(logits_out.shape) == (R, V),
              "vocab_topk: logits_out must be contiguous fp32 [R, V]")
    same_device(t, E, bias, valid, lse_in, logits_out)
    dev = t.device
    if not t.is_cuda:
        lg = vocab_logits_ref(t, E, bias).float()
        if logits_out is not None:
            logits_out.copy_(lg)
        return vocab_select_ref(lg, k, valid, lse_in)
    tok = torch.empty((R, k), dtype=torch.int32, device=dev)
    logit = torch.empty((R, k), dtype=torch.float32, device=dev)
    prob = torch.empty((R, k), dtype=torch.float32, device=dev)
    lse = torch.empty((R,), dtype=torch.float32, device=dev)
    if R == 0:
        return tok, logit, prob, lse
    check(t.dtype == torch.float32 and t.is_contiguous(), "vocab_topk: t must be contiguous fp32")
    check_bf16_dev(E, "E")
    check(E.is_contiguous() and bias.dtype == torch.float32 and bias.is_contiguous(),
          "vocab_topk: E must be contiguous bf16 and bias contiguous fp32")
    P = native().vocab_topk_splits(V)
    ws = torch.empty((R * P * (k + 1), 2), dtype=torch.float32, device=dev)  # [R, P, k] entries, then [R, P] pairs
    opt = lambda x: ptr(x) if x is not None else 0  # noqa: E731
    st = launch_stream(t)
    native().vocab_topk_partial(ptr(t), ptr(E), ptr(bias), ptr(ws), opt(logits_out), R, V, H, k, st)
    native().vocab_topk_merge(ptr(ws), opt(valid), opt(lse_in), ptr(tok), ptr(logit), ptr(prob), ptr(lse), R, V, k, st)
    return tok, logit, prob, lse


def vocab_topk_splits(V: int) -> int:
    """The number of vocabulary splits of ``vocab_topk``: ``ceil(ceil(V / 32) / 16)``, a function of ``V`` alone."""
    return math.ceil(math.ceil(V / 32) / 16)
