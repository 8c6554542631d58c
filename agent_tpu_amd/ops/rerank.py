"""Cross-encoder re-ranker ops. Native: ``csrc/kernels/rerank.hip``.

``pair_assemble``: ``[CLS] query [SEP] passage [SEP]`` rows with their ``type_ids`` from the
single-segment rows the tokenizers emit (spec "atpu-pair v1" and pure-Python twin:
:func:`agent_tpu_amd.tokenizer.pair_rows`). The launch allocates nothing when the outputs are
given and never synchronizes, so it can be captured into a graph.

``group_topk``: the top ``k`` of every query's own candidates, ``scores [P]`` grouped by the
offsets ``goff [Q + 1]``, in the total order of ``sim_topk`` and ``head_topk`` (score descending,
index ascending; ``+0.0`` and ``-0.0`` tie). ``sim_topk`` leaves a NaN score undefined (``better()``
is false both ways); here a NaN ranks as ``-inf`` and is returned as ``-inf``, so the order stays
total. A group shorter than ``k`` is padded with ``(-inf, -1)``.
"""
from __future__ import annotations

from typing import Optional, Tuple

import torch

from .._native import native, ptr, launch_stream
from .. import tokenizer as _tok
from ._util import check, same_device

MAX_K = 32


def _i32(t: torch.Tensor, name: str) -> None:
    check(isinstance(t, torch.Tensor) and t.dtype == torch.int32 and t.is_contiguous(),
          f"{name} must be a contiguous int32 tensor")


def pair_assemble_ref(ids_q, lens_q, ids_p, lens_p, qidx, max_query_tokens: int, cls_id: int, sep_id: int,
                      pad_id: int, rows: int) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """CPU reference: the twin on the first ``rows`` passage rows."""
    i, t, l = _tok.pair_rows(ids_q.numpy(), lens_q.numpy(), ids_p.numpy()[:rows], lens_p.numpy()[:rows],
                             qidx.numpy()[:rows], max_query_tokens, cls_id, sep_id, pad_id)
    return torch.from_numpy(i), torch.from_numpy(t), torch.from_numpy(l)


def pair_assemble(ids_q: torch.Tensor, lens_q: torch.Tensor, ids_p: torch.Tensor, lens_p: torch.Tensor,
                  qidx: torch.Tensor, max_query_tokens: int, cls_id: int = _tok.CLS_ID, sep_id: int = _tok.SEP_ID,
                  pad_id: int = _tok.PAD_ID, ids: Optional[torch.Tensor] = None,
                  type_ids: Optional[torch.Tensor] = None, lens: Optional[torch.Tensor] = None,
                  rows: Optional[int] = None) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """``(ids [P, S], type_ids [P, S], lens [P])`` int32 of the first ``rows`` (default: all) passage
    rows ``ids_p [>=P, S]`` / ``lens_p`` paired with the query rows ``ids_q [Q, S]`` / ``lens_q [Q]`` that
    ``qidx [>=P]`` names (clamped into ``[0, Q)``). Rows past ``rows`` of given outputs are not touched."""
    for t, name in ((ids_q, "ids_q"), (lens_q, "lens_q"), (ids_p, "ids_p"), (lens_p, "lens_p"), (qidx, "qidx")):
        _i32(t, name)
    check(ids_q.dim() == 2 and ids_p.dim() == 2 and ids_q.shape[1] == ids_p.shape[1],
          "pair_assemble: ids_q [Q, S] and ids_p [P, S]")
    Q, S = ids_q.shape
    P = int(ids_p.shape[0] if rows is None else rows)
    check(isinstance(max_query_tokens, int) and not isinstance(max_query_tokens, bool) and max_query_tokens >= 0,
          "pair_assemble: max_query_tokens must be an int >= 0")
    check(S >= 4 and Q >= 1 and P >= 0, "pair_assemble: S >= 4, Q >= 1, P >= 0")
    check(lens_q.numel() == Q, "pair_assemble: lens_q must be [Q]")
    check(ids_p.shape[0] >= P and lens_p.numel() >= P and qidx.numel() >= P, "pair_assemble: ids_p/lens_p/qidx too small")
    same_device(ids_q, lens_q, ids_p, lens_p, qidx, ids, type_ids, lens)
    given = [o is not None for o in (ids, type_ids, lens)]
    check(all(given) or not any(given), "pair_assemble: give ids, type_ids and lens together")
    if all(given):
        _i32(ids, "ids"), _i32(type_ids, "type_ids"), _i32(lens, "lens")
        check(ids.dim() == 2 and ids.shape[1] == S and type_ids.shape == ids.shape and ids.shape[0] >= P
              and lens.numel() >= P, "pair_assemble: ids/type_ids/lens too small")
    if not ids_q.is_cuda:
        i, t, l = pair_assemble_ref(ids_q, lens_q, ids_p, lens_p, qidx, max_query_tokens, cls_id, sep_id, pad_id, P)
        if ids is None:
            return i, t, l
        ids[:P].copy_(i), type_ids[:P].copy_(t), lens[:P].copy_(l)
        return ids, type_ids, lens
    if ids is None:
        ids = torch.empty((P, S), dtype=torch.int32, device=ids_q.device)
        type_ids = torch.empty((P, S), dtype=torch.int32, device=ids_q.device)
        lens = torch.empty((P,), dtype=torch.int32, device=ids_q.device)
    if P:
        native().pair_assemble(ptr(ids_q), ptr(lens_q), ptr(ids_p), ptr(lens_p), ptr(qidx), ptr(ids), ptr(type_ids),
                               ptr(lens), P, Q, S, max_query_tokens, int(cls_id), int(sep_id), int(pad_id),
                               launch_stream(ids_q))
    return ids, type_ids, lens


def group_topk_ref(scores: torch.Tensor, goff: torch.Tensor, k: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """PyTorch twin -> (idx ``[Q, k]`` int32, val ``[Q, k]`` fp32); also the CPU path. A stable descending
    sort gives the (score desc, index asc) order (``torch.topk`` promises no tie order)."""
    P = scores.numel()
    Q = goff.numel() - 1
    idx = torch.full((Q, k), -1, dtype=torch.int32)
    val = torch.full((Q, k), float("-inf"), dtype=torch.float32)
    off = goff.tolist()
    for q in range(Q):
        a = min(max(off[q], 0), P)
        b = max(min(max(off[q + 1], 0), P), a)
        s = scores[a:b].float().cpu()
        s = torch.where(torch.isnan(s), torch.full_like(s, float("-inf")), s)  # a NaN ranks as -inf
        order = torch.sort(s + 0.0, descending=True, stable=True).indices[:k]  # -0.0 + 0.0 = +0.0: they tie
        idx[q, :order.numel()] = order.to(torch.int32)
        val[q, :order.numel()] = s[order]
    return idx, val


def group_topk(scores: torch.Tensor, goff: torch.Tensor, k: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """(idx ``[Q, k]`` int32: the index within the group, val ``[Q, k]`` fp32) of the contiguous fp32
    ``scores [P]`` grouped by the contiguous int32 offsets ``goff [Q + 1]`` (non-decreasing, ``goff[0] = 0``,
    ``goff[Q] = P``; clamped into ``[0, P]`` before use). ``k`` in 1..32."""
    check(isinstance(scores, torch.Tensor) and scores.dtype == torch.float32 and scores.dim() == 1
          and scores.is_contiguous(), "group_topk: scores must be a contiguous fp32 [P]")
    _i32(goff, "group_topk: goff")
    check(goff.dim() == 1 and goff.numel() >= 1, "group_topk: goff must be [Q + 1]")
    check(isinstance(k, int) and not isinstance(k, bool) and 1 <= k <= MAX_K, "group_topk: k must be an int in [1, 32]")
    same_device(scores, goff)
    P, Q = scores.numel(), goff.numel() - 1
    if not scores.is_cuda:
        return group_topk_ref(scores, goff, k)
    idx = torch.empty((Q, k), dtype=torch.int32, device=scores.device)
    val = torch.empty((Q, k), dtype=torch.float32, device=scores.device)
    if P == 0:  # nothing to rank: every group is empty
        return idx.fill_(-1), val.fill_(float("-inf"))
    if Q:
        native().group_topk(ptr(scores), ptr(goff), ptr(idx), ptr(val), P, Q, k, launch_stream(scores))
    return idx, val
