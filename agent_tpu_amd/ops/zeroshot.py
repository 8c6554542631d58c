"""Zero-shot classification ops. Native: ``csrc/kernels/zeroshot.hip``.

``premise_assemble``: ``[CLS] text [SEP] hypothesis [SEP]`` rows with their ``type_ids`` from the
single-segment rows the tokenizers emit (spec "atpu-premise v1" and pure-Python twin:
:func:`agent_tpu_amd.tokenizer.premise_rows`): the text is cut to the room the hypothesis leaves (HF
``only_first``), both segments are shared between rows (``tidx`` / ``hidx``). The launch allocates
nothing when the outputs are given and never synchronizes, so it can be captured into a graph.

``nli_rank``: the label scores of every text and their full ranking from the NLI logits ``pair [P, 2]``
= (entailment, contradiction), grouped by the offsets ``goff [T + 1]``. Multi-label, and any group of
one label (HF's rule): key ``e - c`` (one fp32 subtraction), score ``sigmoid(key)``. Single-label: key
``e``, score the softmax over the group. A NaN logit (or a NaN difference, ``inf - inf``) makes the key
``-inf`` and the score 0; a group whose best key is ``-inf`` scores 0 throughout; keys equal to a ``+inf``
maximum share the mass. The order is the project's total order (key descending, index ascending;
``+0.0`` and ``-0.0`` tie) over the whole group, of any length.
"""
from __future__ import annotations

import math
from typing import Optional, Tuple

import torch

from .._native import native, ptr, launch_stream
from .. import tokenizer as _tok
from ._util import check, same_device


def _i32(t: torch.Tensor, name: str) -> None:
    check(isinstance(t, torch.Tensor) and t.dtype == torch.int32 and t.is_contiguous(),
          f"{name} must be a contiguous int32 tensor")


def premise_assemble_ref(ids_t, lens_t, ids_h, lens_h, tidx, hidx, max_hypothesis_tokens: int, cls_id: int,
                         sep_id: int, pad_id: int, rows: int) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """CPU reference: the twin on the first ``rows`` rows."""
    i, t, l = _tok.premise_rows(ids_t.numpy(), lens_t.numpy(), ids_h.numpy(), lens_h.numpy(), tidx.numpy()[:rows],
                                hidx.numpy()[:rows], max_hypothesis_tokens, cls_id, sep_id, pad_id)
    return torch.from_numpy(i), torch.from_numpy(t), torch.from_numpy(l)


def premise_assemble(ids_t: torch.Tensor, lens_t: torch.Tensor, ids_h: torch.Tensor, lens_h: torch.Tensor,
                     tidx: torch.Tensor, hidx: torch.Tensor, max_hypothesis_tokens: int, cls_id: int = _tok.CLS_ID,
                     sep_id: int = _tok.SEP_ID, pad_id: int = _tok.PAD_ID, ids: Optional[torch.Tensor] = None,
                     type_ids: Optional[torch.Tensor] = None, lens: Optional[torch.Tensor] = None,
                     rows: Optional[int] = None) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """``(ids [P, S], type_ids [P, S], lens [P])`` int32 of the first ``rows`` (default: all of ``tidx``) pairs:
    row ``r`` reads the text row ``tidx[r]`` of ``ids_t [T, S]`` / ``lens_t [T]`` with the hypothesis row
    ``hidx[r]`` of ``ids_h [Hn, S]`` / ``lens_h [Hn]`` (both indices clamped into range). Rows past ``rows`` of
    given outputs are not touched."""
    for t, name in ((ids_t, "ids_t"), (lens_t, "lens_t"), (ids_h, "ids_h"), (lens_h, "lens_h"), (tidx, "tidx"),
                    (hidx, "hidx")):
        _i32(t, name)
    check(ids_t.dim() == 2 and ids_h.dim() == 2 and ids_t.shape[1] == ids_h.shape[1],
          "premise_assemble: ids_t [T, S] and ids_h [Hn, S]")
    T, S = ids_t.shape
    Hn = int(ids_h.shape[0])
    P = int(tidx.numel() if rows is None else rows)
    check(isinstance(max_hypothesis_tokens, int) and not isinstance(max_hypothesis_tokens, bool)
          and max_hypothesis_tokens >= 0, "premise_assemble: max_hypothesis_tokens must be an int >= 0")
    check(S >= 4 and T >= 1 and Hn >= 1 and P >= 0, "premise_assemble: S >= 4, T >= 1, Hn >= 1, P >= 0")
    check(lens_t.numel() == T and lens_h.numel() == Hn, "premise_assemble: lens_t must be [T] and lens_h [Hn]")
    check(tidx.dim() == 1 and hidx.dim() == 1 and tidx.numel() >= P and hidx.numel() >= P,
          "premise_assemble: tidx/hidx too small")
    same_device(ids_t, lens_t, ids_h, lens_h, tidx, hidx, ids, type_ids, lens)
    given = [o is not None for o in (ids, type_ids, lens)]
    check(all(given) or not any(given), "premise_assemble: give ids, type_ids and lens together")
    if all(given):
        _i32(ids, "ids"), _i32(type_ids, "type_ids"), _i32(lens, "lens")
        check(ids.dim() == 2 and ids.shape[1] == S and type_ids.shape == ids.shape and ids.shape[0] >= P
              and lens.numel() >= P, "premise_assemble: ids/type_ids/lens too small")
    if not ids_t.is_cuda:
        i, t, l = premise_assemble_ref(ids_t, lens_t, ids_h, lens_h, tidx, hidx, max_hypothesis_tokens, cls_id,
                                       sep_id, pad_id, P)
        if ids is None:
            return i, t, l
        ids[:P].copy_(i), type_ids[:P].copy_(t), lens[:P].copy_(l)
        return ids, type_ids, lens
    if ids is None:
        ids = torch.empty((P, S), dtype=torch.int32, device=ids_t.device)
        type_ids = torch.empty((P, S), dtype=torch.int32, device=ids_t.device)
        lens = torch.empty((P,), dtype=torch.int32, device=ids_t.device)
    if P:
        native().premise_assemble(ptr(ids_t), ptr(lens_t), ptr(ids_h), ptr(lens_h), ptr(tidx), ptr(hidx), ptr(ids),
                                  ptr(type_ids), ptr(lens), P, T, Hn, S, max_hypothesis_tokens, int(cls_id),
                                  int(sep_id), int(pad_id), launch_stream(ids_t))
    return ids, type_ids, lens


def nli_keys(pair: torch.Tensor, multi: bool) -> torch.Tensor:
    """The fp32 ranking keys of ``pair [n, 2]``: ``e - c`` (one fp32 subtraction) or ``e``; ``-inf`` for a NaN."""
    e, c = pair[:, 0].float(), pair[:, 1].float()
    k = e - c if multi else e.clone()
    bad = torch.isnan(e) | torch.isnan(c) | torch.isnan(k)
    return torch.where(bad, torch.full_like(k, float("-inf")), k)


def nli_rank_ref(pair: torch.Tensor, goff: torch.Tensor, multi_label: bool) -> Tuple[torch.Tensor, torch.Tensor]:
    """PyTorch twin -> (order ``[P]`` int32, score ``[P]`` fp32); also the CPU path. A stable descending sort
    of the keys gives the (key desc, index asc) order; the scores are evaluated in fp64 and rounded to fp32.
    Positions outside every group hold ``(-1, 0)``."""
    P = int(pair.shape[0])
    T = goff.numel() - 1
    order = torch.full((P,), -1, dtype=torch.int32)
    score = torch.zeros(P, dtype=torch.float32)
    off = goff.tolist()
    pair = pair.float().cpu()
    for t in range(T):
        a = min(max(off[t], 0), P)
        b = min(max(off[t + 1], 0), P)
        if b <= a:
            continue
        multi = bool(multi_label) or b - a == 1  # HF: one candidate label is scored entail-vs-contradiction
        k = nli_keys(pair[a:b], multi)
        k64 = k.double()
        if multi:
            s = 1.0 / (1.0 + torch.exp(-k64))
        else:
            mx = float(k64.max())
            if mx == -math.inf:
                s = torch.zeros_like(k64)
            else:
                w = torch.exp(torch.where(k64 == mx, torch.zeros_like(k64), k64 - mx))
                s = w / w.sum()
        o = torch.sort(k + 0.0, descending=True, stable=True).indices  # -0.0 + 0.0 = +0.0: they tie
        order[a:b] = o.to(torch.int32)
        score[a:b] = s[o].float()
    return order, score


def nli_rank(pair: torch.Tensor, goff: torch.Tensor, multi_label: bool) -> Tuple[torch.Tensor, torch.Tensor]:
    """(order ``[P]`` int32, score ``[P]`` fp32) of the contiguous fp32 logits ``pair [P, 2]`` grouped by the
    contiguous int32 offsets ``goff [T + 1]`` (clamped into ``[0, P]``; a decreasing pair is an empty group):
    position ``goff[t] + r`` holds the index within group ``t`` and the score of its ``r``-th ranked label.
    Positions outside every group hold ``(-1, 0)``."""
    check(isinstance(pair, torch.Tensor) and pair.dtype == torch.float32 and pair.dim() == 2 and pair.shape[1] == 2
          and pair.is_contiguous(), "nli_rank: pair must be a contiguous fp32 [P, 2]")
    _i32(goff, "nli_rank: goff")
    check(goff.dim() == 1 and goff.numel() >= 1, "nli_rank: goff must be [T + 1]")
    check(isinstance(multi_label, bool), "nli_rank: multi_label must be a bool")
    same_device(pair, goff)
    P, T = int(pair.shape[0]), goff.numel() - 1
    if not pair.is_cuda:
        return nli_rank_ref(pair, goff, multi_label)
    order = torch.full((P,), -1, dtype=torch.int32, device=pair.device)
    score = torch.zeros(P, dtype=torch.float32, device=pair.device)
    if P and T:
        native().nli_rank(ptr(pair), ptr(goff), ptr(order), ptr(score), P, T, int(multi_label), launch_stream(pair))
    return order, score
