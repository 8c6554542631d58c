"""Sliding windows over long passages ("atpu-window v1"). Native: ``csrc/kernels/window.hip``.

``window_assemble``: the window rows ``[CLS] question [SEP] passage[a : a + len] [SEP]`` of long
passage rows (tokenizer output at a width ``L`` that holds the whole passage), one row per entry of the
host's window table ``(win_pair, win_start)``, with the window-relative start positions ``own [R, 2]``
each row owns (spec and pure-Python twins: :func:`agent_tpu_amd.tokenizer.window_table` /
:func:`agent_tpu_amd.tokenizer.window_rows`). ``ops.span_topk(..., own=own)`` then proposes every span
from exactly one window. The launch allocates nothing when the outputs are given and never
synchronizes, so it can be captured into a graph.

``window_best``: folds the window rows' ``(span [R, n, 2], score [R, n], null [R])`` back into one row
per pair: pair ``p`` owns the rows ``wrow[p] .. wrow[p + 1] - 1`` (offsets clamped into ``[0, R]`` like
``group_topk``'s), its ``n`` best elements in the total order of ``group_topk`` (score descending, then
flattened (row, slot) index ascending; a NaN ranks and is returned as ``-inf``), their spans moved by
``start[row]`` to passage-absolute tokens (an exhausted slot stays ``(-1, -1)``), padded with ``(-1, -1)``
/ ``-inf``. ``null[p]`` is the minimum of the rows' null scores, folded in row order with ``fminf`` (a NaN
is skipped; no rows: ``+inf``). Rows ordered by (pair, window) own rising starts, so the result is in the
order of one long row: score, then start, then end.
"""
from __future__ import annotations

from typing import Optional, Tuple

import torch

from .._native import native, ptr, launch_stream
from .. import tokenizer as _tok
from ._util import check, same_device

MAX_N = 32


def _i32(t: torch.Tensor, name: str) -> None:
    check(isinstance(t, torch.Tensor) and t.dtype == torch.int32 and t.is_contiguous(),
          f"{name} must be a contiguous int32 tensor")


def _is_int(v) -> bool:
    return isinstance(v, int) and not isinstance(v, bool)


def window_assemble_ref(ids_q, lens_q, ids_p, lens_p, qidx, win_pair, win_start, max_query_tokens: int,
                        doc_stride: int, cls_id: int, sep_id: int, pad_id: int, rows: int
                        ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """CPU reference: the twin on the first ``rows`` table entries."""
    out = _tok.window_rows(ids_q.numpy(), lens_q.numpy(), ids_p.numpy(), lens_p.numpy(), qidx.numpy(),
                           win_pair.numpy()[:rows], win_start.numpy()[:rows], max_query_tokens, doc_stride, cls_id,
                           sep_id, pad_id)
    return tuple(torch.from_numpy(a) for a in out)


def window_assemble(ids_q: torch.Tensor, lens_q: torch.Tensor, ids_p: torch.Tensor, lens_p: torch.Tensor,
                    qidx: torch.Tensor, win_pair: torch.Tensor, win_start: torch.Tensor, max_query_tokens: int,
                    doc_stride: int, cls_id: int = _tok.CLS_ID, sep_id: int = _tok.SEP_ID, pad_id: int = _tok.PAD_ID,
                    ids: Optional[torch.Tensor] = None, type_ids: Optional[torch.Tensor] = None,
                    lens: Optional[torch.Tensor] = None, own: Optional[torch.Tensor] = None,
                    rows: Optional[int] = None) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """``(ids [R, S], type_ids [R, S], lens [R], own [R, 2])`` int32 of the first ``rows`` (default: all)
    entries of the window table ``win_pair [>=R]`` / ``win_start [>=R]`` over the question rows ``ids_q
    [Q, S]`` / ``lens_q [Q]`` and the long passage rows ``ids_p [Pp, L]`` / ``lens_p [Pp]`` / ``qidx [Pp]``.
    Table entries are clamped (``win_pair`` into ``[0, Pp)``, ``win_start`` into ``[0, max(T - 1, 0)]``).
    Rows past ``rows`` of given outputs are not touched."""
    for t, name in ((ids_q, "ids_q"), (lens_q, "lens_q"), (ids_p, "ids_p"), (lens_p, "lens_p"), (qidx, "qidx"),
                    (win_pair, "win_pair"), (win_start, "win_start")):
        _i32(t, f"window_assemble: {name}")
    check(ids_q.dim() == 2 and ids_p.dim() == 2, "window_assemble: ids_q [Q, S] and ids_p [Pp, L]")
    (Q, S), (Pp, L) = ids_q.shape, ids_p.shape
    check(win_pair.dim() == 1 and win_start.dim() == 1, "window_assemble: win_pair [R] and win_start [R]")
    R = int(win_pair.numel() if rows is None else rows)
    check(_is_int(max_query_tokens) and max_query_tokens >= 0, "window_assemble: max_query_tokens must be an int >= 0")
    check(_is_int(doc_stride) and doc_stride >= 1, "window_assemble: doc_stride must be an int >= 1")
    check(S >= 4 and L >= 2 and Q >= 1 and Pp >= 1 and R >= 0, "window_assemble: S >= 4, L >= 2, Q >= 1, Pp >= 1, R >= 0")
    check(lens_q.numel() == Q and lens_p.numel() == Pp and qidx.numel() == Pp,
          "window_assemble: lens_q [Q], lens_p [Pp] and qidx [Pp]")
    check(win_pair.numel() >= R and win_start.numel() >= R, "window_assemble: win_pair/win_start too small")
    same_device(ids_q, lens_q, ids_p, lens_p, qidx, win_pair, win_start, ids, type_ids, lens, own)
    given = [o is not None for o in (ids, type_ids, lens, own)]
    check(all(given) or not any(given), "window_assemble: give ids, type_ids, lens and own together")
    if all(given):
        for t, name in ((ids, "ids"), (type_ids, "type_ids"), (lens, "lens"), (own, "own")):
            _i32(t, f"window_assemble: {name}")
        check(ids.dim() == 2 and ids.shape[1] == S and type_ids.shape == ids.shape and ids.shape[0] >= R
              and lens.numel() >= R and own.dim() == 2 and own.shape[1] == 2 and own.shape[0] >= R,
              "window_assemble: ids/type_ids/lens/own too small")
    if not ids_q.is_cuda:
        ref = window_assemble_ref(ids_q, lens_q, ids_p, lens_p, qidx, win_pair, win_start, max_query_tokens,
                                  doc_stride, int(cls_id), int(sep_id), int(pad_id), R)
        if ids is None:
            return ref
        for dst, src in zip((ids, type_ids, lens, own), ref):
            dst[:R].copy_(src)
        return ids, type_ids, lens, own
    if ids is None:
        dev = ids_q.device
        ids = torch.empty((R, S), dtype=torch.int32, device=dev)
        type_ids = torch.empty((R, S), dtype=torch.int32, device=dev)
        lens = torch.empty((R,), dtype=torch.int32, device=dev)
        own = torch.empty((R, 2), dtype=torch.int32, device=dev)
    if R:
        native().window_assemble(ptr(ids_q), ptr(lens_q), ptr(ids_p), ptr(lens_p), ptr(qidx), ptr(win_pair),
                                 ptr(win_start), ptr(ids), ptr(type_ids), ptr(lens), ptr(own), R, int(Pp), int(Q),
                                 int(S), int(L), max_query_tokens, doc_stride, int(cls_id), int(sep_id), int(pad_id),
                                 launch_stream(ids_q))
    return ids, type_ids, lens, own


def window_best_ref(span_w: torch.Tensor, score_w: torch.Tensor, null_w: torch.Tensor, start: torch.Tensor,
                    wrow: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """PyTorch twin -> ``(span [P, n, 2] int32, score [P, n] fp32, null [P] fp32)``; also the CPU path. A
    stable descending sort gives the (score desc, index asc) order."""
    span_w, score_w = span_w.detach().cpu(), score_w.detach().float().cpu()
    null_l, start_l = null_w.detach().float().cpu().tolist(), start.detach().cpu().tolist()
    R, n = score_w.shape
    P = wrow.numel() - 1
    span = torch.full((P, n, 2), -1, dtype=torch.int32)
    score = torch.full((P, n), float("-inf"), dtype=torch.float32)
    null = torch.full((P,), float("inf"), dtype=torch.float32)
    off = wrow.detach().cpu().tolist()
    for p in range(P):
        a = min(max(off[p], 0), R)
        b = max(min(max(off[p + 1], 0), R), a)
        s = score_w[a:b].reshape(-1)
        s = torch.where(torch.isnan(s), torch.full_like(s, float("-inf")), s)  # a NaN ranks as -inf
        order = torch.sort(s + 0.0, descending=True, stable=True).indices[:n]  # -0.0 + 0.0 = +0.0: they tie
        for r, e in enumerate(order.tolist()):
            row, slot = a + e // n, e % n
            s0, s1 = span_w[row, slot].tolist()
            if s0 >= 0:  # an exhausted slot of a window row stays (-1, -1)
                span[p, r, 0], span[p, r, 1] = s0 + start_l[row], s1 + start_l[row]
            score[p, r] = s[e]
        m = float("inf")
        for row in range(a, b):  # fminf in row order: a NaN is skipped
            x = null_l[row]
            if x == x and x < m:
                m = x
        null[p] = m
    return span, score, null


def window_best(span_w: torch.Tensor, score_w: torch.Tensor, null_w: torch.Tensor, start: torch.Tensor,
                wrow: torch.Tensor, span: Optional[torch.Tensor] = None, score: Optional[torch.Tensor] = None,
                null: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """``(span [P, n, 2] int32 passage-absolute, score [P, n] fp32, null [P] fp32)`` of the window rows'
    contiguous ``span_w [R, n, 2]`` int32, ``score_w [R, n]`` fp32, ``null_w [R]`` fp32 and window starts
    ``start [R]`` int32, grouped by the int32 offsets ``wrow [P + 1]``. Given outputs may hold more than
    ``P`` rows; rows past ``P`` are not touched. ``n`` in 1..32."""
    check(isinstance(score_w, torch.Tensor) and score_w.dtype == torch.float32 and score_w.dim() == 2
          and score_w.is_contiguous(), "window_best: score_w must be a contiguous fp32 [R, n]")
    R, n = int(score_w.shape[0]), int(score_w.shape[1])
    check(1 <= n <= MAX_N, "window_best: n must be in [1, 32]")
    _i32(span_w, "window_best: span_w"), _i32(start, "window_best: start"), _i32(wrow, "window_best: wrow")
    check(tuple(span_w.shape) == (R, n, 2), "window_best: span_w must be [R, n, 2]")
    check(isinstance(null_w, torch.Tensor) and null_w.dtype == torch.float32 and null_w.is_contiguous()
          and tuple(null_w.shape) == (R,), "window_best: null_w must be a contiguous fp32 [R]")
    check(tuple(start.shape) == (R,), "window_best: start must be [R]")
    check(wrow.dim() == 1 and wrow.numel() >= 1, "window_best: wrow must be [P + 1]")
    check(R * n < 2 ** 31 - 1, "window_best: R * n must be below 2^31")
    P = wrow.numel() - 1
    same_device(span_w, score_w, null_w, start, wrow, span, score, null)
    given = [o is not None for o in (span, score, null)]
    check(all(given) or not any(given), "window_best: give span, score and null together")
    if all(given):
        _i32(span, "window_best: span")
        check(span.dim() == 3 and tuple(span.shape[1:]) == (n, 2) and span.shape[0] >= P,
              "window_best: span must be [>=P, n, 2]")
        check(score.dtype == torch.float32 and score.is_contiguous() and score.dim() == 2 and score.shape[1] == n
              and score.shape[0] >= P, "window_best: score must be a contiguous fp32 [>=P, n]")
        check(null.dtype == torch.float32 and null.is_contiguous() and null.dim() == 1 and null.numel() >= P,
              "window_best: null must be a contiguous fp32 [>=P]")
    dev = score_w.device
    if not score_w.is_cuda or R == 0:  # no rows: every pair is empty
        ref = window_best_ref(span_w, score_w, null_w, start, wrow)
        if span is None:
            return tuple(t.to(dev) for t in ref)
        for dst, src in zip((span, score, null), ref):
            dst[:P].copy_(src)
        return span, score, null
    if span is None:
        span = torch.empty((P, n, 2), dtype=torch.int32, device=dev)
        score = torch.empty((P, n), dtype=torch.float32, device=dev)
        null = torch.empty((P,), dtype=torch.float32, device=dev)
    if P:
        native().window_best(ptr(span_w), ptr(score_w), ptr(null_w), ptr(start), ptr(wrow), ptr(span), ptr(score),
                             ptr(null), R, P, n, launch_stream(score_w))
    return span, score, null
