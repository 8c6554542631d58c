"""Token classification head on single-segment rows. Native: ``csrc/kernels/tag_head.hip``.

``tag_entities`` turns the last layer's rows of ``[CLS] text [SEP]`` rows into a label and a
probability per text token and the row's grouped entities. The text tokens are the positions ``j``
in ``[1, len - 2]`` with ``len = clamp(lens[b], 2, S)``; ``[CLS]`` and ``[SEP]`` are never tagged.

Logits, as ``span_topk``: on the LayerNorm-folded encoder the last layer leaves raw rows ``g_j`` and
``fin = (rstd_j, rstd_j * mu_j)`` and the LayerNorm folds into the linear head:

    logit_c[j] = rstd_j * (g_j . u_c) - (rstd_j mu_j) * su_c + c_c
    u = gamma * W,  su = the row sums of u,  c = beta . W + b

Without ``fin`` the rows are already normalised and ``logit_c[j] = x_j . u_c + c_c``.

Per token: ``y_j`` is the argmax in the order (logit descending, label ascending); a NaN ranks as
``-inf`` and an all-NaN token has label 0. ``p_j = 1 / sum_c exp(logit_c - max)``: a NaN logit adds 0,
a logit equal to the maximum adds exactly 1 (so infinite maxima are defined), and an all-NaN token
has ``p = 0``.

Grouping, driven by ``label_type [L]`` (the entity type of a label, ``-1`` outside) and
``label_begin [L]`` (1 for a ``B-`` label). With ``t_j = label_type[y_j]``, ``b_j = label_begin[y_j]``:

* mode 0 (tokens): every text token with ``t_j >= 0`` is the record ``(j - 1, j - 1, y_j, 1)``.
* mode 1 (simple): token ``j`` starts a group when ``t_j >= 0`` and (``j == 1`` or ``t_{j-1} != t_j`` or
  ``b_j``); the group runs to the last token before the next start, type change or ``[SEP]``.
* mode 2 (first): a continuation token (``cont[ids[b, j]] != 0``; ids outside ``[0, V)`` and token 1 are
  never one) first takes ``y`` of the nearest earlier non-continuation token, never starts a group,
  always extends its word's group and its ``p`` is left out of the sum. Then as mode 1.

Records ``ent [B, E, 4] = (first, last, type, n)`` with text-relative token positions (in mode 0 the
third field is the label) and ``ent_sum [B, E]``, the fp32 sum of the ``n`` probabilities added in
token order. The first ``E`` groups in token order are written; ``count [B]`` is the true number;
unused slots are ``(-1, -1, -1, 0)`` with ``0.0``.
"""
from __future__ import annotations

import math
from typing import Optional, Tuple

import torch

from .._native import native, ptr, launch_stream
from ._util import check, check_bf16_dev, same_device

MAX_LABELS = 64
MAX_ENTITIES = 512
MODES = {"none": 0, "simple": 1, "first": 2}


def default_tag_names(L: int) -> list:
    """Label names of a head without names: label 0 is ``O``; label ``l >= 1`` is ``B-T{(l-1)//2}`` when
    ``l`` is odd and ``I-T{(l-1)//2}`` when it is even."""
    return ["O"] + [("B-" if l & 1 else "I-") + f"T{(l - 1) // 2}" for l in range(1, int(L))]


def tag_tables(names, outside=("O",)):
    """``(type_names, label_type, label_begin)`` of label ``names``, as HF's ``get_tag`` reads them: ``B-X``
    is ``(X, begin)``, ``I-X`` is ``(X, not begin)``, any other name ``N`` is ``(N, not begin)``; a name in
    ``outside`` has type ``-1``. Types are numbered in order of first appearance."""
    out = set(outside)
    type_names, label_type, label_begin = [], [], []
    for n in names:
        if n in out:
            label_type.append(-1), label_begin.append(0)
            continue
        begin = n.startswith("B-")
        t = n[2:] if begin or n.startswith("I-") else n
        if t not in type_names:
            type_names.append(t)
        label_type.append(type_names.index(t)), label_begin.append(int(begin))
    return (type_names, torch.tensor(label_type, dtype=torch.int32), torch.tensor(label_begin, dtype=torch.int32))


def tag_ok(S: int, H: int, L: int) -> bool:
    """Shapes the kernel takes: 3..512 tokens, H a multiple of 64 from 64 to 1024, 1..64 labels."""
    return 3 <= S <= 512 and H % 64 == 0 and 64 <= H <= 1024 and 1 <= L <= MAX_LABELS


def tag_logits_ref(x: torch.Tensor, lens: torch.Tensor, B: int, u: torch.Tensor, su: Optional[torch.Tensor],
                   c: torch.Tensor, fin: Optional[torch.Tensor] = None, dtype=torch.float32) -> torch.Tensor:
    """``logits [B, S, L]`` of ``dtype`` by the kernel's formula in ``dtype`` math; ``-inf`` outside the
    text tokens ``[1, len - 2]`` (selected with ``torch.where``, never by a multiply)."""
    H = x.shape[-1]
    L = u.shape[0]
    S = x.numel() // (B * H)
    xx = x.to(dtype).view(B * S, H)
    d = xx @ u.to(dtype).t()  # [B*S, L]
    if fin is not None:
        f = fin.to(dtype)
        lg = f[:, :1] * d - f[:, 1:] * su.to(dtype).view(1, L) + c.to(dtype).view(1, L)
    else:
        lg = d + c.to(dtype).view(1, L)
    n = lens.reshape(-1)[:B].to(device=x.device, dtype=torch.int64).clamp(2, S)
    pos = torch.arange(S, device=x.device).view(1, S)
    live = ((pos >= 1) & (pos <= n.view(B, 1) - 2)).view(B, S, 1)
    return torch.where(live, lg.view(B, S, L), torch.full((), float("-inf"), dtype=dtype, device=x.device))


def tag_group_ref(label: torch.Tensor, prob: torch.Tensor, lens: torch.Tensor, label_type: torch.Tensor,
                  label_begin: torch.Tensor, mode: int, E: int, ids: Optional[torch.Tensor] = None,
                  cont: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """The grouping of the kernel on given per-token ``label [B, S]`` and fp32 ``prob [B, S]`` ->
    ``(ent [B, E, 4] int32, ent_sum [B, E] fp32, count [B] int32)`` on the CPU, as plain loops."""
    lab = label.detach().cpu().to(torch.int64)
    B, S = lab.shape
    pr = prob.detach().cpu().float()
    ln = lens.detach().cpu().reshape(-1)[:B].to(torch.int64).clamp(2, S).tolist()
    ltype = label_type.detach().cpu().tolist()
    lbeg = label_begin.detach().cpu().tolist()
    if mode == 2:
        idl = ids.detach().cpu().view(-1, S)[:B].tolist()
        ct = cont.detach().cpu().reshape(-1).tolist()
        V = len(ct)
    ent = torch.full((B, E, 4), -1, dtype=torch.int32)
    ent[:, :, 3] = 0
    ent_sum = torch.zeros((B, E), dtype=torch.float32)
    count = torch.zeros((B,), dtype=torch.int32)
    for b in range(B):
        hi = ln[b] - 2  # the last text token; the text is 1 .. hi
        y = lab[b].tolist()
        co = [False] * S
        if mode == 2:
            for j in range(2, hi + 1):  # token 1 is never a continuation
                v = idl[b][j]
                co[j] = bool(ct[v]) if 0 <= v < V else False
            for j in range(2, hi + 1):
                if co[j]:
                    y[j] = y[j - 1]  # the word's head, by induction
        groups = []  # [first, last, third field, scored positions]
        for j in range(1, hi + 1):
            t = ltype[y[j]]
            if mode == 0:
                if t >= 0:
                    groups.append([j, j, y[j], [j]])
                continue
            prev_t = ltype[y[j - 1]] if j > 1 else None
            start = t >= 0 and not co[j] and (j == 1 or prev_t != t or bool(lbeg[y[j]]))
            if start:
                groups.append([j, j, t, [j]])
            elif t >= 0 and groups and groups[-1][1] == j - 1 and groups[-1][2] == t:
                groups[-1][1] = j
                if not co[j]:
                    groups[-1][3].append(j)
        count[b] = len(groups)
        for e, (first, last, third, scored) in enumerate(groups[:E]):
            s = torch.zeros((), dtype=torch.float32)
            for k in scored:
                s = s + pr[b, k]  # sequential fp32, in token order
            ent[b, e] = torch.tensor([first - 1, last - 1, third, len(scored)], dtype=torch.int32)
            ent_sum[b, e] = s
    return ent, ent_sum, count


def tag_select_ref(logits: torch.Tensor, lens: torch.Tensor, label_type: torch.Tensor, label_begin: torch.Tensor,
                   mode: int, E: int, ids: Optional[torch.Tensor] = None, cont: Optional[torch.Tensor] = None
                   ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """The selection of the kernel on given fp32 ``logits [B, S, L]`` -> ``(ent, ent_sum, count, label
    [B, S] int32, prob [B, S] fp32)`` on the CPU: the argmax and the probability of every text token
    (the exponentials in fp64, rounded once), then :func:`tag_group_ref`. Also the CPU path."""
    lg = logits.detach().float().cpu()
    B, S, L = lg.shape
    ln = lens.detach().cpu().reshape(-1)[:B].to(torch.int64).clamp(2, S).tolist()
    label = torch.full((B, S), -1, dtype=torch.int32)
    prob = torch.zeros((B, S), dtype=torch.float32)
    for b in range(B):
        rows = lg[b].tolist()
        for j in range(1, ln[b] - 1):
            row = rows[j]
            best, bv = 0, float("-inf")
            for cidx in range(L):
                v = row[cidx]
                v = float("-inf") if v != v else v  # a NaN ranks as -inf
                if v > bv:  # ties keep the lower label
                    best, bv = cidx, v
            s = 0.0
            for cidx in range(L):
                v = row[cidx]
                if v != v:
                    continue
                s += 1.0 if v == bv else math.exp(v - bv)
            label[b, j] = best
            prob[b, j] = 1.0 / s if s > 0.0 else 0.0
    return tag_group_ref(label, prob, lens, label_type, label_begin, mode, E, ids, cont) + (label, prob)


def _out(t: Optional[torch.Tensor], shape, dtype, device, name: str) -> torch.Tensor:
    if t is None:
        return torch.empty(shape, dtype=dtype, device=device)
    check(t.dtype == dtype and t.is_contiguous() and t.dim() == len(shape) and t.shape[0] >= shape[0]
          and tuple(t.shape[1:]) == tuple(shape[1:]), f"tag_entities: {name} must be contiguous {dtype} {list(shape)}")
    return t


def tag_entities(x: torch.Tensor, lens: torch.Tensor, B: int, S: int, u: torch.Tensor, su: Optional[torch.Tensor],
                 c: torch.Tensor, label_type: torch.Tensor, label_begin: torch.Tensor, mode: int, max_entities: int,
                 fin: Optional[torch.Tensor] = None, ids: Optional[torch.Tensor] = None,
                 cont: Optional[torch.Tensor] = None, ent: Optional[torch.Tensor] = None,
                 ent_sum: Optional[torch.Tensor] = None, count: Optional[torch.Tensor] = None,
                 label_out: Optional[torch.Tensor] = None, prob_out: Optional[torch.Tensor] = None,
                 logits_out: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """``(ent [B, E, 4] int32, ent_sum [B, E] fp32, count [B] int32)`` of the hidden rows ``x [B*S, H]``
    (raw rows when ``fin [B*S, 2]`` is given, with ``su``; else normalised rows), ``lens [B]`` int32, the
    head ``u [L, H]``, ``su [L]``, ``c [L]`` fp32 and the int32 tables ``label_type [L]``, ``label_begin [L]``.
    ``mode`` 0 / 1 / 2 = tokens / simple / first; mode 2 needs ``ids [B, S]`` int32 and ``cont [V]`` uint8.
    Given outputs may hold more than ``B`` rows; rows past ``B`` are not touched. ``label_out [B, S]``
    int32, ``prob_out [B, S]`` fp32 and ``logits_out [B, S, L]`` fp32 are written when given."""
    E = max_entities
    check(isinstance(B, int) and B >= 0, "tag_entities: B must be an int >= 0")
    check(isinstance(S, int) and not isinstance(S, bool), "tag_entities: S must be an int")
    check(x.dim() == 2 and x.shape[0] == B * S, "tag_entities: x must be [B*S, H]")
    H = int(x.shape[1])
    check(u.dim() == 2 and u.shape[1] == H, "tag_entities: u must be [L, H]")
    L = int(u.shape[0])
    check(isinstance(mode, int) and not isinstance(mode, bool) and mode in (0, 1, 2),
          "tag_entities: mode must be 0, 1 or 2")
    check(isinstance(E, int) and not isinstance(E, bool) and 1 <= E <= MAX_ENTITIES,
          "tag_entities: max_entities must be an int in [1, 512]")
    check(tag_ok(S, H, L), f"tag_entities: unsupported shape S={S} H={H} L={L}")
    check(lens.numel() >= B and lens.dtype == torch.int32 and lens.is_contiguous(),
          "tag_entities: lens must hold B contiguous int32 lengths")
    check(c.numel() == L and (su is None or su.numel() == L), "tag_entities: su [L], c [L]")
    for t, name in ((label_type, "label_type"), (label_begin, "label_begin")):
        check(t.dtype == torch.int32 and t.is_contiguous() and tuple(t.shape) == (L,),
              f"tag_entities: {name} must be contiguous int32 [L]")
    if fin is not None:
        check(tuple(fin.shape) == (B * S, 2) and fin.dtype == torch.float32, "tag_entities: fin must be fp32 [B*S, 2]")
        check(su is not None, "tag_entities: fin needs su")
    V = 0
    if mode == 2:
        check(ids is not None and cont is not None, "tag_entities: mode 2 needs ids and cont")
        check(ids.dtype == torch.int32 and ids.is_contiguous() and ids.dim() == 2 and ids.shape[0] >= B
              and ids.shape[1] == S, "tag_entities: ids must be contiguous int32 [B, S]")
        check(cont.dtype == torch.uint8 and cont.is_contiguous() and cont.dim() == 1 and cont.numel() >= 1,
              "tag_entities: cont must be contiguous uint8 [V]")
        V = int(cont.numel())
    same_device(x, fin, u, su, c, lens, label_type, label_begin, ids if mode == 2 else None,
                cont if mode == 2 else None, ent, ent_sum, count, label_out, prob_out, logits_out)
    dev = x.device
    ent = _out(ent, (B, E, 4), torch.int32, dev, "ent")
    ent_sum = _out(ent_sum, (B, E), torch.float32, dev, "ent_sum")
    count = _out(count, (B,), torch.int32, dev, "count")
    if label_out is not None:
        _out(label_out, (B, S), torch.int32, dev, "label_out")
    if prob_out is not None:
        _out(prob_out, (B, S), torch.float32, dev, "prob_out")
    if logits_out is not None:
        _out(logits_out, (B, S, L), torch.float32, dev, "logits_out")
    if B == 0:
        return ent, ent_sum, count
    if not x.is_cuda:
        lg = tag_logits_ref(x, lens, B, u, su, c, fin).float()
        e, s, n, lab, pr = tag_select_ref(lg, lens, label_type, label_begin, mode, E, ids, cont)
        ent[:B].copy_(e), ent_sum[:B].copy_(s), count[:B].copy_(n)
        if label_out is not None:
            label_out[:B].copy_(lab)
        if prob_out is not None:
            prob_out[:B].copy_(pr)
        if logits_out is not None:
            logits_out[:B].copy_(lg)
        return ent, ent_sum, count
    check_bf16_dev(x, "x")
    check(x.is_contiguous() and (fin is None or fin.is_contiguous()), "tag_entities: contiguous tensors")
    for t, name in ((u, "u"), (su, "su"), (c, "c")):
        check(t is None or (t.dtype == torch.float32 and t.is_contiguous()),
              f"tag_entities: {name} must be contiguous fp32")
    opt = lambda t: ptr(t) if t is not None else 0  # noqa: E731
    native().tag_entities(ptr(x), opt(fin), ptr(u), opt(su), ptr(c), ptr(lens), ptr(label_type), ptr(label_begin),
                          opt(ids) if mode == 2 else 0, opt(cont) if mode == 2 else 0, ptr(ent), ptr(ent_sum),
                          ptr(count), opt(label_out), opt(prob_out), opt(logits_out), B, S, H, L, V, mode, E,
                          launch_stream(x))
    return ent, ent_sum, count
