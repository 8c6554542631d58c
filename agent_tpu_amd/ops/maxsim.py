"""Late-interaction (ColBERT) scoring ops. Native: ``csrc/kernels/maxsim.hip``.

``token_unit``: every row of ``x [M, P]`` (bf16 or fp32) divided by ``max(||row||_2, 1e-12)`` in fp32,
``pool_embed``'s normalisation (a zero row stays zero). Rows of padding positions are normalised like any
other: ``maxsim`` is what ignores them.

``maxsim``: the score of pair ``p``, query row ``qidx[p]`` against passage row ``didx[p]``,

    score = sum over query tokens i < len_q of  max over passage tokens j < len_d of  <Q[i], D[j]>

with every dot product in exact fp32 in ``sim_topk``'s k order (a function of ``P`` alone), the max taken
by select (a token ``>= len`` never wins and adds nothing, whatever its row holds) and the sum in fp32 in
increasing ``i``, left to right. A score is a function of the pair's own rows only: not of ``n``, the pair's
position, ``Qn``, ``Dn`` or the launch. ``lens`` are clamped into ``[1, S]``, ``qidx`` / ``didx`` into
``[0, Qn)`` / ``[0, Dn)``. A NaN in a live dot product is undefined, as in ``sim_topk``. The launches
allocate nothing when ``out`` is given and never synchronize, so they can be captured into a graph.

``maxsim_index`` (``csrc/kernels/maxsim_index.hip``): the same score against a packed index, ``tok [T, P]``
(fp16 or fp32: the live unit token vectors of ``N`` passages back to back, no padding rows) with ``off [N + 1]``
int64. A work item is one passage, ``pidx[m]``; it is scored against every query (all form, ``[Qn, M]``) or
against the queries ``qsel[qoff[m] .. qoff[m + 1])`` (list form, ``[E]``). fp16 rows are widened in registers,
which is exact; an fp32 index has the bits of ``maxsim`` on the padded tensors. ``pidx`` is clamped into
``[0, N)``, ``qsel`` into ``[0, Qn)``, ``qoff`` into ``[0, E]`` and made monotone, a passage's start into
``[0, T)`` and its length ``off[p + 1] - off[p]`` into ``[1, T - start]``.
"""
from __future__ import annotations

from typing import Optional

import torch

from .._native import native, ptr, launch_stream
from ._util import check, same_device

EPS = 1e-12  # F.normalize's, as pool_embed


def maxsim_ok(P: int) -> bool:
    """Widths the kernels take: a multiple of 64 from 64 to 1024 (``sim_topk``'s D)."""
    return P % 64 == 0 and 64 <= P <= 1024


def token_unit_ref(x: torch.Tensor, dtype=torch.float32) -> torch.Tensor:
    """PyTorch twin in ``dtype`` math -> ``[M, P]`` of ``dtype`` (also the CPU path)."""
    xx = x.to(dtype)
    return xx / xx.norm(dim=1, keepdim=True).clamp_min(EPS)


def token_unit(x: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``[M, P]`` fp32: the rows of the contiguous ``x [M, P]`` (bf16 or fp32) L2-normalised in fp32."""
    check(isinstance(x, torch.Tensor) and x.dim() == 2 and x.dtype in (torch.bfloat16, torch.float32),
          "token_unit: x must be a bf16 or fp32 [M, P]")
    M, P = x.shape
    if out is not None:
        check(out.dtype == torch.float32 and tuple(out.shape) == (M, P) and out.is_contiguous(),
              "token_unit: out must be contiguous fp32 [M, P]")
    same_device(x, out)
    if not x.is_cuda:
        y = token_unit_ref(x)
        return out.copy_(y) if out is not None else y
    check(maxsim_ok(P), "token_unit: P must be a multiple of 64 in [64, 1024]")
    check(x.is_contiguous(), "token_unit: x must be contiguous")
    if out is None:
        out = torch.empty((M, P), dtype=torch.float32, device=x.device)
    if M:
        native().token_unit(ptr(x), ptr(out), M, P, 1 if x.dtype == torch.bfloat16 else 0, launch_stream(x))
    return out


def maxsim_ref(qv: torch.Tensor, lens_q: torch.Tensor, dv: torch.Tensor, lens_d: torch.Tensor, qidx: torch.Tensor,
               didx: torch.Tensor, dtype=torch.float32) -> torch.Tensor:
    """PyTorch twin in ``dtype`` math -> ``[n]`` of ``dtype`` (also the CPU path): the same masking by select
    (only the live rows are sliced in; ``torch.maximum``) and the same summation order over the query tokens."""
    Qn, S, _ = qv.shape
    Dn = dv.shape[0]
    n = qidx.numel()
    out = torch.zeros(n, dtype=dtype)
    lq_all = lens_q.reshape(-1).tolist()
    ld_all = lens_d.reshape(-1).tolist()
    for p, (a, b) in enumerate(zip(qidx.reshape(-1).tolist(), didx.reshape(-1).tolist())):
        a, b = min(max(a, 0), Qn - 1), min(max(b, 0), Dn - 1)
        lq, ld = min(max(lq_all[a], 1), S), min(max(ld_all[b], 1), S)
        # only live rows enter the product; + 0.0: a sum of -0.0 products is +0.0, as on an accumulator that
        # starts at +0.0
        sim = qv[a, :lq].to(dtype).cpu() @ dv[b, :ld].to(dtype).cpu().T + 0.0  # [lq, ld]
        m = torch.full((lq,), float("-inf"), dtype=dtype)
        for j in range(ld):
            m = torch.maximum(m, sim[:, j])
        s = m[0].clone()
        for i in range(1, lq):  # ((m0 + m1) + m2) + ...
            s = s + m[i]
        out[p] = s
    return out


def maxsim(qv: torch.Tensor, lens_q: torch.Tensor, dv: torch.Tensor, lens_d: torch.Tensor, qidx: torch.Tensor,
           didx: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``scores [n]`` fp32 of the pairs ``(qidx[p], didx[p])`` over the contiguous fp32 unit token vectors
    ``qv [Qn, S, P]`` / ``dv [Dn, S, P]`` with the contiguous int32 lengths ``lens_q [Qn]`` / ``lens_d [Dn]``
    and indices ``qidx [n]`` / ``didx [n]``. ``P`` a multiple of 64 in [64, 1024]."""
    for t, name in ((qv, "qv"), (dv, "dv")):
        check(isinstance(t, torch.Tensor) and t.dtype == torch.float32 and t.dim() == 3 and t.is_contiguous(),
              f"maxsim: {name} must be a contiguous fp32 [rows, S, P]")
    for t, name in ((lens_q, "lens_q"), (lens_d, "lens_d"), (qidx, "qidx"), (didx, "didx")):
        check(isinstance(t, torch.Tensor) and t.dtype == torch.int32 and t.dim() == 1 and t.is_contiguous(),
              f"maxsim: {name} must be a contiguous int32 vector")
    Qn, S, P = qv.shape
    Dn = dv.shape[0]
    check(tuple(dv.shape[1:]) == (S, P), "maxsim: qv and dv must share S and P")
    check(maxsim_ok(P), "maxsim: P must be a multiple of 64 in [64, 1024]")
    check(S >= 1 and Qn >= 1 and Dn >= 1, "maxsim: S, Qn and Dn must be >= 1")
    check(lens_q.numel() == Qn and lens_d.numel() == Dn, "maxsim: lens_q must be [Qn] and lens_d [Dn]")
    n = qidx.numel()
    check(didx.numel() == n, "maxsim: qidx and didx must have the same length")
    if out is not None:
        check(out.dtype == torch.float32 and out.dim() == 1 and out.numel() == n and out.is_contiguous(),
              "maxsim: out must be contiguous fp32 [n]")
    same_device(qv, lens_q, dv, lens_d, qidx, didx, out)
    if not qv.is_cuda:
        s = maxsim_ref(qv, lens_q, dv, lens_d, qidx, didx)
        return out.copy_(s) if out is not None else s
    if out is None:
        out = torch.empty(n, dtype=torch.float32, device=qv.device)
    if n:
        native().maxsim(ptr(qv), ptr(lens_q), ptr(dv), ptr(lens_d), ptr(qidx), ptr(didx), ptr(out), n, Qn, Dn, S, P,
                        launch_stream(qv))
    return out


def _index_item(off: list, p: int, T: int):
    """``(start, length)`` of passage ``p`` with the kernel's clamps."""
    start = min(max(off[p], 0), T - 1)
    return start, min(max(off[p + 1] - off[p], 1), T - start)


def maxsim_index_ref(qv: torch.Tensor, lens_q: torch.Tensor, tok: torch.Tensor, off: torch.Tensor,
                     pidx: Optional[torch.Tensor] = None, qoff: Optional[torch.Tensor] = None,
                     qsel: Optional[torch.Tensor] = None, dtype=torch.float32) -> torch.Tensor:
    """PyTorch twin of :func:`maxsim_index` in ``dtype`` math (also the CPU path): ``[Qn, M]`` in the all form,
    ``[E]`` in the list form. The same clamps, the same select (only the live rows are sliced in) and the same
    summation order as :func:`maxsim_ref`; the stored values are widened to ``dtype``, which is exact."""
    Qn, S, _ = qv.shape
    T, N = int(tok.shape[0]), int(off.numel()) - 1
    offs = off.reshape(-1).tolist()
    items = list(range(N)) if pidx is None else [min(max(p, 0), N - 1) for p in pidx.reshape(-1).tolist()]
    M = len(items)
    lq_all = [min(max(v, 1), S) for v in lens_q.reshape(-1).tolist()]
    list_form = qoff is not None
    if list_form:
        sel = qsel.reshape(-1).tolist()
        E = len(sel)
        bounds = qoff.reshape(-1).tolist()
        out = torch.zeros(E, dtype=dtype)
    else:
        out = torch.zeros((Qn, M), dtype=dtype)
    qc, tc = qv.cpu(), tok.cpu()
    for m, p in enumerate(items):
        if list_form:
            lo = min(max(bounds[m], 0), E)
            entries = [(e, min(max(sel[e], 0), Qn - 1)) for e in range(lo, min(max(bounds[m + 1], lo), E))]
        else:
            entries = [(q, q) for q in range(Qn)]
        if not entries:
            continue
        start, ln = _index_item(offs, p, T)
        d = tc[start:start + ln].to(dtype)
        for e, a in entries:
            lq = lq_all[a]
            sim = qc[a, :lq].to(dtype) @ d.T + 0.0  # [lq, ln]; + 0.0 as in maxsim_ref
            mx = torch.full((lq,), float("-inf"), dtype=dtype)
            for j in range(ln):
                mx = torch.maximum(mx, sim[:, j])
            s = mx[0].clone()
            for i in range(1, lq):  # ((m0 + m1) + m2) + ...
                s = s + mx[i]
            if list_form:
                out[e] = s
            else:
                out[a, m] = s
    return out


def maxsim_index(qv: torch.Tensor, lens_q: torch.Tensor, tok: torch.Tensor, off: torch.Tensor,
                 pidx: Optional[torch.Tensor] = None, qoff: Optional[torch.Tensor] = None,
                 qsel: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Scores of the contiguous fp32 unit query vectors ``qv [Qn, S, P]`` (int32 ``lens_q [Qn]``) against the
    passages of the index ``tok [T, P]`` (contiguous fp16 or fp32) / ``off [N + 1]`` (int64). Item ``m`` is
    passage ``pidx[m]`` (int32 ``[M]``; ``None``: every passage, ``M = N``). All form (``qoff`` and ``qsel``
    ``None``): ``[Qn, M]`` fp32, query-major. List form: ``[E]``, entry ``e`` in ``qoff[m] .. qoff[m + 1] - 1``
    (int32 ``[M + 1]``) being query ``qsel[e]`` (int32 ``[E]``) against item ``m``; an empty range is valid.
    ``P`` a multiple of 64 in [64, 1024]."""
    check(isinstance(qv, torch.Tensor) and qv.dtype == torch.float32 and qv.dim() == 3 and qv.is_contiguous(),
          "maxsim_index: qv must be a contiguous fp32 [Qn, S, P]")
    check(isinstance(tok, torch.Tensor) and tok.dtype in (torch.float16, torch.float32) and tok.dim() == 2
          and tok.is_contiguous(), "maxsim_index: tok must be a contiguous fp16 or fp32 [T, P]")
    check(isinstance(off, torch.Tensor) and off.dtype == torch.int64 and off.dim() == 1 and off.is_contiguous()
          and off.numel() >= 2, "maxsim_index: off must be a contiguous int64 [N + 1]")
    check((qoff is None) == (qsel is None), "maxsim_index: qoff and qsel come together")
    for t, name in ((lens_q, "lens_q"), (pidx, "pidx"), (qoff, "qoff"), (qsel, "qsel")):
        check(t is None and name != "lens_q" or isinstance(t, torch.Tensor) and t.dtype == torch.int32
              and t.dim() == 1 and t.is_contiguous(), f"maxsim_index: {name} must be a contiguous int32 vector")
    Qn, S, P = qv.shape
    T, N = int(tok.shape[0]), int(off.numel()) - 1
    check(int(tok.shape[1]) == P, "maxsim_index: qv and tok must share P")
    check(maxsim_ok(P), "maxsim_index: P must be a multiple of 64 in [64, 1024]")
    check(S >= 1 and Qn >= 1 and T >= 1, "maxsim_index: S, Qn and T must be >= 1")
    check(lens_q.numel() == Qn, "maxsim_index: lens_q must be [Qn]")
    M = N if pidx is None else int(pidx.numel())
    E = 0
    if qoff is not None:
        check(qoff.numel() == M + 1, "maxsim_index: qoff must be [M + 1]")
        E = int(qsel.numel())
    shape = (E,) if qoff is not None else (Qn, M)
    if out is not None:
        check(out.dtype == torch.float32 and tuple(out.shape) == shape and out.is_contiguous(),
              "maxsim_index: out must be contiguous fp32 [Qn, M] (all form) or [E] (list form)")
    same_device(qv, lens_q, tok, off, pidx, qoff, qsel, out)
    if not qv.is_cuda:
        s = maxsim_index_ref(qv, lens_q, tok, off, pidx, qoff, qsel)
        return out.copy_(s) if out is not None else s
    if out is None:
        out = torch.empty(shape, dtype=torch.float32, device=qv.device)
    if M and out.numel():
        native().maxsim_index(ptr(qv), ptr(lens_q), ptr(tok), ptr(off), ptr(pidx) if pidx is not None else 0,
                              ptr(qoff) if qoff is not None else 0, ptr(qsel) if qsel is not None else 0, ptr(out),
                              Qn, S, P, T, N, M, E, 1 if tok.dtype == torch.float16 else 0, launch_stream(qv))
    return out
