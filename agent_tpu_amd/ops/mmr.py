"""Diversified results: maximal marginal relevance over a query's candidates (``csrc/kernels/sim_mmr.hip``).

:func:`mmr_select` takes every query's ``R <= 32`` candidate rows ``cand[i, :]`` of a ``store [N, D]`` (fp32, or fp16
with an optional fp32 ``row_scale [N]``) with their relevance scores ``rel[i, :]`` and picks ``k`` of them greedily.
With ``S`` the picks so far and ``G[l][j]`` the similarity of candidates ``l`` and ``j``,

    v_l = rel_l * lam                              while S is empty
    v_l = rel_l * lam - mu * max_{j in S} G[l][j]  afterwards

where ``lam`` and ``mu`` are ``lambda`` and ``1 - lambda`` (computed in fp64) rounded to fp32, every operation is one
fp32 rounding (no fused multiply-add), and a round's pick is the arg-max in the project's total order (``v``
descending, id ascending: ``better()`` of ``atpu/topk.h``). ``G[l][j]`` has the bits ``sim_topk`` gives the query
``store[l]`` against row ``j`` (times ``row_scale[l] * row_scale[j]``, that product rounded first) and is symmetric
bit for bit. The kernel forms ``G`` and runs the selection in one launch: neither the matrix nor a row leaves the
GPU. Greedy picks have the prefix property: the first ``k'`` picks of a ``k``-pick call are the ``k'``-pick call's.

An id outside ``[0, N)`` is an empty slot: it is never dereferenced and never picked; when the live candidates run
out the remaining entries are ``(PAD_ID, -inf, -inf)``. The live ids of one query must be distinct. The store may
live in pinned host memory, as ``refine_topk``'s.

:func:`rows_gather` copies rows of a store (and their scales) into a dense buffer: what a data-parallel rank
contributes to the candidate rows that rank 0 selects from.
"""
from __future__ import annotations

from typing import Optional, Tuple

import torch

from .._native import native, ptr, launch_stream
from ._util import check, same_device
from .search import MAX_ROWS, PAD_ID, _NO_ROW, sim_topk_ok

MAX_CANDIDATES = 32  # sim_topk's MAX_K: the candidates are one of its lists


def mmr_weights(lam: float) -> Tuple[float, float]:
    """(lam, mu): ``lambda`` and ``1 - lambda`` (in fp64) rounded to fp32, as Python floats."""
    t = torch.tensor([float(lam), 1.0 - float(lam)], dtype=torch.float64).to(torch.float32)
    return float(t[0]), float(t[1])


def _check_mmr(rel, cand, store, k, lam, id_base, row_scale):
    check(isinstance(store, torch.Tensor) and store.dim() == 2 and store.dtype in (torch.float32, torch.float16)
          and store.is_contiguous(), "mmr_select: the store must be a contiguous fp32 or fp16 [N, D]")
    N, D = store.shape
    check(sim_topk_ok(D, 1) and 1 <= N <= MAX_ROWS, f"mmr_select: unsupported shape D={D} N={N}")
    check(isinstance(cand, torch.Tensor) and cand.dim() == 2 and cand.dtype == torch.int32 and cand.is_contiguous()
          and 1 <= cand.shape[1] <= MAX_CANDIDATES, "mmr_select: cand must be a contiguous int32 [nq, R], R in [1, 32]")
    check(isinstance(rel, torch.Tensor) and rel.dtype == torch.float32 and rel.shape == cand.shape
          and rel.is_contiguous(), "mmr_select: rel must be a contiguous fp32 [nq, R]")
    check(isinstance(k, int) and not isinstance(k, bool) and 1 <= k <= cand.shape[1], "mmr_select: k must be in [1, R]")
    check(isinstance(lam, (int, float)) and not isinstance(lam, bool) and 0.0 <= lam <= 1.0,
          "mmr_select: lam must be a number in [0, 1]")
    if row_scale is not None:
        check(store.dtype == torch.float16, "mmr_select: row_scale needs an fp16 store")
        check(isinstance(row_scale, torch.Tensor) and row_scale.dtype == torch.float32 and row_scale.shape == (N,)
              and row_scale.is_contiguous(), "mmr_select: row_scale must be a contiguous fp32 [N]")
    check(isinstance(id_base, int) and 0 <= id_base < 2 ** 61, "mmr_select: id_base must be in [0, 2^61)")
    same_device(rel, cand, row_scale)
    check(store.device == rel.device or (rel.is_cuda and not store.is_cuda and store.is_pinned()),
          "mmr_select: the store must be on rel's device, or in pinned host memory for a device rel")


def _pad(ids: torch.Tensor, scores: torch.Tensor, mmr: torch.Tensor, empty: torch.Tensor):
    ninf = float("-inf")
    return (torch.where(empty, torch.full_like(ids, PAD_ID), ids), torch.where(empty, torch.full_like(scores, ninf), scores),
            torch.where(empty, torch.full_like(mmr, ninf), mmr))


def mmr_select_ref(rel: torch.Tensor, cand: torch.Tensor, store: torch.Tensor, k: int, lam: float, id_base: int = 0,
                   row_scale: Optional[torch.Tensor] = None, dtype=torch.float32
                   ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """PyTorch twin of :func:`mmr_select` in ``dtype`` math and the CPU path: the Gram matrix as the product of the
    gathered rows, the same three operations per round, the same total order (``-0.0`` and ``+0.0`` tie) and the
    same handling of empty slots. ``scores`` are ``rel``'s own values; ``mmr`` is of ``dtype``."""
    _check_mmr(rel, cand, store, k, lam, id_base, row_scale)
    nq, N = cand.shape[0], store.shape[0]
    dev = rel.device
    live = (cand >= 0) & (cand < N)
    rows = torch.where(live, cand, torch.zeros_like(cand)).to(torch.int64)
    C = store.to(dev)[rows].to(dtype)  # [nq, R, D]
    G = C @ C.transpose(1, 2)
    if row_scale is not None:
        s = row_scale.to(dev)[rows].to(dtype)
        G = G * (s[:, :, None] * s[:, None, :])
    lam32, mu32 = mmr_weights(lam)
    base = rel.to(dtype) * torch.tensor(lam32, dtype=dtype, device=dev)
    mu = torch.tensor(mu32, dtype=dtype, device=dev)
    ninf = torch.full_like(base, float("-inf"))
    ids = torch.where(live, rows, torch.full_like(rows, _NO_ROW))
    v, pen = torch.where(live, base, ninf), ninf.clone()
    out_i = torch.empty((nq, k), dtype=torch.int64, device=dev)
    out_s = torch.empty((nq, k), dtype=torch.float32, device=dev)
    out_m = torch.empty((nq, k), dtype=dtype, device=dev)
    for t in range(k):
        vz = v + 0.0  # -0.0 + 0.0 = +0.0: they tie
        tie = vz == vz.max(1, keepdim=True).values
        w = torch.where(tie, ids, torch.full_like(ids, 2 ** 40)).argmin(1, keepdim=True)  # the lowest id among the best
        out_i[:, t:t + 1] = torch.gather(ids, 1, w)
        out_s[:, t:t + 1] = torch.gather(rel, 1, w)
        out_m[:, t:t + 1] = torch.gather(v, 1, w)
        live = live.scatter(1, w, False)
        ids = torch.where(live, ids, torch.full_like(ids, _NO_ROW))
        pen = torch.maximum(pen, torch.gather(G, 2, w[:, None, :].expand(-1, G.shape[1], 1))[:, :, 0])
        v = torch.where(live, base - mu * pen, ninf)
    return _pad(out_i + int(id_base), out_s, out_m, out_i == _NO_ROW)


def mmr_select(rel: torch.Tensor, cand: torch.Tensor, store: torch.Tensor, k: int, lam: float, id_base: int = 0,
               row_scale: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """(ids ``[nq, k]`` int64 = ``id_base + row``, scores ``[nq, k]`` fp32 (the picks' relevance), mmr ``[nq, k]``
    fp32 (the picks' ``v``)), all in pick order, of the candidates ``cand [nq, R]`` (int32 rows of the contiguous
    ``store [N, D]``, ``R <= 32``) with relevance ``rel [nq, R]``. The result does not depend on the batch."""
    _check_mmr(rel, cand, store, k, lam, id_base, row_scale)
    nq, R = cand.shape
    if nq == 0:
        return (torch.empty((0, k), dtype=torch.int64, device=rel.device),
                torch.empty((0, k), dtype=torch.float32, device=rel.device),
                torch.empty((0, k), dtype=torch.float32, device=rel.device))
    if not rel.is_cuda:
        return mmr_select_ref(rel, cand, store, k, lam, id_base, row_scale)
    Rp = 16 if R <= 16 else 32  # the kernel's tile grid: 1 x 1 or 2 x 2
    if Rp != R:
        cand = torch.cat([cand, cand.new_full((nq, Rp - R), _NO_ROW)], 1).contiguous()
        rel = torch.cat([rel, rel.new_zeros((nq, Rp - R))], 1).contiguous()
    ids = torch.empty((nq, k), dtype=torch.int64, device=rel.device)
    scores = torch.empty((nq, k), dtype=torch.float32, device=rel.device)
    mmr = torch.empty((nq, k), dtype=torch.float32, device=rel.device)
    lam32, mu32 = mmr_weights(lam)
    N, D = store.shape
    native().mmr_select(ptr(cand), ptr(rel), ptr(store), store.dtype == torch.float16, ptr(row_scale), ptr(ids),
                        ptr(scores), ptr(mmr), nq, N, D, Rp, k, lam32, mu32, int(id_base), launch_stream(rel))
    return _pad(ids, scores, mmr, ids == int(id_base) + _NO_ROW)


def rows_gather_ref(ids: torch.Tensor, store: torch.Tensor, id_base: int = 0, row_scale: Optional[torch.Tensor] = None
                    ) -> Tuple[torch.Tensor, Optional[torch.Tensor]]:
    """PyTorch twin of :func:`rows_gather` and the CPU path."""
    N = store.shape[0]
    rows = ids - int(id_base)
    ok = (rows >= 0) & (rows < N)
    rows = torch.where(ok, rows, torch.zeros_like(rows))
    out = torch.where(ok[:, None], store[rows], torch.zeros((), dtype=store.dtype, device=store.device))
    if row_scale is None:
        return out, None
    return out, torch.where(ok, row_scale[rows], torch.ones((), dtype=torch.float32, device=store.device))


def rows_gather(ids: torch.Tensor, store: torch.Tensor, id_base: int = 0, row_scale: Optional[torch.Tensor] = None
                ) -> Tuple[torch.Tensor, Optional[torch.Tensor]]:
    """(out ``[m, D]`` in the store's dtype, out_scale ``[m]`` fp32 or None): the rows ``ids - id_base`` (int64
    ``[m]``) of the contiguous fp32 or fp16 ``store [N, D]`` and their ``row_scale``; an id outside the store gives a
    zero row and scale 1."""
    check(isinstance(store, torch.Tensor) and store.dim() == 2 and store.dtype in (torch.float32, torch.float16)
          and store.is_contiguous() and sim_topk_ok(store.shape[1], 1) and 1 <= store.shape[0] <= MAX_ROWS,
          "rows_gather: the store must be a contiguous fp32 or fp16 [N, D], D a multiple of 64 in [64, 1024]")
    check(isinstance(ids, torch.Tensor) and ids.dim() == 1 and ids.dtype == torch.int64 and ids.is_contiguous(),
          "rows_gather: ids must be a contiguous int64 [m]")
    N, D = store.shape
    if row_scale is not None:
        check(store.dtype == torch.float16 and isinstance(row_scale, torch.Tensor) and row_scale.dtype == torch.float32
              and row_scale.shape == (N,) and row_scale.is_contiguous(),
              "rows_gather: row_scale must be a contiguous fp32 [N] beside an fp16 store")
    check(isinstance(id_base, int) and 0 <= id_base < 2 ** 61, "rows_gather: id_base must be in [0, 2^61)")
    same_device(store, ids, row_scale)
    m = ids.numel()
    if not store.is_cuda or m == 0:
        return rows_gather_ref(ids, store, id_base, row_scale)
    out = torch.empty((m, D), dtype=store.dtype, device=store.device)
    out_scale = torch.empty((m,), dtype=torch.float32, device=store.device) if row_scale is not None else None
    native().rows_gather(ptr(ids), ptr(store), store.dtype == torch.float16, ptr(row_scale), ptr(out), ptr(out_scale), m,
                         N, D, int(id_base), launch_stream(store))
    return out, out_scale
