"""Exact re-scoring of a shortlist: every query against its own candidate rows (``csrc/kernels/sim_refine.hip``).

:func:`refine_topk` scores query ``i`` against the rows ``cand[i, :]`` of a ``store [N, D]`` (fp32, or fp16 with an
optional fp32 ``row_scale [N]``) and returns the best ``k`` of them in the project's total order (score descending,
id ascending: ``better()`` of ``atpu/topk.h``). A candidate's score has the bits ``sim_topk`` gives the same query
and row over the same store (the same MFMA, the same k order, the scale applied at the same place), so a shortlist
that holds every row makes the call the exact search, bit for bit. An id outside ``[0, N)`` is an empty slot: it is
never dereferenced, and a query with fewer than ``k`` live candidates is padded with ``(-inf, PAD_ID)``. The live
ids of one query must be distinct.

The store may live in pinned host memory (``torch.empty(..., pin_memory=True)``): the kernel then reads the
shortlisted rows over the link through the buffer's device-visible address, and nothing of the store is copied.

:func:`pq_scan_segments` builds the shortlist of a product-quantized corpus: the rows are cut into ``G`` segments of
``64 * ceil(N / (64 G))`` rows and the list is the ADC top-32 of each segment in the total order, which is what the
scan kernel leaves in its per-(query, split) workspace before the merge when it runs with ``splits = G``. The list
depends on ``(lut, codes, G)`` alone: not on the batch and not on a tuning heuristic. Segments are disjoint, so it
has no duplicates.
"""
from __future__ import annotations

from typing import Optional, Tuple, Union

import torch

from .._native import native, ptr, launch_stream
from ._util import check, same_device
from .pq import BLOCK_ROWS, PqCodes, _check_scan, pq_deinterleave, pq_interleave
from .search import MAX_K, MAX_ROWS, MAX_SPLITS, PAD_ID, _NO_ROW, _ivf_pad, sim_topk_ok

SEGMENT_LIST = 32  # entries a segment contributes: MAX_K, the scan kernel's longest list
MAX_CANDIDATES = SEGMENT_LIST * MAX_SPLITS


def candidates_ok(R: int) -> bool:
    return isinstance(R, int) and not isinstance(R, bool) and R % SEGMENT_LIST == 0 and SEGMENT_LIST <= R <= MAX_CANDIDATES


def segment_rows(N: int, G: int) -> int:
    """Rows of one of the ``G`` segments of ``N`` rows: whole 64-row code blocks."""
    return BLOCK_ROWS * -(-N // (BLOCK_ROWS * G))


def shortlist_rows(N: int, G: int) -> int:
    """Live entries of a query's shortlist: at most 32 per segment."""
    seg = segment_rows(N, G)
    return sum(min(SEGMENT_LIST, min(N, lo + seg) - lo) for lo in range(0, N, seg))


def _check_refine(q, store, cand, k, id_base, row_scale, chunks):
    check(isinstance(q, torch.Tensor) and isinstance(store, torch.Tensor) and q.dim() == 2 and store.dim() == 2
          and q.shape[1] == store.shape[1], "refine_topk: q [nq, D] and store [N, D]")
    check(q.dtype == torch.float32 and store.dtype in (torch.float32, torch.float16),
          "refine_topk: q must be fp32 and the store fp32 or fp16")
    check(isinstance(k, int) and not isinstance(k, bool) and sim_topk_ok(q.shape[1], k),
          f"refine_topk: unsupported shape D={q.shape[1]} k={k}")
    N = store.shape[0]
    check(1 <= N <= MAX_ROWS, "refine_topk: N must be in [1, 2^31 - 256]")
    check(isinstance(cand, torch.Tensor) and cand.dim() == 2 and cand.dtype == torch.int32
          and cand.shape[0] == q.shape[0] and candidates_ok(int(cand.shape[1])),
          "refine_topk: cand must be int32 [nq, R], R a multiple of 32 in [32, 8192]")
    step = cand.stride(1)
    check(step in (1, 2) and (cand.shape[0] <= 1 or cand.stride(0) == cand.shape[1] * step),
          "refine_topk: cand must be contiguous, or every other element of a contiguous buffer")
    check(q.is_contiguous() and store.is_contiguous(), "refine_topk: contiguous q and store")
    if row_scale is not None:
        check(store.dtype == torch.float16, "refine_topk: row_scale needs an fp16 store")
        check(isinstance(row_scale, torch.Tensor) and row_scale.dtype == torch.float32 and row_scale.shape == (N,)
              and row_scale.is_contiguous(), "refine_topk: row_scale must be a contiguous fp32 [N]")
    check(isinstance(id_base, int) and 0 <= id_base < 2 ** 61, "refine_topk: id_base must be in [0, 2^61)")
    check(chunks is None or (isinstance(chunks, int) and 1 <= chunks <= MAX_SPLITS),
          f"refine_topk: chunks must be in [1, {MAX_SPLITS}]")
    same_device(q, cand, row_scale)
    check(store.device == q.device or (q.is_cuda and not store.is_cuda and store.is_pinned()),
          "refine_topk: the store must be on q's device, or in pinned host memory for a device q")


def refine_topk_ref(q: torch.Tensor, store: torch.Tensor, cand: torch.Tensor, k: int, id_base: int = 0,
                    row_scale: Optional[torch.Tensor] = None, dtype=torch.float32
                    ) -> Tuple[torch.Tensor, torch.Tensor]:
    """PyTorch twin of :func:`refine_topk` in ``dtype`` math and the CPU path: the scores are ``sim_topk_ref``'s (the
    same product over the whole store, so that the same rows get the same bits), gathered at the candidates; two
    stable sorts give the total order."""
    _check_refine(q, store, cand, k, id_base, row_scale, None)
    N = store.shape[0]
    s = q.to(dtype) @ store.to(device=q.device, dtype=dtype).T
    if row_scale is not None:
        s = s * row_scale.to(dtype)
    live = (cand >= 0) & (cand < N)
    rows = torch.where(live, cand, torch.zeros_like(cand)).to(torch.int64)
    sc = torch.gather(s, 1, rows).masked_fill(~live, float("-inf"))  # by select
    rows = torch.where(live, rows, torch.full_like(rows, _NO_ROW))
    by_id = torch.sort(rows, dim=1, stable=True).indices
    s1, i1 = torch.gather(sc, 1, by_id), torch.gather(rows, 1, by_id)
    by_score = torch.sort(s1 + 0.0, dim=1, descending=True, stable=True).indices[:, :k]  # -0.0 + 0.0 = +0.0: they tie
    scores, ids = torch.gather(s1, 1, by_score), torch.gather(i1, 1, by_score)
    return _ivf_pad(scores, ids + int(id_base), ids == _NO_ROW)[:2]


def auto_chunks(nq: int, R: int, device: torch.device) -> int:
    """Workgroups per query: one per 128 candidates (a step of each of its 4 waves) until the grid holds about 8 per
    CU; past that the waves stream several steps each."""
    cus = torch.cuda.get_device_properties(device).multi_processor_count
    return max(1, min(MAX_SPLITS, -(-R // 128), 8 * cus // max(nq, 1)))


def refine_topk(q: torch.Tensor, store: torch.Tensor, cand: torch.Tensor, k: int, id_base: int = 0,
                row_scale: Optional[torch.Tensor] = None, chunks: Optional[int] = None
                ) -> Tuple[torch.Tensor, torch.Tensor]:
    """(scores ``[nq, k]`` fp32, ids ``[nq, k]`` int64 = ``id_base + row``) of the contiguous fp32 ``q [nq, D]``
    against the rows ``cand [nq, R]`` (int32) of the contiguous ``store [N, D]``: on ``q``'s device, or in pinned host
    memory. The result does not depend on ``chunks`` (tests and benches) or on the batch."""
    _check_refine(q, store, cand, k, id_base, row_scale, chunks)
    nq, D = q.shape
    N, R = store.shape[0], int(cand.shape[1])
    if not q.is_cuda or nq == 0:
        return refine_topk_ref(q, store, cand, k, id_base, row_scale)
    nat = native()
    P = nat.refine_chunks(R, chunks if chunks is not None else auto_chunks(nq, R, q.device))
    ws = torch.empty((nq, P, k, 2), dtype=torch.float32, device=q.device)
    scores = torch.empty((nq, k), dtype=torch.float32, device=q.device)
    ids = torch.empty((nq, k), dtype=torch.int64, device=q.device)
    stream = launch_stream(q)
    nat.refine_topk_partial(ptr(q), ptr(store), store.dtype == torch.float16, ptr(row_scale), ptr(cand),
                            int(cand.stride(1)), ptr(ws), nq, N, D, R, k, P, stream)
    nat.sim_topk_merge(ptr(ws), ptr(scores), ptr(ids), nq, P, k, k, int(id_base), stream)
    return _ivf_pad(scores, ids, ids == int(id_base) + _NO_ROW)[:2]  # the merge's empty entries


def _check_segments(lut, codes, G):
    check(isinstance(G, int) and not isinstance(G, bool) and 1 <= G <= MAX_SPLITS,
          f"pq_scan_segments: G must be in [1, {MAX_SPLITS}]")
    return _check_scan(lut, codes, MAX_K, 0, G)


def pq_scan_segments_ref(lut: torch.Tensor, codes: Union[torch.Tensor, PqCodes], G: int) -> torch.Tensor:
    """PyTorch twin of :func:`pq_scan_segments` and the CPU path: ``pq_scan_topk_ref``'s scores, the stable sort per
    segment."""
    N, M = _check_segments(lut, codes, G)
    rows = (pq_deinterleave(codes) if isinstance(codes, PqCodes) else codes).long()
    s = lut[:, 0, rows[:, 0]]
    for m in range(1, M):
        s = s + lut[:, m, rows[:, m]]
    nq, seg = lut.shape[0], segment_rows(N, G)
    P = -(-N // seg)
    flat = torch.full((nq, P * seg), float("-inf"), dtype=s.dtype, device=s.device)  # seg >= 64 > 32 columns each
    flat[:, :N] = s
    order = torch.sort(flat.view(nq, P, seg) + 0.0, dim=2, descending=True, stable=True).indices[:, :, :SEGMENT_LIST]
    ids = order + (torch.arange(P, device=s.device) * seg)[None, :, None]
    ids = torch.where(ids < N, ids, torch.full_like(ids, _NO_ROW))
    return ids.to(torch.int32).reshape(nq, P * SEGMENT_LIST)


def pq_scan_segments(lut: torch.Tensor, codes: Union[torch.Tensor, PqCodes], G: int) -> torch.Tensor:
    """int32 ``[nq, 32 P]``, ``P = ceil(N / segment_rows(N, G)) <= G``: per segment the 32 rows with the largest ADC
    score in the total order (row ids of the slice; empty slots hold the no-row id ``0x7fffffff``). On the GPU the
    result is a view of the scan kernel's un-merged workspace (every other element), which :func:`refine_topk`
    reads as it lies."""
    N, M = _check_segments(lut, codes, G)
    nq = lut.shape[0]
    if not lut.is_cuda or nq == 0:
        return pq_scan_segments_ref(lut, codes, G)
    pc = codes if isinstance(codes, PqCodes) else pq_interleave(codes)
    nat = native()
    P = nat.pq_scan_splits(N, G)
    ws = torch.empty((nq, P, SEGMENT_LIST, 2), dtype=torch.float32, device=lut.device)
    nat.pq_scan_partial(ptr(lut), ptr(pc.data), ptr(ws), nq, N, M, SEGMENT_LIST, P, launch_stream(lut))
    return ws.view(torch.int32).view(nq, P * SEGMENT_LIST, 2)[:, :, 1]
