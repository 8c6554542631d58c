"""IVF-PQ (IVFADC): coarse clusters and product-quantization codes of the residual ``x - centroid[label]``.

The index is the corpus sorted by cluster, as ``sim_topk_ivf``'s: ``row_ids [N]`` int32 (the original row of a sorted
row, ascending inside a cluster) and ``offsets [K + 1]`` int32, with the sorted rows' residual codes in place of the
vectors: row-major ``[N, M]`` uint8 or one interleaved :class:`PqCodes` image over the sorted rows (clusters are not
padded to 64 rows). Query ``i`` scans the ``nprobe`` clusters whose centroids score best against it
(``sim_topk(q, centroids, nprobe)``), and a row's score is

    score(i, r) = (lut[i, 0, code(r, 0)] + ... + lut[i, M-1, code(r, M-1)]) + coarse(i, cluster(r))

``lut = pq_lut(q, codebooks)`` over the residual codebooks: for inner products the table depends on the query only,
so one table serves every probed cluster. ``coarse`` is ``dot(q, centroid)`` in a fixed fp32 order
(:func:`pq_coarse`): columns ``64 s + 4 j + e`` form chain ``j`` of 16 (``s`` ascending, then ``e``; separately
rounded products, no FMA), and the 16 chains are added pairwise: neighbours, then pairs, quads and halves. The probe's
own score is not used: it comes out of the MFMA, whose bits no PyTorch twin has.

A score therefore depends on the query, the centroids, the codebooks and the row's codes only: the same bits for
every batch, every ``splits`` value and every way the rows are cut into slices. The order is (score desc, original
id asc). The ``_ref`` twins do the same operations one column at a time and are the CPU path.
"""
from __future__ import annotations

from typing import Optional, Tuple, Union

import torch

from .._native import native, ptr, launch_stream
from ._util import check, same_device
from .pq import (BLOCK_ROWS, PqCodes, _check_books, _check_encode, pq_deinterleave, pq_encode_ref,
                 pq_interleave, pq_lut, pq_lut_ref)
from .search import (IVF_MAX_CLUSTERS, MAX_K, MAX_ROWS, MAX_SPLITS, PAD_ID, _NO_ROW, _ivf_pad, sim_topk, sim_topk_ok,
                     sim_topk_ref)


# ------------------------------------------------------------------------------------------- the encoder
def _check_residual(x, labels, centroids, codebooks, bias):
    M = _check_encode(x, codebooks, bias)
    check(isinstance(centroids, torch.Tensor) and centroids.dim() == 2 and centroids.dtype == torch.float32
          and centroids.shape[1] == x.shape[1] and 1 <= centroids.shape[0] <= IVF_MAX_CLUSTERS
          and centroids.is_contiguous(), "pq_encode_residual: centroids must be a contiguous fp32 [K, D], K in [1, 4096]")
    check(isinstance(labels, torch.Tensor) and labels.dtype == torch.int32 and labels.shape == (x.shape[0],)
          and labels.is_contiguous(), "pq_encode_residual: labels must be a contiguous int32 [n]")
    same_device(x, labels, centroids)
    return M


def pq_encode_residual_ref(x: torch.Tensor, labels: torch.Tensor, centroids: torch.Tensor, codebooks: torch.Tensor,
                           bias: torch.Tensor) -> torch.Tensor:
    """PyTorch twin of :func:`pq_encode_residual` and the CPU path."""
    _check_residual(x, labels, centroids, codebooks, bias)
    lab = labels.to(torch.int64).clamp(0, centroids.shape[0] - 1)
    return pq_encode_ref((x - centroids[lab]).contiguous(), codebooks, bias)


def pq_encode_residual(x: torch.Tensor, labels: torch.Tensor, centroids: torch.Tensor, codebooks: torch.Tensor,
                       bias: torch.Tensor) -> torch.Tensor:
    """uint8 ``[n, M]``: ``pq_encode`` of the residuals ``x - centroids[labels]`` (one fp32 subtract per column),
    which the kernel forms in registers and never writes. Labels outside ``[0, K)`` are clamped."""
    M = _check_residual(x, labels, centroids, codebooks, bias)
    if not x.is_cuda or x.shape[0] == 0:
        return pq_encode_residual_ref(x, labels, centroids, codebooks, bias)
    codes = torch.empty((x.shape[0], M), dtype=torch.uint8, device=x.device)
    native().pq_encode_residual(ptr(x), ptr(labels), ptr(centroids), ptr(codebooks), ptr(bias), ptr(codes), x.shape[0],
                                x.shape[1], M, centroids.shape[0], launch_stream(x))
    return codes


# --------------------------------------------------------------------------------------- the coarse term
def _check_coarse(q, centroids, probes):
    check(q.dim() == 2 and centroids.dim() == 2 and q.shape[1] == centroids.shape[1] and q.dtype == torch.float32
          and centroids.dtype == torch.float32 and q.is_contiguous() and centroids.is_contiguous(),
          "pq_coarse: q [nq, D] and centroids [K, D] must be contiguous fp32")
    check(sim_topk_ok(q.shape[1], 1) and 1 <= centroids.shape[0] <= IVF_MAX_CLUSTERS,
          "pq_coarse: D must be a multiple of 64 in [64, 1024] and K in [1, 4096]")
    check(isinstance(probes, torch.Tensor) and probes.dtype == torch.int64 and probes.dim() == 2
          and probes.shape[0] == q.shape[0] and 1 <= probes.shape[1] <= min(MAX_K, centroids.shape[0])
          and probes.is_contiguous(), "pq_coarse: probes must be a contiguous int64 [nq, nprobe], nprobe <= min(32, K)")
    same_device(q, centroids, probes)


def pq_coarse_ref(q: torch.Tensor, centroids: torch.Tensor, probes: torch.Tensor) -> torch.Tensor:
    """PyTorch twin of :func:`pq_coarse` and the CPU path: the 16 chains one column at a time, then the four rounds
    of pairwise adds."""
    _check_coarse(q, centroids, probes)
    nq, D = q.shape
    c = centroids[probes.clamp(0, centroids.shape[0] - 1)]  # [nq, nprobe, D]
    qs, cs = q.view(nq, 1, D // 64, 16, 4), c.view(nq, probes.shape[1], D // 64, 16, 4)
    acc = None
    for s in range(D // 64):
        for e in range(4):
            p = qs[:, :, s, :, e] * cs[:, :, s, :, e]
            acc = p if acc is None else acc + p
    for _ in range(4):
        acc = acc[..., 0::2] + acc[..., 1::2]
    return acc[..., 0].contiguous()


def pq_coarse(q: torch.Tensor, centroids: torch.Tensor, probes: torch.Tensor) -> torch.Tensor:
    """fp32 ``[nq, nprobe]``: ``dot(q[i], centroids[probes[i, s]])`` in the module's fixed order."""
    _check_coarse(q, centroids, probes)
    if not q.is_cuda or q.shape[0] == 0:
        return pq_coarse_ref(q, centroids, probes)
    out = torch.empty(probes.shape, dtype=torch.float32, device=q.device)
    native().pq_coarse(ptr(q), ptr(centroids), ptr(probes), ptr(out), q.shape[0], q.shape[1], centroids.shape[0],
                       probes.shape[1], launch_stream(q))
    return out


# ----------------------------------------------------------------------------------------------- search
def _check_ivfpq(q, codebooks, codes, row_ids, offsets, centroids, k, nprobe, id_base, splits):
    check(isinstance(q, torch.Tensor) and q.dim() == 2 and q.dtype == torch.float32 and q.is_contiguous(),
          "sim_topk_ivfpq: q must be a contiguous fp32 [nq, D]")
    M, _ = _check_books(codebooks, q.shape[1], "sim_topk_ivfpq")
    check(isinstance(centroids, torch.Tensor) and centroids.dim() == 2 and centroids.dtype == torch.float32
          and centroids.shape[1] == q.shape[1] and centroids.is_contiguous(),
          "sim_topk_ivfpq: centroids must be a contiguous fp32 [K, D]")
    K = centroids.shape[0]
    check(isinstance(k, int) and not isinstance(k, bool) and sim_topk_ok(q.shape[1], k),
          f"sim_topk_ivfpq: unsupported shape D={q.shape[1]} k={k}")
    check(1 <= K <= IVF_MAX_CLUSTERS, "sim_topk_ivfpq: K must be in [1, 4096]")
    check(isinstance(nprobe, int) and not isinstance(nprobe, bool) and 1 <= nprobe <= min(MAX_K, K),
          "sim_topk_ivfpq: nprobe must be in [1, min(32, K)]")
    if isinstance(codes, PqCodes):
        n, data = codes.rows, codes.data
        check(isinstance(n, int) and codes.M == M and data.dtype == torch.uint8 and data.is_contiguous()
              and data.shape == ((n + BLOCK_ROWS - 1) // BLOCK_ROWS, M // 4, BLOCK_ROWS, 4),
              "sim_topk_ivfpq: PqCodes must be a contiguous uint8 [ceil(rows / 64), M / 4, 64, 4] of the codebooks' M")
    else:
        check(isinstance(codes, torch.Tensor) and codes.dim() == 2 and codes.dtype == torch.uint8
              and codes.shape[1] == M and codes.is_contiguous(),
              "sim_topk_ivfpq: codes must be a contiguous uint8 [n, M] of the codebooks' M (or a PqCodes)")
        n, data = codes.shape[0], codes
    check(0 <= n <= MAX_ROWS, "sim_topk_ivfpq: n must be in [0, 2^31 - 256]")
    check(isinstance(row_ids, torch.Tensor) and isinstance(offsets, torch.Tensor) and row_ids.dtype == torch.int32
          and row_ids.shape == (n,) and offsets.dtype == torch.int32 and offsets.shape == (K + 1,)
          and row_ids.is_contiguous() and offsets.is_contiguous(),
          "sim_topk_ivfpq: row_ids must be a contiguous int32 [n] and offsets a contiguous int32 [K + 1]")
    check(isinstance(id_base, int) and 0 <= id_base < 2 ** 61, "sim_topk_ivfpq: id_base must be in [0, 2^61)")
    check(splits is None or (isinstance(splits, int) and not isinstance(splits, bool) and 1 <= splits <= MAX_SPLITS),
          f"sim_topk_ivfpq: splits must be in [1, {MAX_SPLITS}]")
    same_device(q, codebooks, data, row_ids, offsets, centroids)
    return n, M, K


def sim_topk_ivfpq_ref(q: torch.Tensor, codebooks: torch.Tensor, codes: Union[torch.Tensor, PqCodes],
                       row_ids: torch.Tensor, offsets: torch.Tensor, centroids: torch.Tensor, k: int, nprobe: int,
                       id_base: int = 0) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """PyTorch twin of :func:`sim_topk_ivfpq` and the CPU path: the ``[nq, n]`` scores one sub-space at a time, the
    coarse term of the row's cluster added last, the rows outside the probed clusters masked by select, then the two
    stable sorts of ``sim_topk_ref`` over the rows put back in their original order."""
    n, M, K = _check_ivfpq(q, codebooks, codes, row_ids, offsets, centroids, k, nprobe, id_base, None)
    nq = q.shape[0]
    if nq == 0 or n == 0:
        return (torch.full((nq, k), float("-inf"), dtype=torch.float32, device=q.device),
                torch.full((nq, k), PAD_ID, dtype=torch.int64, device=q.device),
                torch.zeros((nq,), dtype=torch.int64, device=q.device))
    probes = sim_topk_ref(q, centroids, nprobe)[1].contiguous()  # [nq, nprobe]
    coarse = pq_coarse_ref(q, centroids, probes)
    lut = pq_lut_ref(q, codebooks)
    rows = (pq_deinterleave(codes) if isinstance(codes, PqCodes) else codes).long()
    s = lut[:, 0, rows[:, 0]]
    for m in range(1, M):
        s = s + lut[:, m, rows[:, m]]
    sizes = (offsets[1:] - offsets[:-1]).to(torch.int64)
    cluster = torch.repeat_interleave(torch.arange(K, device=q.device), sizes, output_size=n)  # of a sorted row
    probed = torch.zeros((nq, K), dtype=torch.bool, device=q.device).scatter_(1, probes, True)
    by_cluster = torch.zeros((nq, K), dtype=torch.float32, device=q.device).scatter_(1, probes, coarse)
    s = (s + by_cluster[:, cluster]).masked_fill(~probed[:, cluster], float("-inf"))
    orig = row_ids.to(torch.int64)
    so = torch.empty_like(s)
    so[:, orig] = s  # columns in ascending original row
    allowed = torch.empty_like(probed[:, cluster])
    allowed[:, orig] = probed[:, cluster]
    order = torch.sort(so + 0.0, dim=1, descending=True, stable=True).indices[:, :k]
    scores, ids = torch.gather(so, 1, order), order.to(torch.int64) + int(id_base)
    empty = ~torch.gather(allowed, 1, order)
    if scores.shape[1] < k:  # fewer rows than k
        pad = k - scores.shape[1]
        scores = torch.cat([scores, scores.new_full((nq, pad), float("-inf"))], 1)
        ids = torch.cat([ids, ids.new_full((nq, pad), PAD_ID)], 1)
        empty = torch.cat([empty, empty.new_ones((nq, pad))], 1)
    return _ivf_pad(scores, ids, empty)


def ivfpq_splits(nq: int, nprobe: int, K: int, n: int, device: torch.device) -> int:
    """Splits per query (one workgroup per (query, split)): enough workgroups for the CUs at small ``nq``, no more
    than the average query has 32-block steps (one step of the workgroup's 8 waves x 4 blocks), at most 256. A
    first guess that rests on no measurement; the result does not depend on it."""
    cus = torch.cuda.get_device_properties(device).multi_processor_count
    blocks = nprobe * max(1, -(-n // (BLOCK_ROWS * K)))  # of the average query: nprobe clusters of average size
    return max(1, min(MAX_SPLITS, -(-cus // nq), blocks // 32))


def sim_topk_ivfpq(q: torch.Tensor, codebooks: torch.Tensor, codes: Union[torch.Tensor, PqCodes],
                   row_ids: torch.Tensor, offsets: torch.Tensor, centroids: torch.Tensor, k: int, nprobe: int,
                   id_base: int = 0, splits: Optional[int] = None
                   ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """(scores ``[nq, k]`` fp32, ids ``[nq, k]`` int64, counts ``[nq]`` int64) of the fp32 ``q [nq, D]`` against an
    IVF-PQ index (``csrc/kernels/pq_ivf.hip``): the ``sim_topk`` probe of the ``centroids [K, D]``, ``pq_coarse``,
    ``pq_lut`` against the residual ``codebooks [M, 256, dsub]``, the query-stationary scan of the probed clusters'
    codes, and ``sim_topk_merge``. ``codes``: the sorted rows' codes, row-major uint8 ``[n, M]`` (interleaved here,
    on every call) or a :class:`PqCodes`. ``ids = id_base + original row`` in the (score desc, id asc) order; the
    columns past ``counts[i]`` (fewer than ``k`` rows in the probed clusters) hold ``(-inf, PAD_ID)``. The result
    does not depend on ``splits`` (tests and benches) or on the batch."""
    n, M, K = _check_ivfpq(q, codebooks, codes, row_ids, offsets, centroids, k, nprobe, id_base, splits)
    nq = q.shape[0]
    if not q.is_cuda or nq == 0 or n == 0:
        return sim_topk_ivfpq_ref(q, codebooks, codes, row_ids, offsets, centroids, k, nprobe, id_base)
    pc = codes if isinstance(codes, PqCodes) else pq_interleave(codes)
    nat = native()
    probes = sim_topk(q, centroids, nprobe)[1]
    coarse = pq_coarse(q, centroids, probes)
    lut = pq_lut(q, codebooks)
    S = splits if splits is not None else ivfpq_splits(nq, nprobe, K, n, q.device)
    ws = torch.empty((nq, S, k, 2), dtype=torch.float32, device=q.device)
    scores = torch.empty((nq, k), dtype=torch.float32, device=q.device)
    ids = torch.empty((nq, k), dtype=torch.int64, device=q.device)
    stream = launch_stream(q)
    nat.pq_scan_ivf_partial(ptr(lut), ptr(pc.data), ptr(row_ids), ptr(offsets), ptr(probes), ptr(coarse), ptr(ws), nq,
                            n, M, k, K, nprobe, S, stream)
    nat.sim_topk_merge(ptr(ws), ptr(scores), ptr(ids), nq, S, k, k, int(id_base), stream)
    return _ivf_pad(scores, ids, ids == int(id_base) + _NO_ROW)  # the merge's empty entries: (-inf, id_base + kNoRow)
