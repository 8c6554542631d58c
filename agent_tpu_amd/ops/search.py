"""Top-k similarity search over fp32 or fp16 vectors: a GEMM whose score matrix is never written.

``sim_topk`` (``csrc/kernels/sim_topk.hip``) returns, for every query row of ``q [nq, D]``, the
``kk = min(k, N)`` rows of the corpus ``c [N, D]`` with the largest dot product:

    scores[i, j] = dot(q[i], c[ids[i, j] - id_base])

ordered by score descending, then id ascending: a total order (``better()`` of ``atpu/topk.h``;
``+0.0`` and ``-0.0`` tie). The kernel is metric-agnostic: cosine similarity is the same call on
normalised rows.

Every (query, row) score is ONE fp32 accumulator fed by the exact f32 MFMA in a column order that
depends on ``D`` alone, and the corpus splits' partial lists ``[nq, P, k]`` merge in the same
total order, so the result has the same bits for every ``splits`` value and every query batch.
``splits=None`` picks ``P`` from ``N`` and the CU count; the argument exists for tests and benches.

A ``float16`` corpus (``csrc/kernels/sim_topk_f16.hip``) keeps all of that at half the bytes: an
fp16 value widens to fp32 exactly, so the score is the exact fp32 dot product of ``q`` and the
stored values, fed to the same MFMA. An optional fp32 ``row_scale [N]`` multiplies the finished
accumulator once, before the ranking:

    scores[i, j] = dot(q[i], float(c[r])) * row_scale[r],   r = ids[i, j] - id_base

which is cosine similarity over rows stored as they are (``row_scale = 1 / ||c[r]||``).
"""
from __future__ import annotations

from typing import Optional, Tuple

import torch

from .._native import native, ptr, launch_stream
from ._util import check, same_device

MAX_K = 32
MAX_SPLITS = 256  # kSimMaxSplits
MAX_ROWS = 2 ** 31 - 256


def sim_topk_ok(D: int, k: int) -> bool:
    """Shapes the kernel takes: D a multiple of 64 from 64 to 1024 (``pool_embed_ok``'s H), k in 1..32."""
    return D % 64 == 0 and 64 <= D <= 1024 and 1 <= k <= MAX_K


def sim_topk_ref(q: torch.Tensor, c: torch.Tensor, k: int, id_base: int = 0, dtype=torch.float32,
                 row_scale: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """PyTorch twin in ``dtype`` math -> (scores ``[nq, kk]`` of ``dtype``, ids ``[nq, kk]`` int64); also the
    CPU path. Two stable sorts give the (score desc, id asc) order: ``torch.topk`` promises no tie order."""
    check(q.dim() == 2 and c.dim() == 2 and q.shape[1] == c.shape[1], "sim_topk: q [nq, D] and c [N, D]")
    check(k >= 1 and c.shape[0] >= 1, "sim_topk: k and N must be >= 1")
    N = c.shape[0]
    kk = min(k, N)
    s = q.to(dtype) @ c.to(dtype).T  # [nq, N]; columns are already in ascending id
    if row_scale is not None:
        check(row_scale.shape == (N,), "sim_topk: row_scale must be [N]")
        s = s * row_scale.to(dtype)
    order = torch.sort(s + 0.0, dim=1, descending=True, stable=True).indices[:, :kk]  # -0.0 + 0.0 = +0.0: they tie
    return torch.gather(s, 1, order), order.to(torch.int64) + int(id_base)


def auto_splits(N: int, nq: int, device: torch.device) -> int:
    """One workgroup per (split, tile of 32 queries): enough splits to put one on every CU."""
    cus = torch.cuda.get_device_properties(device).multi_processor_count
    return max(1, min(MAX_SPLITS, cus // ((nq + 31) // 32)))


def sim_topk(q: torch.Tensor, c: torch.Tensor, k: int, id_base: int = 0, splits: Optional[int] = None,
             row_scale: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """(scores ``[nq, kk]`` fp32, ids ``[nq, kk]`` int64), ``kk = min(k, N)``, of the contiguous fp32
    ``q [nq, D]`` against the contiguous fp32 or fp16 ``c [N, D]``; ``row_scale`` (fp32 ``[N]``,
    contiguous) goes with an fp16 ``c`` only."""
    check(q.dim() == 2 and c.dim() == 2 and q.shape[1] == c.shape[1], "sim_topk: q [nq, D] and c [N, D]")
    check(q.dtype == torch.float32 and c.dtype in (torch.float32, torch.float16),
          "sim_topk: q must be fp32 and c fp32 or fp16")
    half = c.dtype == torch.float16
    check(row_scale is None or half, "sim_topk: row_scale needs an fp16 c")
    if row_scale is not None:
        check(isinstance(row_scale, torch.Tensor) and row_scale.dtype == torch.float32
              and row_scale.shape == (c.shape[0],) and row_scale.is_contiguous(),
              "sim_topk: row_scale must be a contiguous fp32 [N]")
        same_device(c, row_scale)
    check(isinstance(k, int) and not isinstance(k, bool), "sim_topk: k must be an int")
    nq, D = q.shape
    N = c.shape[0]
    check(sim_topk_ok(D, k), f"sim_topk: unsupported shape D={D} k={k}")
    check(1 <= N <= MAX_ROWS, "sim_topk: N must be in [1, 2^31 - 256]")
    check(q.is_contiguous() and c.is_contiguous(), "sim_topk: contiguous tensors")
    check(splits is None or (isinstance(splits, int) and 1 <= splits <= MAX_SPLITS),
          f"sim_topk: splits must be in [1, {MAX_SPLITS}]")
    same_device(q, c)
    kk = min(k, N)
    if nq == 0:
        return (torch.empty((0, kk), dtype=torch.float32, device=q.device),
                torch.empty((0, kk), dtype=torch.int64, device=q.device))
    if not q.is_cuda:
        return sim_topk_ref(q, c, k, id_base, row_scale=row_scale)
    nat = native()
    P = nat.sim_topk_splits(N, splits if splits is not None else auto_splits(N, nq, q.device))
    ws = torch.empty((nq, P, k, 2), dtype=torch.float32, device=q.device)
    scores = torch.empty((nq, kk), dtype=torch.float32, device=q.device)
    ids = torch.empty((nq, kk), dtype=torch.int64, device=q.device)
    stream = launch_stream(q)
    if half:
        nat.sim_topk_partial_f16(ptr(q), ptr(c), ptr(row_scale) if row_scale is not None else 0, ptr(ws), nq, N, D, k,
                                 P, stream)
    else:
        nat.sim_topk_partial(ptr(q), ptr(c), ptr(ws), nq, N, D, k, P, stream)
    nat.sim_topk_merge(ptr(ws), ptr(scores), ptr(ids), nq, P, k, kk, int(id_base), stream)
    return scores, ids
