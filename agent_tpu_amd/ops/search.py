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

A :class:`RowMask` (``csrc/kernels/sim_topk_masked.hip``) restricts the search to the rows whose
bit is set: ``words [ceil(N / 32)]`` int32, bit ``b`` of word ``w`` = row ``32 w + b``, one word per
32-row wave step of the kernel; ``live`` lists the non-zero words, and only those steps are read.
The filter sits in the kernel's epilogue, and a score keeps the bits it has without a mask, so
``sim_topk(q, c, k, mask=m)`` equals ``sim_topk(q, c[rows], k)`` over the allowed rows with the ids
mapped back, bit for bit, at ``kk = min(k, m.count)`` columns. :func:`row_mask_from_ids` and
:func:`row_mask_from_labels` build masks on the device (``*_ref``: their PyTorch twins).

:func:`sim_topk_ivf` (``csrc/kernels/sim_topk_ivf.hip``) is the approximate form: the corpus sorted by
k-means cluster, and every query scored against the rows of the ``nprobe`` clusters nearest to it only, a
different row set per query. The scores stay exact fp32 dot products with ``sim_topk``'s bits and the ids are
the original rows, so probing every cluster is the exact search bit for bit.
"""
from __future__ import annotations

from typing import NamedTuple, Optional, Sequence, Tuple, Union

import torch

from .._native import native, ptr, launch_stream
from ._util import check, same_device

MAX_K = 32
MAX_SPLITS = 256  # kSimMaxSplits
MAX_ROWS = 2 ** 31 - 256


def sim_topk_ok(D: int, k: int) -> bool:
    """Shapes the kernel takes: D a multiple of 64 from 64 to 1024 (``pool_embed_ok``'s H), k in 1..32."""
    return D % 64 == 0 and 64 <= D <= 1024 and 1 <= k <= MAX_K


class RowMask(NamedTuple):
    """The rows a filtered ``sim_topk`` may return (the module docstring has the layout)."""
    words: torch.Tensor  # [ceil(rows / 32)] int32: bit b of word w = row 32 w + b; bits at or past rows are ignored
    live: torch.Tensor  # int32: the indices of the non-zero words, ascending
    rows: int  # N of the corpus slice the mask is for
    count: int  # set bits below rows


def mask_words(rows: int) -> int:
    return (rows + 31) // 32


def _finish_mask(words: torch.Tensor, rows: int, count: int) -> RowMask:
    live = torch.nonzero(words).flatten().to(torch.int32)  # plumbing: once per mask
    return RowMask(words, live, int(rows), int(count))


def row_mask_bits(mask: RowMask) -> torch.Tensor:
    """bool ``[rows]`` of the mask's words (on their device)."""
    sh = torch.arange(32, device=mask.words.device, dtype=torch.int32)
    return ((mask.words[:, None] >> sh) & 1).flatten()[:mask.rows].bool()


def row_mask_from_bits(bits: torch.Tensor) -> RowMask:
    """The mask of a bool ``[N]`` tensor, packed with PyTorch on its device (tests, benches, CPU)."""
    check(bits.dim() == 1 and bits.dtype == torch.bool and bits.numel() >= 1, "row_mask: bits must be a bool [N]")
    N = bits.numel()
    b = torch.zeros(mask_words(N) * 32, dtype=torch.int64, device=bits.device)
    b[:N] = bits
    w = (b.view(-1, 32) << torch.arange(32, device=bits.device)).sum(1)  # < 2^32
    words = torch.where(w >= 2 ** 31, w - 2 ** 32, w).to(torch.int32)
    return _finish_mask(words, N, int(bits.sum()))


def _ids_tensor(ids, device) -> torch.Tensor:
    t = ids if isinstance(ids, torch.Tensor) else torch.tensor(list(ids), dtype=torch.int64)
    check(t.dim() == 1 and t.dtype == torch.int64, "row_mask_from_ids: ids must be a 1-D int64 tensor or a list of ints")
    return t.to(device).contiguous()


def row_mask_from_ids_ref(ids: Union[torch.Tensor, Sequence[int]], N: int, base: int = 0, exclude: bool = False,
                          device: Union[str, torch.device] = "cpu") -> RowMask:
    """PyTorch twin of :func:`row_mask_from_ids`."""
    check(isinstance(N, int) and 1 <= N <= MAX_ROWS, "row_mask_from_ids: N must be in [1, 2^31 - 256]")
    t = _ids_tensor(ids, torch.device(device))
    bits = torch.zeros(N, dtype=torch.bool, device=t.device)
    t = t[(t >= base) & (t < base + N)] - base
    bits[t] = True
    return row_mask_from_bits(~bits if exclude else bits)


def row_mask_from_ids(ids: Union[torch.Tensor, Sequence[int]], N: int, base: int = 0, exclude: bool = False,
                      device: Union[str, torch.device, None] = None) -> RowMask:
    """The mask of a slice of ``N`` rows that starts at corpus row ``base``: the rows ``id - base`` of the
    ``ids`` in ``[base, base + N)`` (duplicates and other slices' ids are skipped), or with ``exclude``
    every other row. ``device`` defaults to the ids tensor's (CPU for a list)."""
    check(isinstance(N, int) and 1 <= N <= MAX_ROWS, "row_mask_from_ids: N must be in [1, 2^31 - 256]")
    check(isinstance(base, int) and 0 <= base < 2 ** 62, "row_mask_from_ids: base must be in [0, 2^62)")
    dev = torch.device(device) if device is not None else (ids.device if isinstance(ids, torch.Tensor)
                                                          else torch.device("cpu"))
    if dev.type != "cuda":
        return row_mask_from_ids_ref(ids, N, base, exclude, dev)
    t = _ids_tensor(ids, dev)
    words = torch.empty(mask_words(N), dtype=torch.int32, device=dev)
    count = torch.empty(1, dtype=torch.int64, device=dev)
    native().row_mask_from_ids(ptr(t) if t.numel() else 0, t.numel(), int(base), N, bool(exclude), ptr(words),
                               ptr(count), launch_stream(words))
    return _finish_mask(words, N, int(count.item()))


def _label_args(labels, values, lo, hi):
    check(isinstance(labels, torch.Tensor) and labels.dim() == 1 and labels.dtype == torch.int64
          and 1 <= labels.numel() <= MAX_ROWS and labels.is_contiguous(),
          "row_mask_from_labels: labels must be a contiguous 1-D int64 tensor of 1 .. 2^31 - 256 rows")
    check((values is None) != (lo is None and hi is None) and (lo is None) == (hi is None),
          "row_mask_from_labels: give values, or lo and hi")
    i64 = lambda x: isinstance(x, int) and not isinstance(x, bool) and -2 ** 63 <= x < 2 ** 63  # noqa: E731
    if values is not None:
        vals = sorted(set(values.tolist() if isinstance(values, torch.Tensor) else values))
        check(1 <= len(vals) <= 256 and all(i64(v) for v in vals), "row_mask_from_labels: 1 to 256 int64 values")
        return vals, 0, 0
    check(i64(lo) and i64(hi), "row_mask_from_labels: lo and hi must be int64 integers")
    return None, lo, hi


def row_mask_from_labels_ref(labels: torch.Tensor, values=None, lo: Optional[int] = None,
                             hi: Optional[int] = None) -> RowMask:
    """PyTorch twin of :func:`row_mask_from_labels`."""
    vals, lo, hi = _label_args(labels, values, lo, hi)
    if vals is not None:
        bits = torch.isin(labels, torch.tensor(vals, dtype=torch.int64, device=labels.device))
    else:
        bits = (labels >= lo) & (labels <= hi)
    return row_mask_from_bits(bits)


def row_mask_from_labels(labels: torch.Tensor, values=None, lo: Optional[int] = None,
                         hi: Optional[int] = None) -> RowMask:
    """The mask of the rows whose int64 label is one of ``values`` (1 to 256 of them), or lies in
    ``[lo, hi]`` (both inclusive), on the labels' device."""
    if not (isinstance(labels, torch.Tensor) and labels.is_cuda):
        return row_mask_from_labels_ref(labels, values, lo, hi)
    vals, lo, hi = _label_args(labels, values, lo, hi)
    N = labels.numel()
    words = torch.empty(mask_words(N), dtype=torch.int32, device=labels.device)
    count = torch.empty(1, dtype=torch.int64, device=labels.device)
    vt = torch.tensor(vals, dtype=torch.int64).to(labels.device) if vals is not None else None
    native().row_mask_from_labels(ptr(labels), N, ptr(vt) if vt is not None else 0, len(vals) if vals else 0, lo, hi,
                                  ptr(words), ptr(count), launch_stream(labels))
    return _finish_mask(words, N, int(count.item()))


def _check_mask(mask: RowMask, c: torch.Tensor) -> None:
    N = c.shape[0]
    check(isinstance(mask, RowMask), "sim_topk: mask must be a RowMask")
    check(isinstance(mask.rows, int) and mask.rows == N, "sim_topk: the mask is for another number of rows")
    check(isinstance(mask.words, torch.Tensor) and mask.words.dtype == torch.int32
          and mask.words.shape == (mask_words(N),) and mask.words.is_contiguous(),
          "sim_topk: mask.words must be a contiguous int32 [ceil(N / 32)]")
    check(isinstance(mask.live, torch.Tensor) and mask.live.dtype == torch.int32 and mask.live.dim() == 1
          and mask.live.numel() <= mask_words(N) and mask.live.is_contiguous(),
          "sim_topk: mask.live must be a contiguous int32 list of at most ceil(N / 32) words")
    check(isinstance(mask.count, int) and not isinstance(mask.count, bool) and 0 <= mask.count <= N
          and (mask.count == 0) == (mask.live.numel() == 0), "sim_topk: mask.count must be the number of allowed rows")
    same_device(c, mask.words)
    same_device(c, mask.live)


def sim_topk_ref(q: torch.Tensor, c: torch.Tensor, k: int, id_base: int = 0, dtype=torch.float32,
                 row_scale: Optional[torch.Tensor] = None, mask: Optional[RowMask] = None
                 ) -> Tuple[torch.Tensor, torch.Tensor]:
    """PyTorch twin in ``dtype`` math -> (scores ``[nq, kk]`` of ``dtype``, ids ``[nq, kk]`` int64); also the
    CPU path. Two stable sorts give the (score desc, id asc) order: ``torch.topk`` promises no tie order.
    With a ``mask`` the scores of the other rows are ``-inf`` before the sorts and ``kk = min(k, mask.count)``."""
    check(q.dim() == 2 and c.dim() == 2 and q.shape[1] == c.shape[1], "sim_topk: q [nq, D] and c [N, D]")
    check(k >= 1 and c.shape[0] >= 1, "sim_topk: k and N must be >= 1")
    N = c.shape[0]
    kk = min(k, N)
    s = q.to(dtype) @ c.to(dtype).T  # [nq, N]; columns are already in ascending id
    if row_scale is not None:
        check(row_scale.shape == (N,), "sim_topk: row_scale must be [N]")
        s = s * row_scale.to(dtype)
    if mask is not None:
        _check_mask(mask, c)
        kk = min(k, mask.count)
        s = s.masked_fill(~row_mask_bits(mask), float("-inf"))  # by select: a NaN in a masked row cannot leak
    order = torch.sort(s + 0.0, dim=1, descending=True, stable=True).indices[:, :kk]  # -0.0 + 0.0 = +0.0: they tie
    return torch.gather(s, 1, order), order.to(torch.int64) + int(id_base)


def auto_splits(N: int, nq: int, device: torch.device) -> int:
    """One workgroup per (split, tile of 32 queries): enough splits to put one on every CU."""
    cus = torch.cuda.get_device_properties(device).multi_processor_count
    return max(1, min(MAX_SPLITS, cus // ((nq + 31) // 32)))


def sim_topk(q: torch.Tensor, c: torch.Tensor, k: int, id_base: int = 0, splits: Optional[int] = None,
             row_scale: Optional[torch.Tensor] = None, mask: Optional[RowMask] = None
             ) -> Tuple[torch.Tensor, torch.Tensor]:
    """(scores ``[nq, kk]`` fp32, ids ``[nq, kk]`` int64), ``kk = min(k, N)``, of the contiguous fp32
    ``q [nq, D]`` against the contiguous fp32 or fp16 ``c [N, D]``; ``row_scale`` (fp32 ``[N]``,
    contiguous) goes with an fp16 ``c`` only. With a ``mask`` (on ``c``'s device) only its rows are
    searched and ``kk = min(k, mask.count)``; a mask that allows nothing gives ``[nq, 0]`` without a launch."""
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
    if mask is not None:
        _check_mask(mask, c)
        kk = min(k, mask.count)
    if nq == 0 or kk == 0:
        return (torch.empty((nq, kk), dtype=torch.float32, device=q.device),
                torch.empty((nq, kk), dtype=torch.int64, device=q.device))
    if not q.is_cuda:
        return sim_topk_ref(q, c, k, id_base, row_scale=row_scale, mask=mask)
    nat = native()
    if mask is not None:
        n_live = mask.live.numel()
        P = nat.sim_topk_splits_live(n_live, splits if splits is not None else auto_splits(N, nq, q.device))
        ws = torch.empty((nq, P, k, 2), dtype=torch.float32, device=q.device)
        scores = torch.empty((nq, kk), dtype=torch.float32, device=q.device)
        ids = torch.empty((nq, kk), dtype=torch.int64, device=q.device)
        stream = launch_stream(q)
        if half:
            nat.sim_topk_partial_masked_f16(ptr(q), ptr(c), ptr(row_scale) if row_scale is not None else 0,
                                            ptr(mask.words), ptr(mask.live), ptr(ws), nq, N, D, k, P, n_live, stream)
        else:
            nat.sim_topk_partial_masked(ptr(q), ptr(c), ptr(mask.words), ptr(mask.live), ptr(ws), nq, N, D, k, P,
                                        n_live, stream)
        nat.sim_topk_merge(ptr(ws), ptr(scores), ptr(ids), nq, P, k, kk, int(id_base), stream)
        return scores, ids
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


# ------------------------------------------------------------------------------------------------ IVF
PAD_ID = 2 ** 62  # id of the (-inf) padding past a query's count
IVF_QT = 16  # kIvfItemQueries: queries of one cluster per work item
IVF_MAX_CLUSTERS = 4096  # kKmeansMaxK
_NO_ROW = 0x7fffffff  # kNoRow: the id of an empty list entry


def _check_ivf(q, vectors, row_ids, offsets, centroids, k, nprobe, id_base, splits):
    check(q.dim() == 2 and vectors.dim() == 2 and centroids.dim() == 2 and q.shape[1] == vectors.shape[1]
          and q.shape[1] == centroids.shape[1], "sim_topk_ivf: q [nq, D], vectors [n, D] and centroids [K, D]")
    check(q.dtype == torch.float32 and vectors.dtype == torch.float32 and centroids.dtype == torch.float32,
          "sim_topk_ivf: q, vectors and centroids must be fp32")
    n, K = vectors.shape[0], centroids.shape[0]
    check(0 <= n <= MAX_ROWS, "sim_topk_ivf: n must be in [0, 2^31 - 256]")
    check(isinstance(k, int) and not isinstance(k, bool) and sim_topk_ok(q.shape[1], k),
          f"sim_topk_ivf: unsupported shape D={q.shape[1]} k={k}")
    check(1 <= K <= IVF_MAX_CLUSTERS, "sim_topk_ivf: K must be in [1, 4096]")
    check(isinstance(nprobe, int) and not isinstance(nprobe, bool) and 1 <= nprobe <= min(MAX_K, K),
          "sim_topk_ivf: nprobe must be in [1, min(32, K)]")
    check(row_ids.dtype == torch.int32 and row_ids.shape == (n,) and offsets.dtype == torch.int32
          and offsets.shape == (K + 1,), "sim_topk_ivf: row_ids must be int32 [n] and offsets int32 [K + 1]")
    check(all(t.is_contiguous() for t in (q, vectors, row_ids, offsets, centroids)), "sim_topk_ivf: contiguous tensors")
    check(isinstance(id_base, int) and 0 <= id_base < 2 ** 61, "sim_topk_ivf: id_base must be in [0, 2^61)")
    check(splits is None or (isinstance(splits, int) and 1 <= splits * nprobe <= MAX_SPLITS),
          f"sim_topk_ivf: nprobe * splits must be in [1, {MAX_SPLITS}]")
    same_device(q, vectors, row_ids, offsets, centroids)


def _ivf_pad(scores: torch.Tensor, ids: torch.Tensor, empty: torch.Tensor):
    """(scores, ids, counts) with ``(-inf, PAD_ID)`` in the ``empty`` columns (they sort last: a suffix)."""
    scores = torch.where(empty, torch.full_like(scores, float("-inf")), scores)
    ids = torch.where(empty, torch.full_like(ids, PAD_ID), ids)
    return scores, ids, (~empty).sum(1)


def ivf_labels(row_ids: torch.Tensor, offsets: torch.Tensor) -> torch.Tensor:
    """int64 ``[n]``: the cluster of every ORIGINAL row of an index (the inverse of the sort)."""
    n, K = row_ids.numel(), offsets.numel() - 1
    sizes = (offsets[1:] - offsets[:-1]).to(torch.int64)
    by_pos = torch.repeat_interleave(torch.arange(K, device=offsets.device), sizes, output_size=n)
    labels = torch.empty((n,), dtype=torch.int64, device=row_ids.device)
    labels[row_ids.to(torch.int64)] = by_pos
    return labels


def sim_topk_ivf_ref(q: torch.Tensor, vectors: torch.Tensor, row_ids: torch.Tensor, offsets: torch.Tensor,
                     centroids: torch.Tensor, k: int, nprobe: int, id_base: int = 0
                     ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """PyTorch twin of :func:`sim_topk_ivf` and the CPU path: per query, ``sim_topk_ref`` with the mask
    "the row's cluster is in the query's probe list" over the rows put back in their original order."""
    _check_ivf(q, vectors, row_ids, offsets, centroids, k, nprobe, id_base, None)
    nq, n = q.shape[0], vectors.shape[0]
    if nq == 0 or n == 0:
        return (torch.full((nq, k), float("-inf"), dtype=torch.float32, device=q.device),
                torch.full((nq, k), PAD_ID, dtype=torch.int64, device=q.device),
                torch.zeros((nq,), dtype=torch.int64, device=q.device))
    probes = sim_topk_ref(q, centroids, nprobe)[1]  # [nq, nprobe]
    x = torch.empty_like(vectors)
    x[row_ids.to(torch.int64)] = vectors
    labels = ivf_labels(row_ids, offsets)
    allowed = torch.zeros((nq, n), dtype=torch.bool, device=q.device)
    for j in range(nprobe):
        allowed |= labels[None, :] == probes[:, j:j + 1]
    s = (q @ x.T).masked_fill(~allowed, float("-inf"))  # by select: a NaN outside the probed clusters cannot leak
    order = torch.sort(s + 0.0, dim=1, descending=True, stable=True).indices[:, :k]
    scores, ids = torch.gather(s, 1, order), order.to(torch.int64) + int(id_base)
    empty = ~torch.gather(allowed, 1, order)
    if scores.shape[1] < k:  # fewer rows than k
        pad = k - scores.shape[1]
        scores = torch.cat([scores, scores.new_full((nq, pad), float("-inf"))], 1)
        ids = torch.cat([ids, ids.new_full((nq, pad), PAD_ID)], 1)
        empty = torch.cat([empty, empty.new_ones((nq, pad))], 1)
    return _ivf_pad(scores, ids, empty)


def ivf_plan(probes: torch.Tensor, K: int, items: int) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """The work items of a probe table ``[nq, nprobe]`` (cluster ids), built on its device with no copy back:
    (item_cluster ``[items]``, item_query ``[items, 16]``, item_slot ``[items, 16]``), all int32. The
    ``nq * nprobe`` (query, slot) pairs are sorted by cluster (stable: ascending query inside one) and cut into
    items of at most 16 queries of one cluster; every pair lands in exactly one item. ``items`` is the launch
    bound ``min(nq * nprobe, K) + nq * nprobe // 16``: a cluster with ``m`` pairs takes ``ceil(m / 16)``, at
    most one more than ``m // 16``. Surplus items keep cluster ``-1``, padding slots ``-1`` and a valid query.
    On the GPU one small kernel does it in one launch (``sim_topk_ivf_plan``; a pair's slot inside its cluster is
    then whatever the atomics gave, which the search does not depend on); this function's own PyTorch calls are
    its twin and the CPU path."""
    nq, nprobe = probes.shape
    dev = probes.device
    check(probes.dim() == 2 and probes.dtype == torch.int64 and probes.is_contiguous() and nq >= 1 and nprobe >= 1,
          "ivf_plan: probes must be a contiguous int64 [nq, nprobe]")
    if probes.is_cuda:
        item_cluster = torch.empty((items,), dtype=torch.int32, device=dev)
        item_query = torch.empty((items, IVF_QT), dtype=torch.int32, device=dev)
        item_slot = torch.empty((items, IVF_QT), dtype=torch.int32, device=dev)
        native().sim_topk_ivf_plan(ptr(probes), nq, nprobe, K, items, ptr(item_cluster), ptr(item_query), ptr(item_slot),
                                   launch_stream(probes))
        return item_cluster, item_query, item_slot
    cl, pair = torch.sort(probes.reshape(-1), stable=True)
    per = torch.zeros((K,), dtype=torch.int64, device=dev).scatter_add_(0, cl, torch.ones_like(cl))
    first = torch.cumsum(per, 0) - per  # the sorted position of a cluster's first pair
    n_items = (per + (IVF_QT - 1)) // IVF_QT
    item0 = torch.cumsum(n_items, 0) - n_items  # a cluster's first item
    rank = torch.arange(cl.numel(), device=dev) - first[cl]
    item, lane = item0[cl] + rank // IVF_QT, rank % IVF_QT
    item_cluster = torch.full((items,), -1, dtype=torch.int32, device=dev)
    item_query = torch.zeros((items, IVF_QT), dtype=torch.int32, device=dev)
    item_slot = torch.full((items, IVF_QT), -1, dtype=torch.int32, device=dev)
    item_cluster[item] = cl.to(torch.int32)
    item_query[item, lane] = (pair // nprobe).to(torch.int32)
    item_slot[item, lane] = (pair % nprobe).to(torch.int32)
    item_query = torch.where(item_slot >= 0, item_query, item_query[:, :1])  # padding repeats the item's first query
    return item_cluster, item_query.contiguous(), item_slot


def ivf_splits(nq: int, nprobe: int, K: int, n: int, device: torch.device) -> int:
    """Splits per work item: enough workgroups (three of the 16-query form fit a CU) for the item bound, no more
    than a cluster of average size has 32-row steps, and ``nprobe * S <= 256`` lists per query for the merge."""
    cus = torch.cuda.get_device_properties(device).multi_processor_count
    bound = min(nq * nprobe, K) + nq * nprobe // IVF_QT
    steps = max(1, -(-n // (32 * K)))
    return max(1, min(MAX_SPLITS // nprobe, -(-3 * cus // bound), steps))


def sim_topk_ivf(q: torch.Tensor, vectors: torch.Tensor, row_ids: torch.Tensor, offsets: torch.Tensor,
                 centroids: torch.Tensor, k: int, nprobe: int, id_base: int = 0, splits: Optional[int] = None
                 ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """(scores ``[nq, k]`` fp32, ids ``[nq, k]`` int64, counts ``[nq]`` int64) of the fp32 ``q [nq, D]`` against
    an IVF index (``csrc/kernels/sim_topk_ivf.hip``): ``vectors [n, D]`` fp32 sorted by cluster, ``row_ids [n]``
    int32 (the original row of a sorted row, ascending inside a cluster), ``offsets [K + 1]`` int32 and the
    ``centroids [K, D]``. Query ``i`` searches the ``nprobe`` clusters whose centroids score best against it
    (``sim_topk(q, centroids, nprobe)``: fixed bits whatever the batch); ``ids = id_base + original row``, in the
    (score desc, id asc) order of the exact search, and a score has ``sim_topk``'s bits. The columns past
    ``counts[i]`` (fewer than ``k`` rows in the probed clusters) hold ``(-inf, PAD_ID)``. The result does not
    depend on ``splits`` (tests and benches) or on the batch; with ``nprobe == K`` it is ``sim_topk``'s."""
    _check_ivf(q, vectors, row_ids, offsets, centroids, k, nprobe, id_base, splits)
    nq, D = q.shape
    n, K = vectors.shape[0], centroids.shape[0]
    if not q.is_cuda or nq == 0 or n == 0:
        return sim_topk_ivf_ref(q, vectors, row_ids, offsets, centroids, k, nprobe, id_base)
    nat = native()
    probes = sim_topk(q, centroids, nprobe)[1]
    items = int(nat.sim_topk_ivf_items(nq, nprobe, K))
    item_cluster, item_query, item_slot = ivf_plan(probes, K, items)
    S = splits if splits is not None else ivf_splits(nq, nprobe, K, n, q.device)
    P = nprobe * S
    ws = torch.empty((nq, P, k, 2), dtype=torch.float32, device=q.device)
    scores = torch.empty((nq, k), dtype=torch.float32, device=q.device)
    ids = torch.empty((nq, k), dtype=torch.int64, device=q.device)
    stream = launch_stream(q)
    nat.sim_topk_ivf_partial(ptr(q), ptr(vectors), ptr(row_ids), ptr(offsets), ptr(item_cluster), ptr(item_query),
                             ptr(item_slot), ptr(ws), nq, n, D, k, K, nprobe, S, items, stream)
    nat.sim_topk_merge(ptr(ws), ptr(scores), ptr(ids), nq, P, k, k, int(id_base), stream)
    return _ivf_pad(scores, ids, ids == int(id_base) + _NO_ROW)  # the merge's empty entries: (-inf, id_base + kNoRow)
