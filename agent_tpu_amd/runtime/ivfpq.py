"""IVF-PQ (IVFADC) indexes for ``map_search``: coarse clusters with product-quantization codes of the residuals.

The builder keeps ``runtime/pq.py``'s discipline: no collective, and the fp32 slice is never resident.

**Training.** Every rank reads the same sample of the memory-mapped file (``pq.sample_rows(total, T)``, normalised).
The centroids are ``runtime.cluster.kmeans`` of the sample alone (cosine, seed 0, at most ``t`` iterations, ``rank 0``
of ``ws 1``), so they are equal on every rank and every world size. The codebooks are ``pq.train`` (``t`` iterations)
over the sample's residuals ``x - centroids[label]``, an fp32 subtract with one rounding; ``label`` is
``ops.kmeans_assign`` against the final centroids.

**Encoding.** The rank's slice is streamed in chunks of at most ``CHUNK_BYTES`` of fp32: load, check, normalise,
``ops.kmeans_assign``, ``ops.pq_encode_residual`` (the residual exists in registers only). After the last chunk the
``[count, M]`` codes and the int32 labels are sorted stably by label: ``row_ids`` int32 (the slice row of a sorted row,
ascending inside a cluster), ``offsets`` int32 ``[K + 1]`` and the sorted codes, on the GPU as ONE interleaved
``ops.PqCodes`` image over the sorted rows (clusters are not padded to 64 rows), on a CPU engine row-major.

**Cache.** An entry of ``runtime.search``'s LRU under the corpus key extended by ``("ivfpq", K, M, T, t)``;
``cache_info()`` reports its bytes: codes, ids, offsets, centroids and codebooks.

**Search.** ``ops.sim_topk_ivfpq``: the probe, the coarse term, the table, the scan of the probed clusters, the merge.
"""
from __future__ import annotations

from typing import Any, Dict, NamedTuple, Optional, Tuple

import torch

from . import pq
from .ivf import MAX_CLUSTERS
from . import search as rs

SEED = 0

#: the builder's input error (``ops/map_search.py`` lists it in ``IVFPQ_ERRORS``)
ERRORS: Dict[str, str] = {
    "ivfpq_too_large": "ivfpq index slice exceeds SEARCH_INDEX_MAX_GB of codes and row ids",
}


class IvfPqIndex(NamedTuple):
    codes: torch.Tensor  # uint8, rows sorted by cluster: [count, M] (CPU) or [ceil(count / 64), M / 4, 64, 4] (GPU)
    row_ids: torch.Tensor  # [count] int32: the row of the slice that a sorted row is (ascending inside a cluster)
    offsets: torch.Tensor  # [K + 1] int32: cluster c is the sorted rows offsets[c]:offsets[c + 1]
    centroids: torch.Tensor  # [K, dim] fp32, normalised; equal on every rank
    codebooks: torch.Tensor  # [M, 256, dsub] fp32 of the residuals; equal on every rank
    rows: int  # count: rows of the slice
    start: int  # row of the file that slice row 0 is
    total: int  # rows of the whole file
    iterations: int  # k-means iterations run
    converged: bool
    cached: bool = False  # served from the LRU

    @property
    def subvectors(self) -> int:
        return int(self.codebooks.shape[0])


def train(sample: torch.Tensor, K: int, M: int, t: int) -> Tuple[torch.Tensor, torch.Tensor, int, bool]:
    """(centroids ``[K, D]``, residual codebooks ``[M, 256, dsub]``, k-means iterations, converged) of the normalised
    sample ``[T, D]`` (``T >= max(256, K)``)."""
    from .. import ops
    from .cluster import kmeans

    km = kmeans(sample, K, "cosine", seed=SEED, max_iter=t, rank=0, ws=1)
    centroids = km.centroids.contiguous()
    labels = ops.kmeans_assign(sample, centroids)[0].to(torch.int64)
    books = pq.train((sample - centroids[labels]).contiguous(), M, t)
    return centroids, books, int(km.iterations), bool(km.converged)


def encode_slice(arr, start: int, count: int, centroids: torch.Tensor, books: torch.Tensor, device: torch.device):
    """(codes in the device's resident layout, row_ids, offsets) of rows ``[start, start + count)``, chunk by chunk."""
    from .. import ops

    M, dim, K = int(books.shape[0]), int(arr.shape[1]), int(centroids.shape[0])
    codes = torch.empty((count, M), dtype=torch.uint8, device=device)
    labels = torch.empty((count,), dtype=torch.int32, device=device)
    bias = ops.pq_bias(books)
    rows = max(1, rs.CHUNK_BYTES // (dim * 4))
    for lo in range(0, count, rows):
        hi = min(lo + rows, count)
        x = pq._rows_to_device(arr, start + lo, start + hi, True, device)
        labels[lo:hi] = ops.kmeans_assign(x, centroids)[0]
        codes[lo:hi] = ops.pq_encode_residual(x, labels[lo:hi].contiguous(), centroids, books, bias)
    lab = labels.to(torch.int64)
    order = torch.sort(lab, stable=True).indices
    sizes = torch.zeros((K,), dtype=torch.int64, device=device).scatter_add_(0, lab, torch.ones_like(lab))
    offsets = torch.zeros((K + 1,), dtype=torch.int32, device=device)
    offsets[1:] = torch.cumsum(sizes, 0).to(torch.int32)
    codes = codes[order].contiguous()
    if torch.device(device).type == "cuda":
        codes = ops.pq_interleave(codes).data
    return codes, order.to(torch.int32).contiguous(), offsets


def load_index(uri: Any, start: int = 0, count: int = -1, device: torch.device = torch.device("cpu"),
               clusters: int = 16, subvectors: int = 8, train_rows: Optional[int] = None,
               train_iterations: int = 10) -> IvfPqIndex:
    """The cached index of rows ``[start, start + count)`` (``count < 0``: to the end) of the file, or a fresh
    build. No collective: under DP every rank trains the same centroids and codebooks from the same sample."""
    from .. import ops

    K, M, t = int(clusters), int(subvectors), int(train_iterations)
    arr, path, st = rs.open_corpus(uri)
    total, dim = int(arr.shape[0]), int(arr.shape[1])
    T = pq.default_train_rows(total) if train_rows is None else int(train_rows)
    start = max(0, min(int(start), total))
    count = total - start if count < 0 else max(0, min(int(count), total - start))
    key = (path, st.st_mtime_ns, st.st_size, start, count, str(device), "ivfpq", K, M, T, t)
    with rs._lock:
        hit = rs._cache.get(key)
        if hit is not None:
            rs._cache.move_to_end(key)
            return IvfPqIndex(hit[0], hit[1], hit[2], hit[3], hit[4], count, start, total, hit[5], hit[6], True)
    if (not ops.pq_ok(dim, M) or not ops.sim_topk_ok(dim, 1) or not pq.MIN_ROWS <= T <= min(total, pq.MAX_TRAIN_ROWS)
            or not 1 <= K <= min(T, MAX_CLUSTERS) or t < 1):
        raise ValueError("load_index: unsupported (dim, clusters, subvectors, train_rows, train_iterations)")
    if pq.codes_bytes(count, M, device) + 4 * count > rs.max_bytes():  # before any allocation
        raise ValueError(ERRORS["ivfpq_too_large"])
    sample = pq._rows_to_device(arr, 0, 0, True, device, index=pq.sample_rows(total, T).numpy())
    centroids, books, iterations, converged = train(sample, K, M, t)
    del sample
    codes, row_ids, offsets = encode_slice(arr, start, count, centroids, books, device)
    with rs._lock:
        rs._cache[key] = (codes, row_ids, offsets, centroids, books, iterations, converged)
        rs._cache.move_to_end(key)
        while len(rs._cache) > rs.lru_capacity():
            rs._cache.popitem(last=False)
    return IvfPqIndex(codes, row_ids, offsets, centroids, books, count, start, total, iterations, converged, False)


def row_major_codes(index: IvfPqIndex) -> torch.Tensor:
    """uint8 ``[rows, M]`` of the sorted rows of an index on either device (a copy on the GPU)."""
    from .. import ops

    if index.codes.dim() == 2:
        return index.codes
    return ops.pq_deinterleave(ops.PqCodes(index.codes, index.rows, index.subvectors))


def search(qvecs: torch.Tensor, index: IvfPqIndex, k: int, nprobe: int, id_base: int = 0):
    """(scores ``[nq, k]``, ids ``[nq, k]``, counts ``[nq]``) of ``ops.sim_topk_ivfpq`` on the index's device (its
    PyTorch twin on a CPU engine): every list padded to ``k`` with ``(-inf, 2^62)``. An empty slice (a DP rank
    beyond the corpus) gives all padding."""
    from .. import ops

    q = qvecs.to(device=index.codebooks.device, dtype=torch.float32).contiguous()
    codes = index.codes if index.codes.dim() == 2 else ops.PqCodes(index.codes, index.rows, index.subvectors)
    return ops.sim_topk_ivfpq(q, index.codebooks, codes, index.row_ids, index.offsets, index.centroids, k, nprobe,
                              id_base)
