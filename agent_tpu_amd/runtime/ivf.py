"""Inverted-file (IVF) indexes over the resident corpora of ``map_search``.

An index is the normalised fp32 slice that :func:`runtime.search.load_corpus` gives, sorted by k-means cluster:
``runtime.cluster.kmeans`` (cosine, seed 0, at most ``train_iterations`` iterations; a collective under DP, so
the centroids are global and equal on every rank), then one more ``ops.kmeans_assign`` against the final
centroids, so that a row's list is the arg-max over the centroids the queries are probed with even when k-means
stopped at its iteration limit (without a bias that is ``sim_topk(x, centroids, 1)`` bit for bit). The rows are
then gathered in the stable order of their labels: ascending original row inside a cluster.

The entry lives in ``runtime.search``'s LRU under the corpus key extended by ``("ivf", clusters,
train_iterations)``: it counts towards ``SEARCH_INDEX_LRU_SIZE`` and ``cache_info()`` reports its bytes. It does
not hold the original-order copy. Building is one-time plumbing in PyTorch around the k-means kernels; the
search is ``ops.sim_topk_ivf``.
"""
from __future__ import annotations

import math
from typing import Any, Dict, NamedTuple, Optional, Tuple

import torch

from . import search as rs

MAX_CLUSTERS = 4096  # ops.cluster.MAX_K
SEED = 0

#: the builder's input error (``ops/map_search.py`` lists it in ``IVF_ERRORS``)
ERRORS: Dict[str, str] = {
    "index_too_large": "index build exceeds SEARCH_INDEX_MAX_GB (two float32 copies of the corpus slice)",
}


class IvfIndex(NamedTuple):
    vectors: torch.Tensor  # [count, dim] fp32: the slice's normalised rows sorted by cluster
    row_ids: torch.Tensor  # [count] int32: the row of the slice that a sorted row is (ascending inside a cluster)
    offsets: torch.Tensor  # [K + 1] int32: cluster c is vectors[offsets[c]:offsets[c + 1]]
    centroids: torch.Tensor  # [K, dim] fp32, normalised; equal on every rank
    start: int  # row of the file that slice row 0 is
    total: int  # rows of the whole file
    iterations: int  # k-means iterations run
    converged: bool
    cached: bool = False  # served from the LRU


def default_clusters(total: int) -> int:
    return max(1, min(MAX_CLUSTERS, total, math.isqrt(max(total - 1, 0)) + 1))  # ceil(sqrt(total)), clamped


def _key(uri: Any, start: int, count: int, device: torch.device, K: int, t: int) -> Tuple[Tuple, int, int, int, int]:
    arr, path, st = rs.open_corpus(uri)
    total, dim = int(arr.shape[0]), int(arr.shape[1])
    start = max(0, min(int(start), total))
    count = total - start if count < 0 else max(0, min(int(count), total - start))
    return ((path, st.st_mtime_ns, st.st_size, start, count, str(device), "ivf", int(K), int(t)), start, count, total,
            dim)


def open_index(uri: Any, start: int, count: int, device: torch.device, K: int, t: int):
    """The part of a lookup without collectives -> (key, the cached :class:`IvfIndex` or None, the loaded
    ``Corpus`` of a miss or None). A miss checks the build's peak, two fp32 copies of the slice, against
    ``SEARCH_INDEX_MAX_GB`` before any allocation."""
    key, start, count, total, dim = _key(uri, start, count, device, K, t)
    with rs._lock:
        hit = rs._cache.get(key)
        if hit is not None:
            rs._cache.move_to_end(key)
            return key, IvfIndex(hit[0], hit[1], hit[2], hit[3], start, total, hit[4], hit[5], True), None
    if 2 * count * dim * 4 > rs.max_bytes():
        raise ValueError(ERRORS["index_too_large"])
    return key, None, rs.load_corpus(uri, start, count, True, device, "float32")


def original_rows(index: IvfIndex) -> torch.Tensor:
    """The slice in its original row order (a copy)."""
    x = torch.empty_like(index.vectors)
    x[index.row_ids.to(torch.int64)] = index.vectors
    return x


def build(x: torch.Tensor, K: int, t: int, rank: int = 0, ws: int = 1, start: int = 0, total: Optional[int] = None):
    """-> (vectors, row_ids, offsets, centroids, iterations, converged) of the normalised fp32 rows ``x [n, D]``
    that this rank holds (``n`` may be 0). Every rank of the group calls it: k-means is a collective."""
    from .. import ops
    from .cluster import kmeans

    n = int(x.shape[0])
    km = kmeans(x, K, "cosine", seed=SEED, max_iter=t, rank=rank, ws=ws, start=start, total=total)
    centroids = km.centroids.contiguous()
    if n:
        labels = ops.kmeans_assign(x, centroids)[0].to(torch.int64)
    else:
        labels = torch.zeros((0,), dtype=torch.int64, device=x.device)
    order = torch.sort(labels, stable=True).indices
    sizes = torch.zeros((K,), dtype=torch.int64, device=x.device).scatter_add_(0, labels, torch.ones_like(labels))
    offsets = torch.zeros((K + 1,), dtype=torch.int32, device=x.device)
    offsets[1:] = torch.cumsum(sizes, 0).to(torch.int32)
    vectors = torch.empty_like(x)
    rows = max(1, rs.CHUNK_BYTES // (max(1, x.shape[1]) * 4))
    for lo in range(0, n, rows):  # gathered in row chunks: no third copy of the slice
        vectors[lo:lo + rows] = x[order[lo:lo + rows]]
    return vectors, order.to(torch.int32).contiguous(), offsets, centroids, int(km.iterations), bool(km.converged)


def build_index(key: Tuple, x: torch.Tensor, K: int, t: int, rank: int, ws: int, start: int, total: int) -> IvfIndex:
    """Build (a collective under DP) and put the entry into the LRU."""
    entry = build(x, K, t, rank, ws, start, total)
    with rs._lock:
        rs._cache[key] = entry
        rs._cache.move_to_end(key)
        while len(rs._cache) > rs.lru_capacity():
            rs._cache.popitem(last=False)
    return IvfIndex(entry[0], entry[1], entry[2], entry[3], start, total, entry[4], entry[5], False)


def load_index(uri: Any, start: int = 0, count: int = -1, device: torch.device = torch.device("cpu"),
               clusters: Optional[int] = None, train_iterations: int = 10) -> IvfIndex:
    """Single-process form: the cached index of the slice, or a fresh build."""
    total = rs.corpus_shape(uri)[0]
    K = default_clusters(total) if clusters is None else int(clusters)
    key, hit, corpus = open_index(uri, start, count, device, K, train_iterations)
    if hit is not None:
        return hit
    return build_index(key, corpus.vectors, K, train_iterations, 0, 1, corpus.start, corpus.total)


def search(qvecs: torch.Tensor, index: IvfIndex, k: int, nprobe: int, id_base: int = 0):
    """(scores ``[nq, k]``, ids ``[nq, k]``, counts ``[nq]``) of ``ops.sim_topk_ivf`` on the index's device (its
    PyTorch twin on a CPU engine): every list padded to ``k`` with ``(-inf, 2^62)``. An empty slice (a DP rank
    beyond the corpus) gives all padding."""
    from .. import ops

    q = qvecs.to(device=index.vectors.device, dtype=torch.float32).contiguous()
    return ops.sim_topk_ivf(q, index.vectors, index.row_ids, index.offsets, index.centroids, k, nprobe, id_base)
