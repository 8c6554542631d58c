"""Binary (sign-bit) resident corpora for ``map_search``: ``D / 8`` bytes per row instead of ``4 D`` or ``2 D``.

**Threshold.** Bit ``d`` of a row is ``x_d > t_d``. ``"zero"``: ``t = 0``. ``"mean"``: the per-column mean of the
sample ``runtime.pq.sample_rows(total, min(total, 65536))`` of the file (normalised for the cosine metric, as the
rows are), summed in fp64 and rounded once. Every rank reads the same sample, so the threshold is equal on every
rank and every world size and no collective is needed. There is nothing else to train.

**Encoding.** The rank's slice is streamed from the file in chunks, as ``runtime/pq.py`` does: load, check,
normalise, ``ops.binary_pack``. The fp32 slice is never resident: the peak is one chunk plus the codes. An optional
``runtime.refine.Store`` (the originals, for exact re-scoring) is filled from the same chunks.

**Cache.** The entry lives in ``runtime.search``'s LRU under the corpus key extended by ``("binary", threshold,
normalised?)`` (plus ``("refine", vectors, store)``). On the GPU the codes are kept in the scan kernel's layout
(``ops.BinaryCodes``: the last 64-row block padded), on a CPU engine row-major.

**Search.** ``ops.binary_pack`` of the queries -> the Hamming scan -> ``sim_topk_merge`` (``ops.sim_topk_binary``);
with a store: ``ops.hamming_scan_segments`` (the shortlist) -> ``ops.refine_topk``.
"""
from __future__ import annotations

from typing import Any, Dict, NamedTuple, Optional, Tuple

import torch

from . import pq
from . import search as rs

THRESHOLDS = ("zero", "mean")
MEAN_ROWS = 65536

#: the builder's input error (``ops/map_search.py`` lists it in ``BINARY_ERRORS``)
ERRORS: Dict[str, str] = {
    "binary_too_large": "binary corpus slice exceeds SEARCH_INDEX_MAX_GB of codes",
}


class BinaryIndex(NamedTuple):
    codes: torch.Tensor  # int32: [count, D / 32] row-major (CPU) or [ceil(count / 64), D / 32, 64] (GPU)
    thr: torch.Tensor  # [D] fp32; equal on every rank
    rows: int  # count: rows of the slice
    start: int  # row of the file that slice row 0 is
    total: int  # rows of the whole file
    cached: bool = False  # served from the LRU
    store: Optional[Any] = None  # runtime.refine.Store: the rows' originals for exact re-scoring (``refine``)

    @property
    def dim(self) -> int:
        return int(self.thr.shape[0])


def codes_bytes(count: int, dim: int, device: torch.device) -> int:
    """Resident bytes of the codes of ``count`` rows on ``device`` (the GPU layout pads the last 64-row block)."""
    return pq.codes_bytes(count, dim // 8, device)


def threshold(arr, total: int, kind: str, normalize: bool, device: torch.device) -> torch.Tensor:
    """fp32 ``[dim]`` on ``device``: zeros, or the column means of the sample rows (fp64 sums, rounded once)."""
    dim = int(arr.shape[1])
    if kind == "zero":
        return torch.zeros((dim,), dtype=torch.float32, device=device)
    acc, n = torch.zeros((dim,), dtype=torch.float64, device=device), min(total, MEAN_ROWS)
    idx = pq.sample_rows(total, n).numpy()
    rows = max(1, rs.CHUNK_BYTES // (dim * 4))
    for lo in range(0, n, rows):  # in chunks: the sample is never resident at once
        acc += pq._rows_to_device(arr, 0, 0, normalize, device, index=idx[lo:lo + rows]).double().sum(dim=0)
    return (acc / n).to(torch.float32).contiguous()


def encode_slice(arr, start: int, count: int, thr: torch.Tensor, normalize: bool, device: torch.device,
                 store=None) -> torch.Tensor:
    """The codes of rows ``[start, start + count)`` in the device's resident layout, chunk by chunk. ``store`` (a
    ``runtime.refine.Store``) is filled from the same chunks: the file is read once."""
    from .. import ops
    from ..ops.pq import BLOCK_ROWS

    dim = int(arr.shape[1])
    W, cuda = dim // 32, torch.device(device).type == "cuda"
    shape = (-(-count // BLOCK_ROWS), W, BLOCK_ROWS) if cuda else (count, W)
    out = torch.empty(shape, dtype=torch.int32, device=device)
    rows = max(BLOCK_ROWS, rs.CHUNK_BYTES // (dim * 4) // BLOCK_ROWS * BLOCK_ROWS)  # whole blocks per chunk
    for lo in range(0, count, rows):
        hi = min(lo + rows, count)
        raw = pq._raw_rows(arr, start + lo, start + hi, device)
        x = (rs.normalize_rows(raw) if normalize else raw).contiguous()
        if store is not None:
            store.fill(lo, hi, raw, x)
        if cuda:  # a chunk's blocks, the padding rows of the slice's last block zero
            part = ops.binary_pack(x, thr, interleave=True).data
            out[lo // BLOCK_ROWS:lo // BLOCK_ROWS + part.shape[0]] = part
        else:
            out[lo:hi] = ops.binary_pack(x, thr)
    return out


def load_index(uri: Any, start: int = 0, count: int = -1, device: torch.device = torch.device("cpu"),
               kind: str = "zero", normalize: bool = True, refine: Optional[Tuple[str, str]] = None) -> BinaryIndex:
    """The cached index of rows ``[start, start + count)`` (``count < 0``: to the end) of the file, or a fresh
    build. No collective. ``refine`` (``(vectors, store)``: ``runtime/refine.py``) adds the refine store of the slice
    to the entry, under a key of its own: it is built, evicted and rebuilt with the codes."""
    from .. import ops
    from . import refine as rf

    arr, path, st = rs.open_corpus(uri)
    total, dim = int(arr.shape[0]), int(arr.shape[1])
    start = max(0, min(int(start), total))
    count = total - start if count < 0 else max(0, min(int(count), total - start))
    key = (path, st.st_mtime_ns, st.st_size, start, count, str(device), "binary", str(kind), bool(normalize))
    if refine is not None:
        key = key + ("refine",) + tuple(refine)
    with rs._lock:
        hit = rs._cache.get(key)
        if hit is not None:
            rs._cache.move_to_end(key)
            store = rf.Store(hit[2], hit[3]) if refine is not None else None
            return BinaryIndex(hit[0], hit[1], count, start, total, True, store)
    if not ops.binary_ok(dim) or kind not in THRESHOLDS:
        raise ValueError("load_index: unsupported (dim, threshold)")
    nbytes = codes_bytes(count, dim, device)
    if nbytes > rs.max_bytes():  # before any allocation
        raise ValueError(ERRORS["binary_too_large"])
    store = None
    if refine is not None:  # sized before any allocation, as the codes
        rf.check_size(count, dim, refine[0], refine[1], normalize, device, nbytes)
        store = rf.allocate(count, dim, refine[0], refine[1], normalize, device)
    thr = threshold(arr, total, kind, normalize, device)
    codes = encode_slice(arr, start, count, thr, normalize, device, store)
    with rs._lock:
        rs._cache[key] = (codes, thr) if store is None else (codes, thr, store.vectors, store.scale)
        rs._cache.move_to_end(key)
        while len(rs._cache) > rs.lru_capacity():
            rs._cache.popitem(last=False)
    return BinaryIndex(codes, thr, count, start, total, False, store)


def _codes(index: BinaryIndex):
    from .. import ops

    return index.codes if index.codes.dim() == 2 else ops.BinaryCodes(index.codes, index.rows, index.dim)


def search(qvecs: torch.Tensor, index: BinaryIndex, k: int, id_base: int = 0) -> Tuple[torch.Tensor, torch.Tensor]:
    """(scores ``[nq, kk]`` fp32, ids ``[nq, kk]`` int64), ``kk = min(k, rows)``, of ``ops.sim_topk_binary`` on the
    index's device (its PyTorch twin on a CPU engine): the integer +-1 dot products, ordered by (score desc, id asc).
    An empty slice (a DP rank beyond the corpus) gives ``kk = 0``."""
    from .. import ops

    dev = index.thr.device
    q = qvecs.to(device=dev, dtype=torch.float32).contiguous()
    if index.rows == 0 or q.shape[0] == 0:
        kk = min(k, index.rows)
        return (torch.empty((q.shape[0], kk), dtype=torch.float32, device=dev),
                torch.empty((q.shape[0], kk), dtype=torch.int64, device=dev))
    return ops.sim_topk_binary(q, index.thr, _codes(index), k, id_base)


def search_refined(qvecs: torch.Tensor, index: BinaryIndex, k: int, candidates: int, id_base: int = 0
                   ) -> Tuple[torch.Tensor, torch.Tensor, int]:
    """(scores ``[nq, k]`` fp32, ids ``[nq, k]`` int64, rows re-scored per query) of an index with a store: the exact
    scores of the slice's Hamming shortlist of ``candidates`` rows, in the (score desc, id asc) order, padded with
    ``(-inf, 2^62)`` past the shortlist's live rows. An empty slice gives padding only."""
    from .. import ops

    dev = index.thr.device
    q = qvecs.to(device=dev, dtype=torch.float32).contiguous()
    if index.rows == 0 or q.shape[0] == 0:
        return (torch.full((q.shape[0], k), float("-inf"), dtype=torch.float32, device=dev),
                torch.full((q.shape[0], k), ops.search.PAD_ID, dtype=torch.int64, device=dev), 0)
    G = candidates // ops.refine.SEGMENT_LIST
    cand = ops.hamming_scan_segments(ops.binary_pack(q, index.thr), _codes(index), index.dim, G)
    s, i = ops.refine_topk(q, index.store.vectors, cand, k, id_base, row_scale=index.store.scale)
    return s, i, ops.shortlist_rows(index.rows, G)
