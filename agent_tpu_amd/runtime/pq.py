"""Product-quantized (PQ) resident corpora for ``map_search``: ``M`` bytes per row instead of ``4 D`` or ``2 D``.

**Training.** Every rank reads the same sample of the memory-mapped file, the rows
``sorted(randperm(total, seed 0)[:T])`` (normalised for the cosine metric), so no collective is needed and the
codebooks are equal on every rank and every world size. All ``M`` sub-spaces train together: the first 256 sample
rows' sub-vectors are the initial codewords; an iteration assigns with ``ops.pq_encode`` (bias ``-0.5 ||c||^2``:
the nearest codeword) and updates with int64 fixed-point sums (``ops.to_fixed`` at ``ops.fixed_shift``'s shift,
``index_add_``: integer adds have no order), finalized in fp64 and rounded once to fp32; an empty codeword keeps
its value. One-time PyTorch plumbing around the kernel, as ``runtime/ivf.py``.

**Encoding.** The rank's slice is streamed from the file in chunks of at most ``CHUNK_BYTES`` of fp32: load,
check, normalise, ``ops.pq_encode``. The fp32 slice is never resident: the peak is one chunk plus the codes.

**Cache.** The entry lives in ``runtime.search``'s LRU under the corpus key extended by ``("pq", M, T, t,
normalised?)``: it counts towards ``SEARCH_INDEX_LRU_SIZE`` and ``cache_info()`` reports its bytes (the codes and
the codebooks). On the GPU the codes are kept in the scan kernel's interleaved layout (``ops.PqCodes``: the last
64-row block padded), on a CPU engine row-major.

**Search.** ``ops.pq_lut`` -> the ADC scan -> ``sim_topk_merge`` (``ops.pq_scan_topk``).
"""
from __future__ import annotations

from typing import Any, Dict, NamedTuple, Optional, Tuple

import torch

from . import search as rs

SEED = 0
MIN_ROWS = 256  # one sample row per codeword at the least
MAX_TRAIN_ROWS = 1048576
DEFAULT_TRAIN_ROWS = 65536

#: the builder's input error (``ops/map_search.py`` lists it in ``PQ_ERRORS``)
ERRORS: Dict[str, str] = {
    "compression_too_large": "compressed corpus slice exceeds SEARCH_INDEX_MAX_GB of codes",
}


class PqIndex(NamedTuple):
    codes: torch.Tensor  # uint8: [count, M] row-major (CPU) or [ceil(count / 64), M / 4, 64, 4] interleaved (GPU)
    codebooks: torch.Tensor  # [M, 256, dsub] fp32; equal on every rank
    rows: int  # count: rows of the slice
    start: int  # row of the file that slice row 0 is
    total: int  # rows of the whole file
    cached: bool = False  # served from the LRU

    @property
    def subvectors(self) -> int:
        return int(self.codebooks.shape[0])


def default_train_rows(total: int) -> int:
    return min(total, DEFAULT_TRAIN_ROWS)


def sample_rows(total: int, T: int) -> torch.Tensor:
    """int64 ``[T]``: the training sample of a corpus of ``total`` rows, ascending (the same wherever it is drawn)."""
    gen = torch.Generator().manual_seed(SEED)
    return torch.sort(torch.randperm(total, generator=gen)[:T]).values


def _rows_to_device(arr, lo: int, hi: int, normalize: bool, device: torch.device, index=None) -> torch.Tensor:
    """fp32 rows of the memory-mapped file on ``device``, checked and (for cosine) normalised."""
    import numpy as np

    src = arr[index] if index is not None else arr[lo:hi]
    x = torch.from_numpy(np.array(src, order="C")).to(device).to(torch.float32)  # a copy: only these rows are read
    if not bool(torch.isfinite(x).all()):
        raise ValueError(rs.ERRORS["corpus_nonfinite"])
    return (rs.normalize_rows(x) if normalize else x).contiguous()


def train(sample: torch.Tensor, M: int, t: int) -> torch.Tensor:
    """Codebooks ``[M, 256, dsub]`` fp32 of ``t`` Lloyd iterations over ``sample [T, D]`` (``T >= 256``)."""
    from .. import ops

    T, D = sample.shape
    dsub = D // M
    books = sample[:ops.pq.CODEWORDS].view(ops.pq.CODEWORDS, M, dsub).permute(1, 0, 2).contiguous()
    s = ops.fixed_shift(int(T), float(sample.abs().max()))
    fixed = ops.to_fixed(sample, s).view(T * M, dsub)  # row i, sub-space m at i * M + m
    sub = torch.arange(M, device=sample.device, dtype=torch.int64) * ops.pq.CODEWORDS
    ones = torch.ones((T * M,), dtype=torch.int64, device=sample.device)
    for _ in range(t):
        codes = ops.pq_encode(sample, books, ops.pq_bias(books))
        slot = (codes.to(torch.int64) + sub[None, :]).reshape(-1)  # (sub-space, codeword) of every sub-vector
        sums = torch.zeros((M * ops.pq.CODEWORDS, dsub), dtype=torch.int64, device=sample.device).index_add_(0, slot, fixed)
        counts = torch.zeros((M * ops.pq.CODEWORDS,), dtype=torch.int64, device=sample.device).index_add_(0, slot, ones)
        mean = (sums.double() / (counts.clamp_min(1).double() * (2.0 ** s))[:, None]).to(torch.float32)
        books = torch.where((counts > 0)[:, None], mean, books.view(-1, dsub)).view(M, ops.pq.CODEWORDS, dsub).contiguous()
    return books


def _key(uri: Any, start: int, count: int, device: torch.device, M: int, T: int, t: int, normalize: bool):
    arr, path, st = rs.open_corpus(uri)
    total, dim = int(arr.shape[0]), int(arr.shape[1])
    start = max(0, min(int(start), total))
    count = total - start if count < 0 else max(0, min(int(count), total - start))
    key = (path, st.st_mtime_ns, st.st_size, start, count, str(device), "pq", int(M), int(T), int(t), bool(normalize))
    return key, arr, start, count, total, dim


def codes_bytes(count: int, M: int, device: torch.device) -> int:
    """Resident bytes of the codes of ``count`` rows on ``device`` (the GPU layout pads the last 64-row block)."""
    from ..ops.pq import BLOCK_ROWS

    rows = -(-count // BLOCK_ROWS) * BLOCK_ROWS if torch.device(device).type == "cuda" else count
    return rows * M


def encode_slice(arr, start: int, count: int, books: torch.Tensor, normalize: bool, device: torch.device) -> torch.Tensor:
    """The codes of rows ``[start, start + count)`` in the device's resident layout, chunk by chunk."""
    from .. import ops
    from ..ops.pq import BLOCK_ROWS

    M, dim = int(books.shape[0]), int(arr.shape[1])
    cuda = torch.device(device).type == "cuda"
    nb = -(-count // BLOCK_ROWS)
    if cuda:
        out = torch.zeros((nb, M // 4, BLOCK_ROWS, 4), dtype=torch.uint8, device=device)
    else:
        out = torch.empty((count, M), dtype=torch.uint8, device=device)
    bias = ops.pq_bias(books)
    rows = max(BLOCK_ROWS, rs.CHUNK_BYTES // (dim * 4) // BLOCK_ROWS * BLOCK_ROWS)  # whole blocks per chunk
    for lo in range(0, count, rows):
        hi = min(lo + rows, count)
        codes = ops.pq_encode(_rows_to_device(arr, start + lo, start + hi, normalize, device), books, bias)
        if cuda:
            part = ops.pq_interleave(codes).data
            out[lo // BLOCK_ROWS:lo // BLOCK_ROWS + part.shape[0]] = part
        else:
            out[lo:hi] = codes
    return out


def load_index(uri: Any, start: int = 0, count: int = -1, device: torch.device = torch.device("cpu"),
               subvectors: int = 8, train_rows: Optional[int] = None, train_iterations: int = 10,
               normalize: bool = True) -> PqIndex:
    """The cached index of rows ``[start, start + count)`` (``count < 0``: to the end) of the file, or a fresh
    build. No collective: under DP every rank trains the same codebooks from the same sample."""
    from .. import ops

    M, t = int(subvectors), int(train_iterations)
    total = rs.corpus_shape(uri)[0]
    T = default_train_rows(total) if train_rows is None else int(train_rows)
    key, arr, start, count, total, dim = _key(uri, start, count, device, M, T, t, normalize)
    with rs._lock:
        hit = rs._cache.get(key)
        if hit is not None:
            rs._cache.move_to_end(key)
            return PqIndex(hit[0], hit[1], count, start, total, True)
    if not ops.pq_ok(dim, M) or not MIN_ROWS <= T <= min(total, MAX_TRAIN_ROWS) or t < 1:
        raise ValueError("load_index: unsupported (dim, subvectors, train_rows, train_iterations)")
    if codes_bytes(count, M, device) > rs.max_bytes():  # before any allocation
        raise ValueError(ERRORS["compression_too_large"])
    sample = _rows_to_device(arr, 0, 0, normalize, device, index=sample_rows(total, T).numpy())
    books = train(sample, M, t)
    del sample
    codes = encode_slice(arr, start, count, books, normalize, device)
    with rs._lock:
        rs._cache[key] = (codes, books)
        rs._cache.move_to_end(key)
        while len(rs._cache) > rs.lru_capacity():
            rs._cache.popitem(last=False)
    return PqIndex(codes, books, count, start, total, False)


def row_major_codes(index: PqIndex) -> torch.Tensor:
    """uint8 ``[rows, M]`` of an index on either device (a copy on the GPU)."""
    from .. import ops

    if index.codes.dim() == 2:
        return index.codes
    return ops.pq_deinterleave(ops.PqCodes(index.codes, index.rows, index.subvectors))


def search(qvecs: torch.Tensor, index: PqIndex, k: int, id_base: int = 0) -> Tuple[torch.Tensor, torch.Tensor]:
    """(scores ``[nq, kk]`` fp32, ids ``[nq, kk]`` int64), ``kk = min(k, rows)``, of ``ops.sim_topk_pq`` on the
    index's device (its PyTorch twin on a CPU engine): ADC scores, ordered by (score desc, id asc). An empty slice
    (a DP rank beyond the corpus) gives ``kk = 0``."""
    from .. import ops

    dev = index.codebooks.device
    q = qvecs.to(device=dev, dtype=torch.float32).contiguous()
    if index.rows == 0 or q.shape[0] == 0:
        kk = min(k, index.rows)
        return (torch.empty((q.shape[0], kk), dtype=torch.float32, device=dev),
                torch.empty((q.shape[0], kk), dtype=torch.int64, device=dev))
    codes = index.codes if index.codes.dim() == 2 else ops.PqCodes(index.codes, index.rows, index.subvectors)
    return ops.sim_topk_pq(q, index.codebooks, codes, k, id_base)
