"""Inverted index over learned sparse (SPLADE) term weights and its top-k scan (``csrc/kernels/sparse_index.hip``).

**Score.** A document weight is stored as fp16 (the file's fp32 rounded to nearest even, once); a query weight stays
fp32. For a term shared by query and row

    c = rint(double(wq) * double(wd) * 2^32)   as int64 (the product is exact in fp64; ties to even)

a row's ``acc`` is the integer sum of its ``c`` (it has no order) and ``score = float(acc) * 2^-32``: one
int64 -> fp32 rounding, then an exact scaling. A row is a hit if ``acc > 0``; rows that share no term, or whose sum
rounds to 0, are never returned. Hits are ranked by (score descending, row id ascending) on the fp32 score, the
project's total order (``better()`` of ``atpu/topk.h``). Weights on both sides are finite and in ``(0, 256]``; with at
most 1024 query terms ``acc < 2^58``. The ``_ref`` twins (plain PyTorch int64 math, the CPU path) give identical bits,
and a result does not depend on the batch, on ``splits`` or on how the rows are cut into slices.

**Index** (:class:`SparseIndex`). Rows are cut into blocks of ``BLOCK_ROWS = 8192`` consecutive rows; inside a block
the postings are grouped by token. A posting is one 32-bit word: the low 16 bits are ``row - block_base``, the high
16 bits the fp16 weight bits. ``offsets [nblocks, V + 1]`` (int32) are relative to the block's start (a block holds
fewer than 2^23 postings) and ``block_start [nblocks + 1]`` (int64) says where a block's postings begin. The order of
the postings inside one (block, token) segment is unspecified (on the GPU it is whatever the atomics gave): integer
sums make every result independent of it.

Queries are CSR: ``q_ptr [nq + 1]`` int64, ``q_tok`` int32 and ``q_w`` fp32, at most ``MAX_QUERY_TERMS`` distinct
tokens per query.
"""
from __future__ import annotations

from typing import NamedTuple, Optional, Sequence, Tuple

import torch

from .._native import native, ptr, launch_stream
from ._util import check, same_device
from .search import MAX_K, MAX_ROWS, MAX_SPLITS, PAD_ID, _NO_ROW, _ivf_pad

BLOCK_ROWS = 8192  # kSparseBlockRows
MAX_QUERY_TERMS = 1024  # kSparseMaxTerms: also the most entries of a corpus row
MAX_WEIGHT = 256.0
_SCALE = 4294967296.0  # 2^32


class SparseIndex(NamedTuple):
    """The inverted index of ``rows`` rows over a vocabulary of ``V`` tokens (layout: the module docstring). The
    order of the postings inside one (block, token) segment is unspecified; no result depends on it."""
    postings: torch.Tensor  # int32 [nnz]: (fp16 weight bits << 16) | (row - block_base)
    offsets: torch.Tensor  # int32 [nblocks, V + 1], relative to the block's start
    block_start: torch.Tensor  # int64 [nblocks + 1]
    rows: int
    V: int

    @property
    def nnz(self) -> int:
        return int(self.postings.numel())


def _is_int(x) -> bool:
    return isinstance(x, int) and not isinstance(x, bool)


def _check_csr(ptr_t, tok, w, V, what, names) -> int:
    """Shape, dtype and value checks of a CSR triple (rows or queries); the count of its rows."""
    p, t, d = names
    check(_is_int(V) and 1 <= V < 2 ** 31 - 1, f"{what}: V must be in [1, 2^31 - 2]")
    check(isinstance(ptr_t, torch.Tensor) and ptr_t.dim() == 1 and ptr_t.dtype == torch.int64 and ptr_t.numel() >= 1
          and ptr_t.is_contiguous(), f"{what}: {p} must be a contiguous int64 [n + 1]")
    check(isinstance(tok, torch.Tensor) and tok.dim() == 1 and tok.dtype == torch.int32 and tok.is_contiguous(),
          f"{what}: {t} must be a contiguous int32 [nnz]")
    check(isinstance(w, torch.Tensor) and w.dtype == torch.float32 and w.shape == tok.shape and w.is_contiguous(),
          f"{what}: {d} must be a contiguous fp32 [nnz]")
    same_device(ptr_t, tok, w)
    n, nnz = int(ptr_t.numel()) - 1, int(tok.numel())
    lens = ptr_t[1:] - ptr_t[:-1]
    check(int(ptr_t[0]) == 0 and int(ptr_t[-1]) == nnz and (n == 0 or int(lens.min()) >= 0),
          f"{what}: {p} must rise from 0 to nnz")
    check(n == 0 or int(lens.max()) <= MAX_QUERY_TERMS, f"{what}: at most {MAX_QUERY_TERMS} entries per row")
    if nnz:
        lo, hi = torch.aminmax(tok)
        check(int(lo) >= 0 and int(hi) < V, f"{what}: {t} must be in [0, V)")
        wlo, whi = torch.aminmax(w)  # a NaN propagates and fails both comparisons
        check(float(wlo) > 0.0 and float(whi) <= MAX_WEIGHT, f"{what}: {d} must be finite and in (0, 256]")
        row = torch.repeat_interleave(torch.arange(n, device=tok.device), lens, output_size=nnz)
        key = torch.sort(row * V + tok.to(torch.int64)).values
        check(nnz < 2 or bool((key[1:] != key[:-1]).all()), f"{what}: the tokens of a row must be distinct")
    return n


def _check_build(indptr, indices, data, V) -> int:
    N = _check_csr(indptr, indices, data, V, "sparse_index_build", ("indptr", "indices", "data"))
    check(1 <= N <= MAX_ROWS, "sparse_index_build: N must be in [1, 2^31 - 256]")
    return N


def _layout(counts: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """(offsets, block_start) of the per-(block, token) posting counts ``[nblocks, V]``."""
    nb, V = counts.shape
    csum = torch.cumsum(counts, dim=1, dtype=torch.int64)
    check(int(csum[:, -1].max()) < 2 ** 23, "sparse_index_build: a block must hold fewer than 2^23 postings")
    offsets = torch.zeros((nb, V + 1), dtype=torch.int32, device=counts.device)
    offsets[:, 1:] = csum
    block_start = torch.zeros((nb + 1,), dtype=torch.int64, device=counts.device)
    block_start[1:] = torch.cumsum(csum[:, -1], dim=0)
    return offsets, block_start


def sparse_index_build_ref(indptr: torch.Tensor, indices: torch.Tensor, data: torch.Tensor, V: int) -> SparseIndex:
    """PyTorch twin of :func:`sparse_index_build` and the CPU path (segments in ascending row order)."""
    N = _check_build(indptr, indices, data, V)
    nb = -(-N // BLOCK_ROWS)
    row = torch.repeat_interleave(torch.arange(N, device=indices.device), indptr[1:] - indptr[:-1],
                                  output_size=int(indices.numel()))
    hb = data.to(torch.float16).view(torch.int16).to(torch.int64) & 0xffff
    keep = hb != 0  # a weight that rounds to fp16 zero is dropped
    row, tok, hb = row[keep], indices[keep].to(torch.int64), hb[keep]
    key = (row // BLOCK_ROWS) * V + tok
    order = torch.sort(key, stable=True).indices
    words = ((hb << 16) | (row % BLOCK_ROWS))[order].to(torch.int32)
    offsets, block_start = _layout(torch.bincount(key, minlength=nb * V).view(nb, V))
    return SparseIndex(words, offsets, block_start, N, V)


def sparse_index_build(indptr: torch.Tensor, indices: torch.Tensor, data: torch.Tensor, V: int) -> SparseIndex:
    """The :class:`SparseIndex` of ``N`` rows given as CSR (``indptr [N + 1]`` int64 from 0, ``indices`` int32 token
    ids in ``[0, V)``, distinct within a row and at most 1024 of them, ``data`` fp32 weights in ``(0, 256]``; all
    checked here, before any launch). An entry whose fp16 weight is zero is dropped. Built block by block: count,
    exclusive scan, fill."""
    N = _check_build(indptr, indices, data, V)
    nnz = int(indices.numel())
    if not indices.is_cuda or nnz == 0:
        return sparse_index_build_ref(indptr, indices, data, V)
    nb, dev = -(-N // BLOCK_ROWS), indices.device
    stream, nat = launch_stream(indices), native()
    counts = torch.zeros((nb, V), dtype=torch.int32, device=dev)
    blocks = [(b, min(BLOCK_ROWS, N - b * BLOCK_ROWS)) for b in range(nb)]
    for b, rows in blocks:
        nat.postings_count(ptr(indptr) + 8 * b * BLOCK_ROWS, ptr(indices), ptr(data), ptr(counts[b]), rows, V, nnz, stream)
    offsets, block_start = _layout(counts)
    starts = block_start.tolist()
    postings = torch.empty((starts[-1],), dtype=torch.int32, device=dev)
    cursor = offsets[:, :V].clone(memory_format=torch.contiguous_format)  # a copy also at one block: fill advances it
    for b, rows in blocks:
        cap = starts[b + 1] - starts[b]
        if cap:
            nat.postings_fill(ptr(indptr) + 8 * b * BLOCK_ROWS, ptr(indices), ptr(data), ptr(cursor[b]),
                              ptr(postings) + 4 * starts[b], rows, V, nnz, cap, stream)
    return SparseIndex(postings, offsets, block_start, N, V)


def sparse_index_cat(parts: Sequence[SparseIndex]) -> SparseIndex:
    """One index of consecutive row groups, every group but the last a whole number of blocks (a streamed build)."""
    check(len(parts) >= 1 and all(p.V == parts[0].V for p in parts)
          and all(p.rows % BLOCK_ROWS == 0 for p in parts[:-1]),
          "sparse_index_cat: groups of whole blocks over one vocabulary")
    if len(parts) == 1:
        return parts[0]
    starts, base = [parts[0].block_start[:1]], 0
    for p in parts:
        starts.append(p.block_start[1:] + base)
        base += p.nnz
    return SparseIndex(torch.cat([p.postings for p in parts]), torch.cat([p.offsets for p in parts]),
                       torch.cat(starts), sum(p.rows for p in parts), parts[0].V)


def check_queries(q_ptr: torch.Tensor, q_tok: torch.Tensor, q_w: torch.Tensor, V: int) -> int:
    """The value checks of a query batch (tokens in ``[0, V)`` and distinct within a query, at most 1024 of them,
    weights finite and in ``(0, 256]``); the count of queries. They read the values, so on the GPU path they are the
    caller's to make (the kernel clamps every index and never leaves its tensors)."""
    return _check_csr(q_ptr, q_tok, q_w, V, "sparse_scan_topk", ("q_ptr", "q_tok", "q_w"))


def _check_scan(index, q_ptr, q_tok, q_w, k, id_base, splits) -> int:
    what = "sparse_scan_topk"
    check(isinstance(index, SparseIndex) and _is_int(index.rows) and 1 <= index.rows <= MAX_ROWS
          and _is_int(index.V) and index.V >= 1, f"{what}: index must be a SparseIndex of 1 to 2^31 - 256 rows")
    nb = -(-index.rows // BLOCK_ROWS)
    check(index.postings.dtype == torch.int32 and index.postings.dim() == 1 and index.postings.is_contiguous()
          and index.offsets.dtype == torch.int32 and index.offsets.shape == (nb, index.V + 1)
          and index.offsets.is_contiguous() and index.block_start.dtype == torch.int64
          and index.block_start.shape == (nb + 1,) and index.block_start.is_contiguous(),
          f"{what}: postings int32 [nnz], offsets int32 [nblocks, V + 1], block_start int64 [nblocks + 1], contiguous")
    check(isinstance(q_ptr, torch.Tensor) and q_ptr.dim() == 1 and q_ptr.dtype == torch.int64 and q_ptr.numel() >= 1
          and q_ptr.is_contiguous(), f"{what}: q_ptr must be a contiguous int64 [nq + 1]")
    check(isinstance(q_tok, torch.Tensor) and q_tok.dim() == 1 and q_tok.dtype == torch.int32 and q_tok.is_contiguous()
          and isinstance(q_w, torch.Tensor) and q_w.dtype == torch.float32 and q_w.shape == q_tok.shape
          and q_w.is_contiguous(), f"{what}: q_tok int32 and q_w fp32 must be contiguous [nterms]")
    same_device(index.postings, index.offsets, index.block_start, q_ptr, q_tok, q_w)
    check(_is_int(k) and 1 <= k <= MAX_K, f"{what}: k must be in [1, 32]")
    check(_is_int(id_base) and 0 <= id_base < 2 ** 61, f"{what}: id_base must be in [0, 2^61)")
    check(splits is None or (_is_int(splits) and 1 <= splits <= MAX_SPLITS),
          f"{what}: splits must be in [1, {MAX_SPLITS}]")
    return int(q_ptr.numel()) - 1


def _padding(nq: int, k: int, device) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    return (torch.full((nq, k), float("-inf"), dtype=torch.float32, device=device),
            torch.full((nq, k), PAD_ID, dtype=torch.int64, device=device),
            torch.zeros((nq,), dtype=torch.int64, device=device))


def sparse_scan_topk_ref(index: SparseIndex, q_ptr: torch.Tensor, q_tok: torch.Tensor, q_w: torch.Tensor, k: int,
                         id_base: int = 0) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """PyTorch twin of :func:`sparse_scan_topk` and the CPU path: int64 sums per row, then the stable sort."""
    nq = _check_scan(index, q_ptr, q_tok, q_w, k, id_base, None)
    check_queries(q_ptr, q_tok, q_w, index.V)
    dev, N, V = q_tok.device, index.rows, index.V
    scores, ids, counts = _padding(nq, k, dev)
    if nq == 0 or index.nnz == 0:
        return scores, ids, counts
    seg = (index.offsets[:, 1:] - index.offsets[:, :-1]).reshape(-1).to(torch.int64)
    key = torch.repeat_interleave(torch.arange(seg.numel(), device=dev), seg, output_size=index.nnz)
    words = index.postings.to(torch.int64)
    row = (key // V) * BLOCK_ROWS + (words & 0xffff)
    tok = key % V
    wd = ((words >> 16) & 0xffff).to(torch.int16).view(torch.float16).to(torch.float64)
    ptrs = q_ptr.tolist()
    for i in range(nq):
        wq = torch.zeros((V,), dtype=torch.float64, device=dev)
        wq[q_tok[ptrs[i]:ptrs[i + 1]].to(torch.int64)] = q_w[ptrs[i]:ptrs[i + 1]].to(torch.float64)
        sel = wq[tok] != 0
        c = torch.round(wq[tok[sel]] * wd[sel] * _SCALE).to(torch.int64)  # exact product, ties to even
        acc = torch.zeros((N,), dtype=torch.int64, device=dev).index_add_(0, row[sel], c)
        s = torch.where(acc > 0, acc.to(torch.float32) * (1.0 / _SCALE), torch.full((), float("-inf"), device=dev))
        order = torch.sort(s, descending=True, stable=True).indices[:k]
        live = s[order] > float("-inf")
        n = int(live.sum())
        scores[i, :n], ids[i, :n], counts[i] = s[order][:n], order[:n] + int(id_base), n
    return scores, ids, counts


def _auto_items(nq: int, nblocks: int, device: torch.device) -> int:
    """Workgroups per query: about two per CU in all (two fit a CU's LDS). Tuning only."""
    cus = torch.cuda.get_device_properties(device).multi_processor_count
    return max(1, min(MAX_SPLITS, nblocks, -(-2 * cus // nq)))


def sparse_scan_topk(index: SparseIndex, q_ptr: torch.Tensor, q_tok: torch.Tensor, q_w: torch.Tensor, k: int,
                     id_base: int = 0, splits: Optional[int] = None
                     ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """(scores ``[nq, k]`` fp32, ids ``[nq, k]`` int64, counts ``[nq]``): per query the ``k`` hits with the largest
    score in the order (score desc, id asc), ``ids = id_base + row``. The columns past ``counts[i]`` (fewer than ``k``
    rows share a term with the query) hold ``(-inf, PAD_ID)``. The result does not depend on ``splits`` (tests and
    benches), on the batch or on the order of the postings inside a segment. :func:`check_queries` is the caller's on
    the GPU path."""
    nq = _check_scan(index, q_ptr, q_tok, q_w, k, id_base, splits)
    if not q_tok.is_cuda:
        return sparse_scan_topk_ref(index, q_ptr, q_tok, q_w, k, id_base)
    if nq == 0 or index.nnz == 0 or q_tok.numel() == 0:
        return _padding(nq, k, q_tok.device)
    check(nq <= 65535, "sparse_scan_topk: at most 65535 queries per call")
    nb, dev = -(-index.rows // BLOCK_ROWS), q_tok.device
    items = min(splits, nb) if splits is not None else _auto_items(nq, nb, dev)
    ws = torch.empty((nq, items, k, 2), dtype=torch.float32, device=dev)
    scores = torch.empty((nq, k), dtype=torch.float32, device=dev)
    ids = torch.empty((nq, k), dtype=torch.int64, device=dev)
    stream, nat = launch_stream(q_tok), native()
    nat.sparse_scan_partial(ptr(index.postings), ptr(index.offsets), ptr(index.block_start), ptr(q_ptr), ptr(q_tok),
                            ptr(q_w), ptr(ws), nq, index.rows, index.V, index.nnz, int(q_tok.numel()), k, items, stream)
    nat.sim_topk_merge(ptr(ws), ptr(scores), ptr(ids), nq, items, k, k, int(id_base), stream)
    return _ivf_pad(scores, ids, ids == int(id_base) + _NO_ROW)  # the merge's empty entries: (-inf, id_base + kNoRow)
