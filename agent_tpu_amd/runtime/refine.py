"""Exact re-scoring of a product-quantized search (``refine``): the originals of a slice beside its codes.

**Store.** While ``runtime/pq.py`` streams the slice chunk by chunk to encode it, the same chunks fill the refine
store: the rows as ``float32`` (normalised for the cosine metric, as the fp32-resident corpus keeps them) or as
``float16`` (as stored, with the fp32 ``row_scale = 1 / max(||row||_2, 1e-12)`` of the rounded values on the device,
as the fp16-resident corpus keeps them). ``store: "host"`` puts the rows in pinned host memory, which the kernel
reads through its device-visible address: nothing but the shortlisted rows crosses the link, and the device holds
the codes (and 4 bytes per row of scale for fp16 cosine) only. ``store: "device"`` keeps them on the device, for
small corpora and tests. On a CPU engine both are plain host tensors. The store is part of the PQ entry of
``runtime.search``'s LRU, under the entry's key extended by ``("refine", vectors, store)``.

**Search.** ``ops.pq_lut`` -> ``ops.pq_scan_segments`` (the scan kernel's un-merged per-segment lists: the
shortlist) -> ``ops.refine_topk``. The shortlist is a function of the slice and ``candidates`` alone.
"""
from __future__ import annotations

import os
from typing import Dict, NamedTuple, Optional, Tuple

import torch

from . import search as rs

VECTORS = ("float16", "float32")
STORES = ("host", "device")

#: the builder's input error (``ops/map_search.py`` lists it in ``REFINE_ERRORS``)
ERRORS: Dict[str, str] = {
    "refine_too_large": ("refine store of the corpus slice exceeds SEARCH_REFINE_MAX_GB of pinned host memory "
                         "(store 'device': SEARCH_INDEX_MAX_GB together with the codes)"),
}


def max_bytes() -> int:
    return int(float(os.getenv("SEARCH_REFINE_MAX_GB", "64")) * 2 ** 30)


class Store(NamedTuple):
    vectors: torch.Tensor  # [count, dim] fp32 or fp16: pinned host memory, or on the device
    scale: Optional[torch.Tensor]  # [count] fp32 on the device: the cosine row scale of fp16 vectors

    def fill(self, lo: int, hi: int, raw: torch.Tensor, x: torch.Tensor) -> None:
        """Rows ``[lo, hi)`` from one chunk on the device: ``raw`` as the file holds them (fp32), ``x`` normalised
        for the cosine metric (``raw`` itself for dot)."""
        if self.vectors.dtype == torch.float32:
            self.vectors[lo:hi].copy_(x)
            return
        part = raw.to(torch.float16)  # a float32 file: round to nearest; past the range: inf
        if not bool(torch.isfinite(part).all()):
            raise ValueError(rs.F16_ERRORS["corpus_f16_range"])
        self.vectors[lo:hi].copy_(part)
        if self.scale is not None:  # runtime.search._load_f16's scale: from the rounded values, summed in fp64
            self.scale[lo:hi] = part.double().norm(dim=1).clamp_min(rs.EPS).reciprocal().to(torch.float32)


def store_bytes(count: int, dim: int, vectors: str) -> int:
    return count * dim * (2 if vectors == "float16" else 4)


def check_size(count: int, dim: int, vectors: str, where: str, normalize: bool, device: torch.device,
               codes_bytes: int) -> None:
    """Before any allocation: a host store against ``SEARCH_REFINE_MAX_GB``, a device store (and an fp16 scale)
    against ``SEARCH_INDEX_MAX_GB`` together with the codes."""
    rows = store_bytes(count, dim, vectors)
    scale = count * 4 if vectors == "float16" and normalize else 0
    host = where == "host" and torch.device(device).type == "cuda"
    if (host and rows > max_bytes()) or codes_bytes + scale + (0 if host else rows) > rs.max_bytes():
        raise ValueError(ERRORS["refine_too_large"])


def allocate(count: int, dim: int, vectors: str, where: str, normalize: bool, device: torch.device) -> Store:
    dtype = torch.float16 if vectors == "float16" else torch.float32
    if where == "host" and torch.device(device).type == "cuda":
        vec = torch.empty((count, dim), dtype=dtype, pin_memory=True)
    else:
        vec = torch.empty((count, dim), dtype=dtype, device=device)
    scale = torch.empty((count,), dtype=torch.float32, device=device) if vectors == "float16" and normalize else None
    return Store(vec, scale)


def search(qvecs: torch.Tensor, index, k: int, candidates: int, id_base: int = 0
           ) -> Tuple[torch.Tensor, torch.Tensor, int]:
    """(scores ``[nq, k]`` fp32, ids ``[nq, k]`` int64, rows re-scored per query) of a ``runtime.pq.PqIndex`` with a
    store: the exact scores of the slice's shortlist of ``candidates`` rows, in the (score desc, id asc) order,
    padded with ``(-inf, 2^62)`` past the shortlist's live rows. An empty slice (a DP rank beyond the corpus) gives
    padding only."""
    from .. import ops

    dev = index.codebooks.device
    q = qvecs.to(device=dev, dtype=torch.float32).contiguous()
    if index.rows == 0 or q.shape[0] == 0:
        return (torch.full((q.shape[0], k), float("-inf"), dtype=torch.float32, device=dev),
                torch.full((q.shape[0], k), ops.search.PAD_ID, dtype=torch.int64, device=dev), 0)
    G = candidates // ops.refine.SEGMENT_LIST
    codes = index.codes if index.codes.dim() == 2 else ops.PqCodes(index.codes, index.rows, index.subvectors)
    cand = ops.pq_scan_segments(ops.pq_lut(q, index.codebooks), codes, G)
    s, i = ops.refine_topk(q, index.store.vectors, cand, k, id_base, row_scale=index.store.scale)
    return s, i, ops.shortlist_rows(index.rows, G)
