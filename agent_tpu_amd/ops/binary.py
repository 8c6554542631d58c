"""Binary (sign-bit) rows scored by the Hamming distance (``csrc/kernels/sim_binary.hip``).

A row of ``D`` floats is stored as ``D`` bits in ``W = D / 32`` words: bit ``b`` of word ``w`` is
``x[row, 32 w + b] > thr[32 w + b]`` (a plain comparison: ``-0.0``, ``+0.0`` and NaN give 0 against a zero threshold).
A query is packed the same way and

    score(q, r) = D - 2 * popcount(qbits XOR rbits)

the dot product of the two +-1 vectors, as fp32: an exact integer with ``|score| <= 1024``, larger is better. The
search returns the project's total order (score descending, id ascending: ``better()`` of ``atpu/topk.h``) through
``sim_topk``'s workspace and merge. Integer scores have no rounding, so the ``_ref`` twins (plain PyTorch, the CPU
path) give identical results, and the result does not depend on the batch, on ``splits`` / ``parts`` or on how the
rows are cut into slices.

Words are ``int32`` tensors (the bit pattern of the kernel's ``uint32``). Queries are row-major ``[nq, W]``; the scan
reads the corpus in its own layout (:class:`BinaryCodes`): blocks of 64 rows, inside a block word ``w`` of the 64
rows side by side, so that a wave's load is one contiguous 256 bytes: the bytes of ``ops.PqCodes`` at ``M = 4 W``.

:func:`hamming_scan_segments` builds the shortlist that :func:`ops.refine_topk` re-scores exactly: the rows are cut
into ``G`` segments (``ops.segment_rows``) and the list is the Hamming top-32 of every segment in the total order,
the contract of ``ops.pq_scan_segments``. Every segment is scanned by ``parts`` workgroups per query tile, so the
shortlist is computed by the full grid whatever ``G`` is.
"""
from __future__ import annotations

from typing import NamedTuple, Optional, Tuple, Union

import torch

from .._native import native, ptr, launch_stream
from ._util import check, same_device
from .pq import BLOCK_ROWS
from .refine import SEGMENT_LIST, segment_rows
from .search import MAX_K, MAX_ROWS, MAX_SPLITS, _NO_ROW, sim_topk_ok

QUERY_TILE = 32  # kHamTile: queries of one work item
STEP_BLOCKS = 16  # blocks of one workgroup step: 8 waves x 2 blocks


def binary_ok(D: int) -> bool:
    """Dims the kernels take: those of ``sim_topk`` (a multiple of 64 from 64 to 1024), so ``W`` is even, <= 32."""
    return isinstance(D, int) and not isinstance(D, bool) and sim_topk_ok(D, 1)


class BinaryCodes(NamedTuple):
    """The scan kernel's layout of ``rows`` rows of ``D`` bits."""
    data: torch.Tensor  # int32 [ceil(rows / 64), D / 32, 64]: word (b, w, lane) = bits(64 b + lane, w); padding rows 0
    rows: int
    D: int


def binary_interleave(bits: torch.Tensor) -> BinaryCodes:
    """:class:`BinaryCodes` of row-major ``bits [N, W]`` (a copy; the rows past ``N`` of the last block are zero)."""
    check(isinstance(bits, torch.Tensor) and bits.dim() == 2 and bits.dtype == torch.int32 and bits.shape[1] >= 1,
          "binary_interleave: bits must be int32 [N, W]")
    N, W = bits.shape
    nb = (N + BLOCK_ROWS - 1) // BLOCK_ROWS
    full = bits if N == nb * BLOCK_ROWS else torch.cat(
        [bits, torch.zeros((nb * BLOCK_ROWS - N, W), dtype=torch.int32, device=bits.device)])
    return BinaryCodes(full.view(nb, BLOCK_ROWS, W).permute(0, 2, 1).contiguous(), int(N), 32 * int(W))


def binary_deinterleave(bc: BinaryCodes) -> torch.Tensor:
    """Row-major ``[rows, W]`` of a :class:`BinaryCodes` (a copy)."""
    nb, W = bc.data.shape[0], bc.data.shape[1]
    return bc.data.permute(0, 2, 1).reshape(nb * BLOCK_ROWS, W)[:bc.rows].contiguous()


def _check_pack(x, thr):
    check(isinstance(x, torch.Tensor) and x.dim() == 2 and x.dtype == torch.float32 and x.is_contiguous(),
          "binary_pack: x must be a contiguous fp32 [n, D]")
    D = int(x.shape[1])
    check(binary_ok(D), f"binary_pack: unsupported shape D={D}")
    check(isinstance(thr, torch.Tensor) and thr.dtype == torch.float32 and thr.shape == (D,) and thr.is_contiguous(),
          "binary_pack: thr must be a contiguous fp32 [D]")
    check(x.shape[0] <= MAX_ROWS, "binary_pack: n must be at most 2^31 - 256")
    same_device(x, thr)
    return D


def binary_pack_ref(x: torch.Tensor, thr: torch.Tensor, interleave: bool = False
                    ) -> Union[torch.Tensor, BinaryCodes]:
    """PyTorch twin of :func:`binary_pack` and the CPU path."""
    D = _check_pack(x, thr)
    weight = torch.tensor([1 << b for b in range(31)] + [-2 ** 31], dtype=torch.int32, device=x.device)
    bits = ((x > thr[None, :]).view(x.shape[0], D // 32, 32).to(torch.int32) * weight).sum(dim=2, dtype=torch.int32)
    return binary_interleave(bits) if interleave else bits


def binary_pack(x: torch.Tensor, thr: torch.Tensor, interleave: bool = False) -> Union[torch.Tensor, BinaryCodes]:
    """The sign bits ``x > thr`` of ``x [n, D]``: int32 ``[n, D / 32]`` row-major (queries), or with ``interleave``
    the :class:`BinaryCodes` of the rows (a corpus)."""
    D = _check_pack(x, thr)
    n, W = int(x.shape[0]), D // 32
    if not x.is_cuda or n == 0:
        return binary_pack_ref(x, thr, interleave)
    nb = (n + BLOCK_ROWS - 1) // BLOCK_ROWS
    out = torch.empty((nb, W, BLOCK_ROWS) if interleave else (n, W), dtype=torch.int32, device=x.device)
    native().binary_pack(ptr(x), ptr(thr), ptr(out), n, D, bool(interleave), launch_stream(x))
    return BinaryCodes(out, n, D) if interleave else out


def _check_scan(qbits, codes, D, k, id_base, splits, what="hamming_scan_topk"):
    check(binary_ok(D), f"{what}: unsupported shape D={D}")
    W = D // 32
    check(isinstance(qbits, torch.Tensor) and qbits.dim() == 2 and qbits.dtype == torch.int32 and qbits.shape[1] == W
          and qbits.is_contiguous(), f"{what}: qbits must be a contiguous int32 [nq, D / 32]")
    if isinstance(codes, BinaryCodes):
        N = codes.rows
        check(isinstance(N, int) and codes.D == D and codes.data.dtype == torch.int32 and codes.data.is_contiguous()
              and codes.data.shape == ((N + BLOCK_ROWS - 1) // BLOCK_ROWS, W, BLOCK_ROWS),
              f"{what}: BinaryCodes must be a contiguous int32 [ceil(rows / 64), D / 32, 64] of the same D")
        same_device(qbits, codes.data)
    else:
        check(isinstance(codes, torch.Tensor) and codes.dim() == 2 and codes.dtype == torch.int32
              and codes.shape[1] == W and codes.is_contiguous(),
              f"{what}: codes must be a contiguous int32 [N, D / 32] (or a BinaryCodes)")
        N = int(codes.shape[0])
        same_device(qbits, codes)
    check(isinstance(k, int) and not isinstance(k, bool) and 1 <= k <= MAX_K, f"{what}: k must be in [1, 32]")
    check(1 <= N <= MAX_ROWS, f"{what}: N must be in [1, 2^31 - 256]")
    check(isinstance(id_base, int) and 0 <= id_base < 2 ** 61, f"{what}: id_base must be in [0, 2^61)")
    check(splits is None or (isinstance(splits, int) and not isinstance(splits, bool) and 1 <= splits <= MAX_SPLITS),
          f"{what}: splits / parts must be in [1, {MAX_SPLITS}]")
    return N


def _signs(bits: torch.Tensor) -> torch.Tensor:
    """fp32 ``[n, 32 W]`` of +-1: bit 1 -> +1."""
    sh = torch.arange(32, dtype=torch.int32, device=bits.device)
    return (((bits[:, :, None] >> sh) & 1).reshape(bits.shape[0], -1) * 2 - 1).to(torch.float32)


def _scores_ref(qbits: torch.Tensor, codes: Union[torch.Tensor, BinaryCodes]) -> torch.Tensor:
    rows = binary_deinterleave(codes) if isinstance(codes, BinaryCodes) else codes
    return _signs(qbits) @ _signs(rows).T  # integers of magnitude <= 1024: exact in fp32 in any order


def hamming_scan_topk_ref(qbits: torch.Tensor, codes: Union[torch.Tensor, BinaryCodes], D: int, k: int,
                          id_base: int = 0) -> Tuple[torch.Tensor, torch.Tensor]:
    """PyTorch twin of :func:`hamming_scan_topk` and the CPU path: the +-1 product, then the stable sort."""
    N = _check_scan(qbits, codes, D, k, id_base, None)
    s = _scores_ref(qbits, codes)
    order = torch.sort(s, dim=1, descending=True, stable=True).indices[:, :min(k, N)]
    return torch.gather(s, 1, order), order.to(torch.int64) + int(id_base)


def _auto_parts(nq: int, seg_blocks: int, segments: int, device: torch.device) -> int:
    """Workgroups per (segment, query tile): about 4 work items per CU in all, and no part under one workgroup step
    (16 blocks). Tuning only."""
    cus = torch.cuda.get_device_properties(device).multi_processor_count
    tiles = -(-nq // QUERY_TILE)
    return max(1, min(MAX_SPLITS, -(-4 * cus // (segments * tiles)), seg_blocks // STEP_BLOCKS))


def hamming_scan_topk(qbits: torch.Tensor, codes: Union[torch.Tensor, BinaryCodes], D: int, k: int, id_base: int = 0,
                      splits: Optional[int] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """(scores ``[nq, kk]`` fp32, ids ``[nq, kk]`` int64), ``kk = min(k, N)``: the rows with the largest
    ``D - 2 * hamming`` against every query's bits, ordered by (score desc, id asc), ``ids = id_base + row``.
    ``codes``: row-major int32 ``[N, W]`` (interleaved here, on every call) or a :class:`BinaryCodes`. The result
    does not depend on ``splits`` (tests and benches) or on the batch."""
    N = _check_scan(qbits, codes, D, k, id_base, splits)
    nq, kk = int(qbits.shape[0]), min(k, N)
    if nq == 0:
        return (torch.empty((0, kk), dtype=torch.float32, device=qbits.device),
                torch.empty((0, kk), dtype=torch.int64, device=qbits.device))
    if not qbits.is_cuda:
        return hamming_scan_topk_ref(qbits, codes, D, k, id_base)
    bc = codes if isinstance(codes, BinaryCodes) else binary_interleave(codes)
    nblocks = (N + BLOCK_ROWS - 1) // BLOCK_ROWS
    parts = splits if splits is not None else _auto_parts(nq, nblocks, 1, qbits.device)
    ws = torch.empty((nq, parts, k, 2), dtype=torch.float32, device=qbits.device)
    scores = torch.empty((nq, kk), dtype=torch.float32, device=qbits.device)
    ids = torch.empty((nq, kk), dtype=torch.int64, device=qbits.device)
    stream, nat = launch_stream(qbits), native()
    nat.hamming_scan_partial(ptr(qbits), ptr(bc.data), ptr(ws), nq, N, D, k, nblocks, parts, stream)
    nat.sim_topk_merge(ptr(ws), ptr(scores), ptr(ids), nq, parts, k, kk, int(id_base), stream)
    return scores, ids


def _check_segments(qbits, codes, D, G, parts):
    check(isinstance(G, int) and not isinstance(G, bool) and 1 <= G <= MAX_SPLITS,
          f"hamming_scan_segments: G must be in [1, {MAX_SPLITS}]")
    return _check_scan(qbits, codes, D, MAX_K, 0, parts, "hamming_scan_segments")


def hamming_scan_segments_ref(qbits: torch.Tensor, codes: Union[torch.Tensor, BinaryCodes], D: int, G: int
                              ) -> torch.Tensor:
    """PyTorch twin of :func:`hamming_scan_segments` and the CPU path: the stable sort per segment."""
    N = _check_segments(qbits, codes, D, G, None)
    s = _scores_ref(qbits, codes)
    nq, seg = s.shape[0], segment_rows(N, G)
    P = -(-N // seg)
    flat = torch.full((nq, P * seg), float("-inf"), dtype=s.dtype, device=s.device)  # seg >= 64 > 32 columns each
    flat[:, :N] = s
    order = torch.sort(flat.view(nq, P, seg), dim=2, descending=True, stable=True).indices[:, :, :SEGMENT_LIST]
    ids = order + (torch.arange(P, device=s.device) * seg)[None, :, None]
    ids = torch.where(ids < N, ids, torch.full_like(ids, _NO_ROW))
    return ids.to(torch.int32).reshape(nq, P * SEGMENT_LIST)


def hamming_scan_segments(qbits: torch.Tensor, codes: Union[torch.Tensor, BinaryCodes], D: int, G: int,
                          parts: Optional[int] = None) -> torch.Tensor:
    """int32 ``[nq, 32 P]``, ``P = ceil(N / segment_rows(N, G)) <= G``: per segment the 32 rows with the largest score
    in the total order (row ids of the slice; empty slots hold the no-row id ``0x7fffffff``; no duplicates). Every
    segment is scanned in ``parts`` pieces (``None``: enough to fill the device) whose lists ``sim_topk_merge``
    reduces per (query, segment); the result does not depend on ``parts``. On the GPU it is every other element of
    a buffer, which :func:`ops.refine_topk` reads as it lies."""
    N = _check_segments(qbits, codes, D, G, parts)
    nq = int(qbits.shape[0])
    if not qbits.is_cuda or nq == 0:
        return hamming_scan_segments_ref(qbits, codes, D, G)
    bc = codes if isinstance(codes, BinaryCodes) else binary_interleave(codes)
    seg_blocks = segment_rows(N, G) // BLOCK_ROWS
    P = -(-((N + BLOCK_ROWS - 1) // BLOCK_ROWS) // seg_blocks)
    if parts is None:
        parts = _auto_parts(nq, seg_blocks, P, qbits.device)
    ws = torch.empty((nq, P * parts, SEGMENT_LIST, 2), dtype=torch.float32, device=qbits.device)
    stream, nat = launch_stream(qbits), native()
    nat.hamming_scan_partial(ptr(qbits), ptr(bc.data), ptr(ws), nq, N, D, SEGMENT_LIST, seg_blocks, parts, stream)
    if parts == 1:  # the workspace holds the segments' lists already: its row halves
        return ws.view(torch.int32).view(nq, P * SEGMENT_LIST, 2)[:, :, 1]
    scores = torch.empty((nq * P, SEGMENT_LIST), dtype=torch.float32, device=qbits.device)
    ids = torch.empty((nq * P, SEGMENT_LIST), dtype=torch.int64, device=qbits.device)
    nat.sim_topk_merge(ptr(ws), ptr(scores), ptr(ids), nq * P, parts, SEGMENT_LIST, SEGMENT_LIST, 0, stream)
    return ids.view(torch.int32).view(nq, P * SEGMENT_LIST, 2)[:, :, 0]  # the low halves; an empty id is 0x7fffffff


def sim_topk_binary_ref(q: torch.Tensor, thr: torch.Tensor, codes: Union[torch.Tensor, BinaryCodes], k: int,
                        id_base: int = 0) -> Tuple[torch.Tensor, torch.Tensor]:
    """PyTorch twin of :func:`sim_topk_binary`."""
    return hamming_scan_topk_ref(binary_pack_ref(q, thr), codes, int(q.shape[1]), k, id_base)


def sim_topk_binary(q: torch.Tensor, thr: torch.Tensor, codes: Union[torch.Tensor, BinaryCodes], k: int,
                    id_base: int = 0, splits: Optional[int] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """``hamming_scan_topk(binary_pack(q, thr), codes, D, k, ...)``: the approximate ``sim_topk`` over sign bits."""
    return hamming_scan_topk(binary_pack(q, thr), codes, int(q.shape[1]), k, id_base, splits)
