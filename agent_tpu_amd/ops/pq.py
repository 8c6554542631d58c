"""Product quantization (PQ): rows stored as ``M`` bytes and scored by asymmetric distance computation (ADC).

A row of ``D`` floats is cut into ``M`` sub-vectors of ``dsub = D / M`` columns; byte ``m`` of its code is the
nearest of the 256 codewords ``codebooks[m]`` of sub-space ``m`` (``csrc/kernels/pq.hip``):

    codes[i, m]  = arg-max_j  dot(x[i, m*dsub : (m+1)*dsub], codebooks[m, j]) + bias[m, j]       (pq_encode)
    lut[i, m, j] = dot(q[i, m*dsub : (m+1)*dsub], codebooks[m, j])                               (pq_lut)
    score(i, r)  = lut[i, 0, codes[r, 0]] + lut[i, 1, codes[r, 1]] + ... + lut[i, M-1, codes[r, M-1]]   (pq_scan_topk)

``bias = -0.5 ||codeword||^2`` (:func:`pq_bias`) makes the arg-max the nearest codeword. Ties go to the lower
codeword (``+0.0`` and ``-0.0`` tie), and the scan returns the project's total order (score descending, id
ascending: ``better()`` of ``atpu/topk.h``) through ``sim_topk``'s workspace and merge.

The arithmetic is fixed: a sub-space dot product is the fp32 chain ``p_0, + p_1, ..., + p_{dsub-1}`` of separately
rounded products (no FMA), and a score is the fp32 chain of its ``M`` table entries in ascending ``m``, starting at
the first entry. A value depends on its own operands only, so the codes, the tables and the result have the same
bits for every batch, every ``splits`` value and every way the rows are cut into slices; the ``_ref`` twins do the
same operations one column at a time in PyTorch, give the same bits, and are the CPU path.

The score approximates ``dot(q, x)``: it is ``dot(q, decode(codes)[r])`` in another association.

``codes`` is ``[N, M]`` uint8, row-major. The scan kernel reads an interleaved copy (:func:`pq_interleave`,
:class:`PqCodes`): blocks of 64 rows, inside a block the four bytes of sub-spaces ``4 m4 .. 4 m4 + 3`` of the 64
rows side by side, so that a wave's load is one contiguous 256 bytes. :func:`pq_scan_topk` takes either; an index
converts once when it is built.
"""
from __future__ import annotations

from typing import NamedTuple, Optional, Tuple, Union

import torch

from .._native import native, ptr, launch_stream
from ._util import check, same_device
from .search import MAX_K, MAX_ROWS, MAX_SPLITS

CODEWORDS = 256
MAX_SUBVECTORS = 128  # kPqMaxSubvectors: the table of one query is M KiB of LDS
BLOCK_ROWS = 64  # kPqBlock: rows of one interleaved block


def pq_ok(D: int, M: int) -> bool:
    """Shapes the kernels take: ``dsub = D / M`` of 4, 8 or 16 and ``M`` a multiple of 4 from 4 to 128."""
    return (isinstance(D, int) and isinstance(M, int) and 4 <= M <= MAX_SUBVECTORS and M % 4 == 0 and D % M == 0
            and D // M in (4, 8, 16))


class PqCodes(NamedTuple):
    """The scan kernel's private layout of ``rows`` codes of ``M`` bytes."""
    data: torch.Tensor  # uint8 [ceil(rows / 64), M / 4, 64, 4]: byte e of (b, m4, lane) = codes[64 b + lane, 4 m4 + e]
    rows: int
    M: int


def pq_interleave(codes: torch.Tensor) -> PqCodes:
    """:class:`PqCodes` of row-major ``codes [N, M]`` (a copy; the rows past ``N`` of the last block are zero)."""
    check(isinstance(codes, torch.Tensor) and codes.dim() == 2 and codes.dtype == torch.uint8
          and codes.shape[1] % 4 == 0 and codes.shape[1] >= 4, "pq_interleave: codes must be uint8 [N, M], M % 4 == 0")
    N, M = codes.shape
    nb = (N + BLOCK_ROWS - 1) // BLOCK_ROWS
    full = codes if N == nb * BLOCK_ROWS else torch.cat(
        [codes, torch.zeros((nb * BLOCK_ROWS - N, M), dtype=torch.uint8, device=codes.device)])
    return PqCodes(full.view(nb, BLOCK_ROWS, M // 4, 4).permute(0, 2, 1, 3).contiguous(), int(N), int(M))


def pq_deinterleave(pc: PqCodes) -> torch.Tensor:
    """Row-major ``[rows, M]`` of a :class:`PqCodes` (a copy)."""
    nb = pc.data.shape[0]
    return pc.data.permute(0, 2, 1, 3).reshape(nb * BLOCK_ROWS, pc.M)[:pc.rows].contiguous()


def _check_books(codebooks: torch.Tensor, D: int, what: str) -> Tuple[int, int]:
    check(isinstance(codebooks, torch.Tensor) and codebooks.dim() == 3 and codebooks.dtype == torch.float32
          and codebooks.shape[1] == CODEWORDS and codebooks.is_contiguous(),
          f"{what}: codebooks must be a contiguous fp32 [M, 256, dsub]")
    M, _, dsub = codebooks.shape
    check(M * dsub == D and pq_ok(D, M), f"{what}: unsupported shape D={D} M={M}")
    return M, dsub


def _sub_dots(x: torch.Tensor, codebooks: torch.Tensor) -> torch.Tensor:
    """``[n, M, 256]``: every sub-vector against every codeword of its sub-space, one column at a time (each
    product and each add an op of its own: one rounding each, as the kernels)."""
    M, _, dsub = codebooks.shape
    xs = x.view(x.shape[0], M, dsub)
    acc = xs[:, :, None, 0] * codebooks[None, :, :, 0]
    for d in range(1, dsub):
        acc = acc + xs[:, :, None, d] * codebooks[None, :, :, d]
    return acc


def pq_bias(codebooks: torch.Tensor) -> torch.Tensor:
    """fp32 ``[M, 256]``: ``-0.5 ||codeword||^2``, summed in fp64 in ascending column order and rounded once."""
    c = codebooks.double()
    acc = c[:, :, 0] * c[:, :, 0]
    for d in range(1, c.shape[2]):
        acc = acc + c[:, :, d] * c[:, :, d]
    return (acc * -0.5).to(torch.float32).contiguous()


def _check_encode(x, codebooks, bias):
    check(isinstance(x, torch.Tensor) and x.dim() == 2 and x.dtype == torch.float32 and x.is_contiguous(),
          "pq_encode: x must be a contiguous fp32 [n, D]")
    M, _ = _check_books(codebooks, x.shape[1], "pq_encode")
    check(isinstance(bias, torch.Tensor) and bias.dtype == torch.float32 and bias.shape == (M, CODEWORDS)
          and bias.is_contiguous(), "pq_encode: bias must be a contiguous fp32 [M, 256]")
    check(x.shape[0] <= MAX_ROWS, "pq_encode: n must be at most 2^31 - 256")
    same_device(x, codebooks, bias)
    return M


def pq_encode_ref(x: torch.Tensor, codebooks: torch.Tensor, bias: torch.Tensor) -> torch.Tensor:
    """PyTorch twin of :func:`pq_encode` and the CPU path (in row chunks: the ``[n, M, 256]`` scores of a chunk)."""
    M = _check_encode(x, codebooks, bias)
    n = x.shape[0]
    out = torch.empty((n, M), dtype=torch.uint8, device=x.device)
    ids = torch.arange(CODEWORDS, device=x.device)
    rows = max(1, (1 << 22) // (M * CODEWORDS))
    for lo in range(0, n, rows):
        s = _sub_dots(x[lo:lo + rows], codebooks) + bias[None]
        best = s.max(dim=2, keepdim=True).values  # -0.0 == +0.0: they tie
        out[lo:lo + rows] = torch.where(s == best, ids, CODEWORDS).min(dim=2).values.to(torch.uint8)
    return out


def pq_encode(x: torch.Tensor, codebooks: torch.Tensor, bias: torch.Tensor) -> torch.Tensor:
    """uint8 ``[n, M]``: per (row, sub-space) the codeword with the largest ``dot + bias``, ties to the lower id."""
    M = _check_encode(x, codebooks, bias)
    if not x.is_cuda or x.shape[0] == 0:
        return pq_encode_ref(x, codebooks, bias)
    codes = torch.empty((x.shape[0], M), dtype=torch.uint8, device=x.device)
    native().pq_encode(ptr(x), ptr(codebooks), ptr(bias), ptr(codes), x.shape[0], x.shape[1], M, launch_stream(x))
    return codes


def _check_lut_in(q, codebooks):
    check(isinstance(q, torch.Tensor) and q.dim() == 2 and q.dtype == torch.float32 and q.is_contiguous(),
          "pq_lut: q must be a contiguous fp32 [nq, D]")
    M, _ = _check_books(codebooks, q.shape[1], "pq_lut")
    same_device(q, codebooks)
    return M


def pq_lut_ref(q: torch.Tensor, codebooks: torch.Tensor) -> torch.Tensor:
    """PyTorch twin of :func:`pq_lut` and the CPU path."""
    _check_lut_in(q, codebooks)
    return _sub_dots(q, codebooks).contiguous()


def pq_lut(q: torch.Tensor, codebooks: torch.Tensor) -> torch.Tensor:
    """fp32 ``[nq, M, 256]``: the ADC tables of the queries."""
    M = _check_lut_in(q, codebooks)
    if not q.is_cuda or q.shape[0] == 0:
        return pq_lut_ref(q, codebooks)
    lut = torch.empty((q.shape[0], M, CODEWORDS), dtype=torch.float32, device=q.device)
    native().pq_lut(ptr(q), ptr(codebooks), ptr(lut), q.shape[0], q.shape[1], M, launch_stream(q))
    return lut


def decode(codes: torch.Tensor, codebooks: torch.Tensor) -> torch.Tensor:
    """fp32 ``[N, D]``: the reconstruction of every row, its codewords side by side."""
    check(codes.dim() == 2 and codes.dtype == torch.uint8 and codebooks.dim() == 3
          and codes.shape[1] == codebooks.shape[0], "decode: codes uint8 [N, M] and codebooks [M, 256, dsub]")
    M, _, dsub = codebooks.shape
    m = torch.arange(M, device=codes.device)
    return codebooks[m[None, :], codes.long()].reshape(codes.shape[0], M * dsub)


def _check_scan(lut, codes, k, id_base, splits):
    check(isinstance(lut, torch.Tensor) and lut.dim() == 3 and lut.dtype == torch.float32 and lut.shape[2] == CODEWORDS
          and lut.is_contiguous(), "pq_scan_topk: lut must be a contiguous fp32 [nq, M, 256]")
    M = lut.shape[1]
    check(4 <= M <= MAX_SUBVECTORS and M % 4 == 0, "pq_scan_topk: M must be a multiple of 4 in [4, 128]")
    if isinstance(codes, PqCodes):
        N = codes.rows
        check(isinstance(N, int) and codes.M == M and codes.data.dtype == torch.uint8 and codes.data.is_contiguous()
              and codes.data.shape == ((N + BLOCK_ROWS - 1) // BLOCK_ROWS, M // 4, BLOCK_ROWS, 4),
              "pq_scan_topk: PqCodes must be a contiguous uint8 [ceil(rows / 64), M / 4, 64, 4] of the lut's M")
        same_device(lut, codes.data)
    else:
        check(isinstance(codes, torch.Tensor) and codes.dim() == 2 and codes.dtype == torch.uint8
              and codes.shape[1] == M and codes.is_contiguous(),
              "pq_scan_topk: codes must be a contiguous uint8 [N, M] of the lut's M (or a PqCodes)")
        N = codes.shape[0]
        same_device(lut, codes)
    check(isinstance(k, int) and not isinstance(k, bool) and 1 <= k <= MAX_K, "pq_scan_topk: k must be in [1, 32]")
    check(1 <= N <= MAX_ROWS, "pq_scan_topk: N must be in [1, 2^31 - 256]")
    check(isinstance(id_base, int) and 0 <= id_base < 2 ** 61, "pq_scan_topk: id_base must be in [0, 2^61)")
    check(splits is None or (isinstance(splits, int) and 1 <= splits <= MAX_SPLITS),
          f"pq_scan_topk: splits must be in [1, {MAX_SPLITS}]")
    return N, M


def pq_scan_topk_ref(lut: torch.Tensor, codes: Union[torch.Tensor, PqCodes], k: int, id_base: int = 0
                     ) -> Tuple[torch.Tensor, torch.Tensor]:
    """PyTorch twin of :func:`pq_scan_topk` and the CPU path: the ``[nq, N]`` scores one sub-space at a time, then
    the two stable sorts of ``sim_topk_ref``."""
    N, M = _check_scan(lut, codes, k, id_base, None)
    rows = (pq_deinterleave(codes) if isinstance(codes, PqCodes) else codes).long()
    s = lut[:, 0, rows[:, 0]]
    for m in range(1, M):
        s = s + lut[:, m, rows[:, m]]
    kk = min(k, N)
    order = torch.sort(s + 0.0, dim=1, descending=True, stable=True).indices[:, :kk]  # -0.0 + 0.0 = +0.0: they tie
    return torch.gather(s, 1, order), order.to(torch.int64) + int(id_base)


def pq_auto_splits(N: int, device: torch.device) -> int:
    """One workgroup per split (it loops over the queries): a split per CU, but no split under 2048 rows (one step
    of the workgroup's 8 waves x 4 blocks)."""
    cus = torch.cuda.get_device_properties(device).multi_processor_count
    return max(1, min(MAX_SPLITS, cus, (N + 2047) // 2048))


def pq_scan_topk(lut: torch.Tensor, codes: Union[torch.Tensor, PqCodes], k: int, id_base: int = 0,
                 splits: Optional[int] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """(scores ``[nq, kk]`` fp32, ids ``[nq, kk]`` int64), ``kk = min(k, N)``: the rows with the largest ADC score
    of every query's table, ordered by (score desc, id asc), ``ids = id_base + row``. ``codes``: row-major uint8
    ``[N, M]`` (interleaved here, on every call) or a :class:`PqCodes`. The result does not depend on ``splits``
    (tests and benches) or on the batch."""
    N, M = _check_scan(lut, codes, k, id_base, splits)
    nq = lut.shape[0]
    kk = min(k, N)
    if nq == 0:
        return (torch.empty((0, kk), dtype=torch.float32, device=lut.device),
                torch.empty((0, kk), dtype=torch.int64, device=lut.device))
    if not lut.is_cuda:
        return pq_scan_topk_ref(lut, codes, k, id_base)
    pc = codes if isinstance(codes, PqCodes) else pq_interleave(codes)
    nat = native()
    P = nat.pq_scan_splits(N, splits if splits is not None else pq_auto_splits(N, lut.device))
    ws = torch.empty((nq, P, k, 2), dtype=torch.float32, device=lut.device)
    scores = torch.empty((nq, kk), dtype=torch.float32, device=lut.device)
    ids = torch.empty((nq, kk), dtype=torch.int64, device=lut.device)
    stream = launch_stream(lut)
    nat.pq_scan_partial(ptr(lut), ptr(pc.data), ptr(ws), nq, N, M, k, P, stream)
    nat.sim_topk_merge(ptr(ws), ptr(scores), ptr(ids), nq, P, k, kk, int(id_base), stream)
    return scores, ids


def sim_topk_pq_ref(q: torch.Tensor, codebooks: torch.Tensor, codes: Union[torch.Tensor, PqCodes], k: int,
                    id_base: int = 0) -> Tuple[torch.Tensor, torch.Tensor]:
    """PyTorch twin of :func:`sim_topk_pq`."""
    return pq_scan_topk_ref(pq_lut_ref(q, codebooks), codes, k, id_base)


def sim_topk_pq(q: torch.Tensor, codebooks: torch.Tensor, codes: Union[torch.Tensor, PqCodes], k: int,
                id_base: int = 0, splits: Optional[int] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """``pq_scan_topk(pq_lut(q, codebooks), codes, k, ...)``: the approximate ``sim_topk`` over compressed rows."""
    return pq_scan_topk(pq_lut(q, codebooks), codes, k, id_base, splits)
