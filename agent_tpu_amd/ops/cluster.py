"""k-means building blocks: the assignment step, order-free fixed-point sums, the centroid update and finalize.

``kmeans_assign`` (``csrc/kernels/kmeans.hip``) gives every row of ``x [N, D]`` the centroid of ``c [K, D]``
with the largest ``score(i, k) = dot(x[i], c[k]) (+ bias[k])`` in the project's total order (score descending,
centroid id ascending, ``+0.0`` and ``-0.0`` tie: ``better()`` of ``atpu/topk.h``). A score is ONE fp32
accumulator on the exact f32 MFMA fed in ``sim_topk``'s column order (a function of ``D`` alone) and the bias
is one fp32 add afterwards, so a row's ``(label, best)`` has the same bits whatever the launch shape, ``N``,
``K``'s tiling or the row's position, and without a bias it equals ``sim_topk(x, c, 1)`` bit for bit. For the
Euclidean metric ``bias[k] = -0.5 ||c[k]||^2`` makes the arg-max the nearest centroid.

Order-free sums (``fixed_sum``, ``kmeans_update``): a value ``v`` enters a sum as the int64
``rint(v * 2^s)`` (ties to even). The product is exact (a power-of-two scale), integer addition is
associative, so a total has the same bits in any order, chunking or rank split. :func:`fixed_shift` picks
``s`` from the global row count and the global absolute maximum only, so that no total can exceed ``2^62``.

``kmeans_finalize`` turns the integer sums into centroids with single correctly rounded fp64 operations in
ascending column order; the PyTorch twin does the same operations and gives the same bits.

Every ``_ref`` twin is also the CPU path. The twins trade speed for a fixed arithmetic order
(``kmeans_assign_ref`` adds one column at a time, so a row's score does not depend on the batch it is in).
"""
from __future__ import annotations

import math
from typing import Optional, Tuple

import torch

from .._native import native, ptr, launch_stream
from ._util import check, same_device

MAX_K = 4096  # kKmeansMaxK
MAX_ROWS = 2 ** 31 - 256
EPS = 1e-12
METRICS = ("cosine", "l2")


def kmeans_ok(D: int, K: int) -> bool:
    """Shapes the kernels take: D as ``sim_topk_ok`` (a multiple of 64 from 64 to 1024), K in 1..4096."""
    return D % 64 == 0 and 64 <= D <= 1024 and 1 <= K <= MAX_K


# ------------------------------------------------------------------------------------------ fixed-point sums
def fixed_shift(n_total: int, absmax: float) -> int:
    """``s = 62 - ceil(log2(max(n_total, 2))) - E`` with ``E`` the smallest integer such that
    ``absmax <= 2^E`` (``absmax == 0``: ``E = 0``; every sum is zero whatever the shift)."""
    check(isinstance(n_total, int) and not isinstance(n_total, bool) and n_total >= 1, "fixed_shift: n_total must be >= 1")
    absmax = float(absmax)
    check(math.isfinite(absmax) and absmax >= 0.0, "fixed_shift: absmax must be finite and >= 0")
    bits = (max(n_total, 2) - 1).bit_length()  # ceil(log2)
    if absmax == 0.0:
        return 62 - bits
    m, e = math.frexp(absmax)  # absmax = m * 2^e, 0.5 <= m < 1
    return 62 - bits - (e - 1 if m == 0.5 else e)


def to_fixed(v: torch.Tensor, s: int) -> torch.Tensor:
    """``rint(v * 2^s)`` as int64 (ties to even; the fp64 product of an fp32 value and a power of two is exact)."""
    return (v.double() * (2.0 ** s)).round().to(torch.int64)


def fixed_sum_ref(v: torch.Tensor, s: int) -> torch.Tensor:
    return to_fixed(v.reshape(-1), s).sum().reshape(1)


def fixed_sum(v: torch.Tensor, s: int) -> torch.Tensor:
    """int64 ``[1]``: the order-free sum of the fp32 values ``v``."""
    check(v.dtype == torch.float32 and v.is_contiguous(), "fixed_sum: v must be a contiguous fp32 tensor")
    check(isinstance(s, int) and -1000 <= s <= 1000, "fixed_sum: s must be an int in [-1000, 1000]")
    if not v.is_cuda:
        return fixed_sum_ref(v, s)
    out = torch.empty((1,), dtype=torch.int64, device=v.device)
    native().fixed_sum(ptr(v), v.numel(), s, ptr(out), launch_stream(v))
    return out


# ------------------------------------------------------------------------------------------------- assign
def _check_assign(x, c, bias, prev_labels) -> None:
    check(x.dim() == 2 and c.dim() == 2 and x.shape[1] == c.shape[1], "kmeans_assign: x [N, D] and c [K, D]")
    check(x.dtype == torch.float32 and c.dtype == torch.float32, "kmeans_assign: x and c must be fp32")
    check(x.is_contiguous() and c.is_contiguous(), "kmeans_assign: contiguous tensors")
    N, K = x.shape[0], c.shape[0]
    check(1 <= N <= MAX_ROWS, "kmeans_assign: N must be in [1, 2^31 - 256]")
    check(bias is None or (bias.dtype == torch.float32 and bias.shape == (K,) and bias.is_contiguous()),
          "kmeans_assign: bias must be a contiguous fp32 [K]")
    check(prev_labels is None or (prev_labels.dtype == torch.int32 and prev_labels.shape == (N,)
                                  and prev_labels.is_contiguous()),
          "kmeans_assign: prev_labels must be a contiguous int32 [N]")
    same_device(x, c, bias, prev_labels)


def kmeans_assign_ref(x: torch.Tensor, c: torch.Tensor, bias: Optional[torch.Tensor] = None,
                      prev_labels: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """PyTorch twin and CPU path: fp32 scores accumulated one column at a time (one rounding per product and
    per add, the same order for every row and batch), the arg-max in the (score desc, id asc) order."""
    _check_assign(x, c, bias, prev_labels)
    N, D = x.shape
    K = c.shape[0]
    check(1 <= K <= MAX_K, f"kmeans_assign: unsupported shape D={D} K={K}")
    ct = c.T.contiguous()
    s = torch.zeros((N, K), dtype=torch.float32, device=x.device)
    for d in range(D):
        s += x[:, d:d + 1] * ct[d]
    if bias is not None:
        s = s + bias
    top = s.max(dim=1, keepdim=True).values
    ids = torch.arange(K, device=x.device).expand(N, K)
    labels = torch.where(s == top, ids, K).min(dim=1).values  # the lowest id among the maxima (+0.0 == -0.0)
    best = torch.gather(s, 1, labels[:, None])[:, 0]
    labels = labels.to(torch.int32)
    prev = prev_labels if prev_labels is not None else torch.full((N,), -1, dtype=torch.int32, device=x.device)
    changed = (labels != prev).sum().to(torch.int64).reshape(1)
    return labels, best, changed


def kmeans_assign(x: torch.Tensor, c: torch.Tensor, bias: Optional[torch.Tensor] = None,
                  prev_labels: Optional[torch.Tensor] = None, max_wgs: int = 0
                  ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """(labels ``[N]`` int32, best ``[N]`` fp32, changed ``[1]`` int64) of the contiguous fp32 ``x [N, D]``
    against ``c [K, D]``; ``prev_labels=None`` counts every row as changed. ``max_wgs`` caps the persistent
    grid (0: the device's own) and exists for tests: the result does not depend on it."""
    _check_assign(x, c, bias, prev_labels)
    N, D = x.shape
    K = c.shape[0]
    check(kmeans_ok(D, K), f"kmeans_assign: unsupported shape D={D} K={K}")
    check(isinstance(max_wgs, int) and max_wgs >= 0, "kmeans_assign: max_wgs must be an int >= 0")
    if not x.is_cuda:
        return kmeans_assign_ref(x, c, bias, prev_labels)
    if prev_labels is None:
        prev_labels = torch.full((N,), -1, dtype=torch.int32, device=x.device)
    labels = torch.empty((N,), dtype=torch.int32, device=x.device)
    best = torch.empty((N,), dtype=torch.float32, device=x.device)
    changed = torch.empty((1,), dtype=torch.int64, device=x.device)
    native().kmeans_assign(ptr(x), ptr(c), ptr(bias), ptr(prev_labels), ptr(labels), ptr(best), ptr(changed), N, K, D,
                           max_wgs, launch_stream(x))
    return labels, best, changed


# ------------------------------------------------------------------------------------------------- update
def _check_update(x, labels, K, s) -> None:
    check(x.dim() == 2 and x.dtype == torch.float32 and x.is_contiguous(), "kmeans_update: x must be a contiguous fp32 [N, D]")
    check(labels.dtype == torch.int32 and labels.shape == (x.shape[0],) and labels.is_contiguous(),
          "kmeans_update: labels must be a contiguous int32 [N]")
    check(isinstance(K, int) and 1 <= K <= MAX_K, "kmeans_update: K must be in [1, 4096]")
    check(isinstance(s, int) and -1000 <= s <= 1000, "kmeans_update: s must be an int in [-1000, 1000]")
    same_device(x, labels)


def kmeans_update_ref(x: torch.Tensor, labels: torch.Tensor, K: int, s: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """int64 twin and CPU path: ``index_add_`` of the fixed-point rows (a label outside ``[0, K)`` leaves its
    row out, as the kernel does)."""
    _check_update(x, labels, K, s)
    lab = labels.to(torch.int64)
    keep = (lab >= 0) & (lab < K)
    if not bool(keep.all()):
        x, lab = x[keep], lab[keep]
    sums = torch.zeros((K, x.shape[1]), dtype=torch.int64, device=x.device).index_add_(0, lab, to_fixed(x, s))
    counts = torch.zeros((K,), dtype=torch.int64, device=x.device).index_add_(0, lab, torch.ones_like(lab))
    return sums, counts


def kmeans_update(x: torch.Tensor, labels: torch.Tensor, K: int, s: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """(sums ``[K, D]`` int64, counts ``[K]`` int64): per label, the order-free sums of its rows of ``x`` at
    shift ``s`` and its member count. An empty ``x`` gives zeros."""
    _check_update(x, labels, K, s)
    N, D = x.shape
    if not x.is_cuda or N == 0:
        return kmeans_update_ref(x, labels, K, s)
    check(kmeans_ok(D, K), f"kmeans_update: unsupported shape D={D} K={K}")
    check(N <= MAX_ROWS, "kmeans_update: N must be in [1, 2^31 - 256]")
    nat = native()
    sums = torch.empty((K, D), dtype=torch.int64, device=x.device)
    counts = torch.empty((K,), dtype=torch.int64, device=x.device)
    ws = torch.empty((nat.kmeans_update_ws_bytes(N, K) // 4,), dtype=torch.int32, device=x.device)
    nat.kmeans_update(ptr(x), ptr(labels), s, ptr(sums), ptr(counts), ptr(ws), N, K, D, launch_stream(x))
    return sums, counts


# ----------------------------------------------------------------------------------------------- finalize
def _check_finalize(sums, counts, c_old, s, metric) -> None:
    check(c_old.dim() == 2 and c_old.dtype == torch.float32 and c_old.is_contiguous(),
          "kmeans_finalize: c_old must be a contiguous fp32 [K, D]")
    K, D = c_old.shape
    check(sums.dtype == torch.int64 and sums.shape == (K, D) and sums.is_contiguous()
          and counts.dtype == torch.int64 and counts.shape == (K,) and counts.is_contiguous(),
          "kmeans_finalize: sums must be int64 [K, D] and counts int64 [K], contiguous")
    check(1 <= K <= MAX_K and D >= 1, "kmeans_finalize: K must be in [1, 4096]")
    check(isinstance(s, int) and -1000 <= s <= 1000, "kmeans_finalize: s must be an int in [-1000, 1000]")
    check(metric in METRICS, "kmeans_finalize: metric must be 'cosine' or 'l2'")
    same_device(sums, counts, c_old)


def _sumsq64(m: torch.Tensor) -> torch.Tensor:
    """fp64 ``sum_d m[:, d]^2``, columns in ascending order, one rounding per product and per add."""
    ss = torch.zeros((m.shape[0],), dtype=torch.float64, device=m.device)
    md = m.double()
    for d in range(m.shape[1]):
        ss = ss + md[:, d] * md[:, d]
    return ss


def kmeans_finalize_ref(sums: torch.Tensor, counts: torch.Tensor, c_old: torch.Tensor, s: int, metric: str
                        ) -> Tuple[torch.Tensor, Optional[torch.Tensor]]:
    """fp64 twin and CPU path: every step is one correctly rounded IEEE operation, as in the kernel."""
    _check_finalize(sums, counts, c_old, s, metric)
    live = counts > 0
    den = torch.where(live, counts.double() * (2.0 ** s), torch.ones((), dtype=torch.float64, device=counts.device))
    mean = (sums.double() / den[:, None]).to(torch.float32)
    if metric == "cosine":
        nrm = _sumsq64(mean).sqrt().clamp_min(EPS)
        mean = (mean.double() / nrm[:, None]).to(torch.float32)
    c_new = torch.where(live[:, None], mean, c_old).contiguous()
    bias = (-0.5 * _sumsq64(c_new)).to(torch.float32) if metric == "l2" else None
    return c_new, bias


def kmeans_finalize(sums: torch.Tensor, counts: torch.Tensor, c_old: torch.Tensor, s: int, metric: str
                    ) -> Tuple[torch.Tensor, Optional[torch.Tensor]]:
    """(c_new ``[K, D]`` fp32, bias ``[K]`` fp32 for ``l2`` else None): the mean
    ``float(double(sum) / (double(count) * 2^s))`` of every non-empty cluster, divided by
    ``max(its fp64 norm, 1e-12)`` for ``cosine``; an empty cluster keeps its old centroid."""
    _check_finalize(sums, counts, c_old, s, metric)
    if not c_old.is_cuda:
        return kmeans_finalize_ref(sums, counts, c_old, s, metric)
    K, D = c_old.shape
    c_new = torch.empty_like(c_old)
    bias = torch.empty((K,), dtype=torch.float32, device=c_old.device) if metric == "l2" else None
    native().kmeans_finalize(ptr(sums), ptr(counts), ptr(c_old), ptr(c_new), ptr(bias), K, D, s,
                             1 if metric == "cosine" else 0, launch_stream(c_old))
    return c_new, bias
