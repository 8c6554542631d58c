"""Lloyd's k-means over device-resident vectors: the loop of ``map_cluster``.

Every iteration is ``ops.kmeans_assign`` (a row's label: fixed-order fp32 arithmetic on the row and the
centroids), ``ops.kmeans_update`` (exact integer sums of the labelled rows), under DP one integer
all-reduce (SUM) of the sums, the counts and the changed count, ``ops.kmeans_finalize`` (single-rounding
fp64 operations on the integer totals) and one small copy back of the changed count. Nothing in it depends
on how the rows are split: by induction over the iterations the labels, sizes, centroids, objective and
iteration count have the same bits for every launch shape and every DP world size.

For the cosine metric the rows of ``x`` are expected normalised (``runtime.search.load_corpus`` and
``normalize_rows`` do that); the centroids are normalised by the finalize step.
"""
from __future__ import annotations

import math
from typing import NamedTuple, Optional

import torch

METRICS = ("cosine", "l2")


class KMeans(NamedTuple):
    labels: torch.Tensor  # [n] int32: this rank's rows, on x's device
    best: torch.Tensor  # [n] fp32: the rows' scores against the centroids they were assigned with
    centroids: torch.Tensor  # [K, D] fp32: the finalize of `labels` (equal on every rank)
    sizes: torch.Tensor  # [K] int64: members over all ranks
    iterations: int
    converged: bool
    changed_last: int
    objective: float  # cosine: sum of best; l2: sum of max(||x||^2 - 2 best, 0); a fixed-point sum
    shift: int  # of the centroid sums


def _all_reduce(t: torch.Tensor, op: str, ws: int) -> torch.Tensor:
    """SUM / MAX over the DP group (in place for a tensor on the communicator's device)."""
    if ws <= 1:
        return t
    import torch.distributed as dist

    from ..parallel import dp, watchdog

    cdev = dp.comm_device(t.device)
    buf = t if t.device == cdev else t.to(cdev)
    buf = buf.contiguous()
    nc = dp.native_comm(cdev)
    with watchdog.collective("cluster all-reduce"):
        if nc is not None:
            nc.all_reduce(buf, op)
            nc.wait("cluster all-reduce")
        else:
            dist.all_reduce(buf, op=dist.ReduceOp.SUM if op == "sum" else dist.ReduceOp.MAX, group=dp.group())
    return buf if buf.device == t.device else buf.to(t.device)


def _absmax(v: torch.Tensor, ws: int) -> float:
    a = v.abs().max().reshape(1) if v.numel() else torch.zeros((1,), dtype=torch.float32, device=v.device)
    return float(_all_reduce(a.to(torch.float32), "max", ws).item())


def _row_sumsq(x: torch.Tensor) -> torch.Tensor:
    """fp32 ``||x[i]||^2``, one column at a time: a row's value does not depend on the batch it is in."""
    out = torch.zeros((x.shape[0],), dtype=torch.float32, device=x.device)
    for d in range(x.shape[1]):
        out += x[:, d] * x[:, d]
    return out


def initial_centroids(x: torch.Tensor, K: int, seed: int, start: int, total: int, ws: int) -> torch.Tensor:
    """Rows ``sorted(randperm(total, seed)[:K])`` of the whole input. Every rank derives the same ids; the owner of
    a row contributes its bit pattern and the others zero bits to an integer all-reduce, so the centroids
    are exact and do not depend on the world size."""
    gen = torch.Generator().manual_seed(int(seed))
    ids = torch.randperm(total, generator=gen)[:K].sort().values
    mine = (ids >= start) & (ids < start + x.shape[0])
    bits = torch.zeros((K, x.shape[1]), dtype=torch.int32, device=x.device)
    if bool(mine.any()):
        bits[mine.to(x.device)] = x[(ids[mine] - start).to(x.device)].view(torch.int32)
    return _all_reduce(bits, "sum", ws).view(torch.float32).contiguous()


def kmeans(x: torch.Tensor, K: int, metric: str = "cosine", seed: int = 0, max_iter: int = 25, tol: float = 0.0,
           init: Optional[torch.Tensor] = None, rank: int = 0, ws: int = 1, start: int = 0,
           total: Optional[int] = None) -> KMeans:
    """k-means of the rows ``[start, start + n)`` that this rank holds in the contiguous fp32 ``x [n, D]`` out of
    ``total`` rows over ``ws`` ranks (every rank calls it; ``n`` may be 0). ``init [K, D]`` replaces the seeded
    choice of ``K`` input rows. Stops when no label changed, when ``changed <= tol * total``, or at ``max_iter``."""
    from .. import ops
    from .search import normalize_rows

    if metric not in METRICS:
        raise ValueError("kmeans: metric must be 'cosine' or 'l2'")
    n, D = int(x.shape[0]), int(x.shape[1])
    total = n if total is None else int(total)
    if not 1 <= K <= total:
        raise ValueError("kmeans: K must be in [1, rows]")
    dev = x.device
    shift = ops.fixed_shift(total, _absmax(x, ws))
    if init is not None:
        c = init.to(device=dev, dtype=torch.float32).contiguous()
        if c.shape != (K, D):
            raise ValueError("kmeans: init must be [K, D]")
        c = normalize_rows(c).contiguous() if metric == "cosine" else c
    else:
        c = initial_centroids(x, K, seed, start, total, ws)
    zs, zc = torch.zeros((K, D), dtype=torch.int64, device=dev), torch.zeros((K,), dtype=torch.int64, device=dev)
    c, bias = ops.kmeans_finalize(zs, zc, c, shift, metric)  # no members: c as it is, and its bias for l2
    labels = torch.full((n,), -1, dtype=torch.int32, device=dev)
    best = torch.zeros((n,), dtype=torch.float32, device=dev)
    none = torch.zeros((1,), dtype=torch.int64, device=dev)
    it, changed, converged, counts = 0, total, False, zc
    while it < max_iter:
        it += 1
        if n:
            labels, best, ch = ops.kmeans_assign(x, c, bias, labels)
            sums, counts = ops.kmeans_update(x, labels, K, shift)
        else:
            sums, counts, ch = zs, zc, none
        if ws > 1:
            buf = _all_reduce(torch.cat([sums.reshape(-1), counts, ch]), "sum", ws)
            sums, counts, ch = buf[:K * D].view(K, D), buf[K * D:K * D + K], buf[K * D + K:]
        c, bias = ops.kmeans_finalize(sums.contiguous(), counts.contiguous(), c, shift, metric)
        changed = int(ch.item())  # the iteration's one copy back
        if changed == 0 or changed <= tol * total:
            converged = True
            break
    vals = best if metric == "cosine" else (_row_sumsq(x) - 2.0 * best).clamp_min(0.0)
    vals = vals.contiguous()
    oshift = ops.fixed_shift(total, _absmax(vals, ws))
    osum = int(_all_reduce(ops.fixed_sum(vals, oshift), "sum", ws).item())
    return KMeans(labels, best, c, counts.clone(), it, converged, changed, math.ldexp(float(osum), -oshift), shift)
