"""Residual-compressed token-vector indexes for ``map_maxsim`` (ColBERTv2's stored form).

A token row is the id of its nearest centroid and ``bits`` (1, 2 or 4) per dimension; the value that is scored is
``centroids[cid][d] + weights[code[d]]``, one fp32 add and **no renormalisation**, so a score is the exact
``maxsim_index`` fp32 score of the stored values (``agent_tpu_amd/ops/maxsim.py`` has the byte layout). The
kernel decodes a passage while it loads it into LDS; the decoded rows never exist in device memory.

Five local ``.npy`` files, the companions named after the main file ``<name>.npy``:

* ``<name>.npy`` uint8 ``[T, P * bits / 8]``: the codes (a 2-D **uint8** main file is what selects this loader);
* ``<name>.offsets.npy`` int64 ``[N + 1]``: as in :mod:`runtime.maxsim_index`;
* ``<name>.cids.npy`` int32 ``[T]``; ``<name>.centroids.npy`` fp32 ``[K, P]``; ``<name>.weights.npy`` fp32 ``[2^bits]``.

:func:`compress` trains on the gathered fp32 rows in one process: k-means (``runtime.cluster.kmeans``, cosine,
seed 0), the labels of ``ops.kmeans_assign``, the bucket cutoffs and weights from the quantiles of the residuals
of evenly strided sample rows, then ``ops.residual_encode``. :func:`load_index` is :func:`maxsim_index.load_index`
for this form: a DP rank reads only its slice of codes and ids plus the whole tables, and the slice stays in
``runtime.search``'s LRU under a key of its own kind.
"""
from __future__ import annotations

import os
from typing import Any, Dict, NamedTuple, Tuple

import torch

from . import maxsim_index as mi
from . import search as rs

#: the loader's input errors (``ops/map_maxsim.py`` lists them in ``RESIDUAL_ERRORS``)
ERRORS: Dict[str, str] = {
    "residual_file": "a 2-D uint8 index_uri is a residual index: it needs <name>.cids.npy (1-D int32, one id per "
                     "token row), <name>.centroids.npy (2-D float32 [K, P], K in [1, 4096]) and <name>.weights.npy "
                     "(1-D float32 of 2, 4 or 16 values) next to it, and P * bits / 8 code columns",
    "residual_nonfinite": "residual index centroids or weights hold non-finite values",
    "index_too_large": mi.ERRORS["index_too_large"],
}
BITS = (1, 2, 4)
MAX_CENTROIDS = 4096  # ops.cluster.kmeans_ok's
SAMPLE_ROWS = 8192  # 8192 * 1024 values: under torch.quantile's 16 M input limit at the widest P


class ResidualIndex(NamedTuple):
    codes: torch.Tensor  # [T_r, P * bits / 8] uint8 on the device: the slice's token rows
    cids: torch.Tensor  # [T_r] int32
    centroids: torch.Tensor  # [K, P] fp32 (whole)
    weights: torch.Tensor  # [2^bits] fp32 (whole)
    offsets: torch.Tensor  # [count + 1] int64 on the device, rebased
    start: int
    total: int
    dtype: str  # "residual1", "residual2" or "residual4"
    cached: bool

    @property
    def count(self) -> int:
        return int(self.offsets.numel()) - 1


def companion(path: str, kind: str) -> str:
    return (path[:-len(".npy")] if path.endswith(".npy") else path) + f".{kind}.npy"


def is_residual(uri: Any) -> bool:
    """True when ``uri`` names a local 2-D uint8 ``.npy`` file (anything else goes to the float loader, which
    raises its own errors)."""
    import numpy as np

    try:
        arr = np.load(os.path.realpath(rs.local_path(uri)), mmap_mode="r", allow_pickle=False)
    except (OSError, ValueError, EOFError):
        return False
    return isinstance(arr, np.ndarray) and arr.ndim == 2 and arr.dtype == np.uint8


def compress(x: torch.Tensor, K: int, bits: int, iterations: int) -> Dict[str, Any]:
    """``codes``, ``cids``, ``centroids``, ``weights``, ``cutoffs`` and the k-means ``iterations`` run, for the
    contiguous fp32 rows ``x [T, P]`` (``T >= K``), on ``x``'s device."""
    from .. import ops
    from .cluster import kmeans

    T = int(x.shape[0])
    km = kmeans(x, K, "cosine", seed=0, max_iter=iterations)
    centroids = km.centroids.contiguous()
    cids = ops.kmeans_assign(x, centroids)[0]
    n = min(T, SAMPLE_ROWS)
    rows = (torch.arange(n, dtype=torch.int64) * T // n).to(x.device)  # evenly strided, deterministic
    res = (x[rows] - centroids[cids[rows].long()]).reshape(-1)
    steps = torch.arange(2 ** bits, dtype=torch.float32, device=x.device)
    cutoffs = torch.quantile(res, steps[1:] / 2 ** bits).contiguous()
    weights = torch.quantile(res, (steps + 0.5) / 2 ** bits).contiguous()
    codes = ops.residual_encode(x, cids, centroids, cutoffs)
    return {"codes": codes, "cids": cids, "centroids": centroids, "weights": weights, "cutoffs": cutoffs,
            "iterations": km.iterations}


def write_index(uri: Any, parts: Dict[str, Any], lens: torch.Tensor) -> Dict[str, Any]:
    """Writes :func:`compress`'s result for passages of ``lens [N]`` tokens: each file through a temporary file
    and ``os.replace``, the companions before the main file, so a reader that finds the new codes finds the rest."""
    import numpy as np

    path = rs.local_path(uri)
    codes = parts["codes"].cpu().numpy()
    off = np.zeros(int(lens.numel()) + 1, dtype=np.int64)
    off[1:] = np.cumsum(lens.cpu().numpy().astype(np.int64))
    if int(off[-1]) != int(codes.shape[0]):
        raise ValueError("write_index: lens must sum to the token rows")
    files = [(mi.offsets_path(path), off), (companion(path, "cids"), parts["cids"].cpu().numpy().astype(np.int32)),
             (companion(path, "centroids"), parts["centroids"].cpu().numpy().astype(np.float32)),
             (companion(path, "weights"), parts["weights"].cpu().numpy().astype(np.float32)), (path, codes)]
    for p, a in files:
        mi._write_npy(p, a)
    bits = int(parts["weights"].numel()).bit_length() - 1
    return {"index_uri": path, "offsets_uri": mi.offsets_path(path), "passage_count": int(lens.numel()),
            "token_count": int(codes.shape[0]), "dim": int(parts["centroids"].shape[1]), "dtype": f"residual{bits}",
            "compression": "residual", "centroids": int(parts["centroids"].shape[0]), "bits": bits,
            "kmeans_iterations": int(parts["iterations"]), "bytes": int(sum(os.path.getsize(p) for p, _ in files))}


def open_index(uri: Any):
    """-> (codes, offsets, cids, centroids, weights memmaps, realpath, the five stats); shapes and dtypes checked."""
    import numpy as np

    path = os.path.realpath(rs.local_path(uri))
    try:
        stats = [os.stat(path)]
        arr = np.load(path, mmap_mode="r", allow_pickle=False)
        assert arr.ndim == 2 and arr.dtype == np.uint8 and arr.flags["C_CONTIGUOUS"] and arr.shape[0] and arr.shape[1]
    except (OSError, ValueError, EOFError, AssertionError):
        raise ValueError(ERRORS["residual_file"]) from None
    try:
        opath = mi.offsets_path(path)
        stats.append(os.stat(opath))
        off = np.load(opath, mmap_mode="r", allow_pickle=False)
    except (OSError, ValueError, EOFError):
        raise ValueError(mi.ERRORS["offsets_file"]) from None
    if not isinstance(off, np.ndarray) or off.ndim != 1 or off.dtype.str != "<i8" or off.shape[0] < 2 \
            or int(off[0]) != 0 or int(off[-1]) != int(arr.shape[0]):
        raise ValueError(mi.ERRORS["offsets_file"])
    tables = []
    try:
        for kind in ("cids", "centroids", "weights"):
            stats.append(os.stat(companion(path, kind)))
            tables.append(np.load(companion(path, kind), mmap_mode="r", allow_pickle=False))
    except (OSError, ValueError, EOFError):
        raise ValueError(ERRORS["residual_file"]) from None
    cids, cent, w = tables
    if (cids.ndim != 1 or cids.dtype.str != "<i4" or cids.shape[0] != arr.shape[0]
            or cent.ndim != 2 or cent.dtype.str != "<f4" or not 1 <= cent.shape[0] <= MAX_CENTROIDS
            or w.ndim != 1 or w.dtype.str != "<f4" or w.shape[0] not in (2, 4, 16)
            or int(arr.shape[1]) * 8 != int(cent.shape[1]) * (int(w.shape[0]).bit_length() - 1)):
        raise ValueError(ERRORS["residual_file"])
    return arr, off, cids, cent, w, path, stats


def index_shape(uri: Any) -> Tuple[int, int, int, str]:
    """``(passages, tokens, width, dtype)`` of the files."""
    arr, off, _, cent, w, _, _ = open_index(uri)
    return int(off.shape[0]) - 1, int(arr.shape[0]), int(cent.shape[1]), f"residual{int(w.shape[0]).bit_length() - 1}"


def load_index(uri: Any, start: int = 0, count: int = -1, device: torch.device = torch.device("cpu")) -> ResidualIndex:
    """Passages ``[start, start + count)`` (``count < 0``: to the end) of the index on ``device``."""
    import numpy as np

    arr, off, cids, cent, w, path, stats = open_index(uri)
    total = int(off.shape[0]) - 1
    dtype = f"residual{int(w.shape[0]).bit_length() - 1}"
    start = max(0, min(int(start), total))
    count = total - start if count < 0 else max(0, min(int(count), total - start))
    key = (path,) + tuple(v for st in stats for v in (st.st_mtime_ns, st.st_size)) + (start, count, str(device),
                                                                                     "maxsim_residual")
    with rs._lock:
        hit = rs._cache.get(key)
        if hit is not None:
            rs._cache.move_to_end(key)
            return ResidualIndex(*hit, start, total, dtype, True)
    o = np.array(off[start:start + count + 1], dtype=np.int64, order="C")  # only this slice is read
    if o.size and (bool((np.diff(o) <= 0).any()) or int(o[0]) < 0 or int(o[-1]) > int(arr.shape[0])):
        raise ValueError(mi.ERRORS["offsets_file"])
    r0, r1 = (int(o[0]), int(o[-1])) if count else (0, 0)
    if (r1 - r0) * (int(arr.shape[1]) + 4) + o.size * 8 + cent.size * 4 + w.size * 4 > rs.max_bytes():  # before any allocation
        raise ValueError(ERRORS["index_too_large"])
    tables = [torch.from_numpy(np.array(t, order="C")) for t in (cent, w)]
    if not all(bool(torch.isfinite(t).all()) for t in tables):
        raise ValueError(ERRORS["residual_nonfinite"])
    hit = (torch.from_numpy(np.array(arr[r0:r1], order="C")).to(device), torch.from_numpy(np.array(cids[r0:r1], order="C")).to(device),
           tables[0].to(device), tables[1].to(device), torch.from_numpy(o - r0).to(device).contiguous())
    with rs._lock:
        rs._cache[key] = hit
        rs._cache.move_to_end(key)
        while len(rs._cache) > rs.lru_capacity():
            rs._cache.popitem(last=False)
    return ResidualIndex(*hit, start, total, dtype, False)
