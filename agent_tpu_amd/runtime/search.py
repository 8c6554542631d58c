"""Device-resident corpora for ``map_search`` and the search over them.

A corpus is a 2-D C-order ``.npy`` of ``float32`` or ``float16`` rows: exactly what ``map_embed``
writes with ``output: "npy"``. :func:`load_corpus` memory-maps it, so a DP rank touches only its
``[start, start + count)`` slice, widens ``float16`` to fp32 once, normalises the rows on the
device for the cosine metric (one-time work per index, not the hot path), refuses non-finite
values, and keeps the loaded slices in a small LRU keyed by the file's identity (a rewritten file
misses). :func:`search` is ``ops.sim_topk`` on the GPU and its PyTorch twin on a CPU engine.

With ``dtype="float16"`` the resident rows are fp16 (a ``float16`` file as it is, a ``float32`` file
rounded to nearest) at half the bytes, and cosine keeps the rows unnormalised beside an fp32
``row_scale = 1 / max(||row||_2, 1e-12)`` that ``sim_topk`` multiplies into the finished score.

The IVF indexes of ``runtime/ivf.py`` are entries of the same LRU, under the corpus key extended by
``("ivf", clusters, train_iterations)``, and the product-quantized corpora of ``runtime/pq.py`` under
``("pq", subvectors, train_rows, train_iterations, normalised?)``.
"""
from __future__ import annotations

import os
import threading
from collections import OrderedDict
from typing import Any, Dict, NamedTuple, Optional, Tuple

import torch

EPS = 1e-12  # F.normalize's, as pool_embed

#: the loader's input errors (``ops/map_search.py`` lists them in its own ``ERRORS``)
ERRORS: Dict[str, str] = {
    "corpus_file": "corpus_uri must be a local 2-D float32 or float16 .npy file",
    "corpus_empty": "corpus has no rows",
    "corpus_nonfinite": "corpus holds non-finite values",
    "corpus_too_large": "corpus slice exceeds SEARCH_INDEX_MAX_GB of float32",
}
#: those of a ``float16``-resident corpus (``ops/map_search.py``: ``F16_ERRORS``)
F16_ERRORS: Dict[str, str] = {
    "corpus_f16_range": "corpus values exceed the float16 range",
    "corpus_too_large_f16": "corpus slice exceeds SEARCH_INDEX_MAX_GB of float16",
}
#: that of a label file (``ops/map_search.py``: ``FILTER_ERRORS``)
LABEL_ERRORS: Dict[str, str] = {
    "labels_file": "corpus_labels_uri must be a local 1-D int32 or int64 .npy file with one label per corpus row",
}
DTYPES = ("float32", "float16")
CHUNK_BYTES = 64 * 2 ** 20  # fp32 bytes of the row chunks that a float16 load checks and norms


class Corpus(NamedTuple):
    vectors: torch.Tensor  # [count, dim] fp32 or fp16 on the device, contiguous
    start: int  # row of the file that vectors[0] is
    total: int  # rows of the whole file
    cached: bool  # served from the LRU
    scale: Optional[torch.Tensor] = None  # [count] fp32: the cosine row scale of fp16 vectors


_lock = threading.Lock()
_cache: "OrderedDict[Tuple, Tuple[torch.Tensor, Optional[torch.Tensor]]]" = OrderedDict()
_label_cache: "OrderedDict[Tuple, torch.Tensor]" = OrderedDict()  # int64 label slices (load_labels)
_label_stats = {"hits": 0, "loads": 0}


def lru_capacity() -> int:
    return max(1, int(os.getenv("SEARCH_INDEX_LRU_SIZE", "2")))


def max_bytes() -> int:
    return int(float(os.getenv("SEARCH_INDEX_MAX_GB", "64")) * 2 ** 30)


def local_path(uri: Any) -> str:
    if not isinstance(uri, str) or not uri or ("://" in uri and not uri.startswith("file://")):
        raise ValueError(ERRORS["corpus_file"])
    return uri[len("file://"):] if uri.startswith("file://") else uri


def open_corpus(uri: Any):
    """-> (memory-mapped array, realpath, stat); the file's shape and dtype checked, nothing read."""
    import numpy as np

    path = os.path.realpath(local_path(uri))
    try:
        st = os.stat(path)
        arr = np.load(path, mmap_mode="r", allow_pickle=False)
    except (OSError, ValueError, EOFError):
        raise ValueError(ERRORS["corpus_file"]) from None
    if not isinstance(arr, np.ndarray) or arr.ndim != 2 or arr.dtype.str not in ("<f4", "<f2") \
            or not arr.flags["C_CONTIGUOUS"]:
        raise ValueError(ERRORS["corpus_file"])
    if arr.shape[0] == 0 or arr.shape[1] == 0:
        raise ValueError(ERRORS["corpus_empty"])
    return arr, path, st


def corpus_shape(uri: Any) -> Tuple[int, int]:
    arr, _, _ = open_corpus(uri)
    return int(arr.shape[0]), int(arr.shape[1])


def normalize_rows(x: torch.Tensor) -> torch.Tensor:
    return x / x.norm(dim=1, keepdim=True).clamp_min(EPS)


def _load_f16(arr, start: int, count: int, normalize: bool, device: torch.device):
    """-> (fp16 rows ``[count, dim]``, fp32 scale ``[count]`` or None) on ``device``, in row chunks: the
    finiteness and range checks and the norms never hold an fp32 copy of more than one chunk."""
    import numpy as np

    dim = int(arr.shape[1])
    vec = torch.empty((count, dim), dtype=torch.float16, device=device)
    scale = torch.empty((count,), dtype=torch.float32, device=device) if normalize else None
    rows = max(1, CHUNK_BYTES // (dim * 4))
    for lo in range(0, count, rows):
        hi = min(lo + rows, count)
        src = torch.from_numpy(np.array(arr[start + lo:start + hi], order="C")).to(device)  # only these rows are read
        if not bool(torch.isfinite(src).all()):
            raise ValueError(ERRORS["corpus_nonfinite"])
        part = src.to(torch.float16)  # a float32 file: round to nearest; past the range: inf
        if not bool(torch.isfinite(part).all()):
            raise ValueError(F16_ERRORS["corpus_f16_range"])
        vec[lo:hi] = part
        if normalize:  # from the resident values; the sum in fp64, so the fp32 scale carries one rounding
            scale[lo:hi] = part.double().norm(dim=1).clamp_min(EPS).reciprocal().to(torch.float32)
    return vec, scale


def load_corpus(uri: Any, start: int = 0, count: int = -1, normalize: bool = True,
                device: torch.device = torch.device("cpu"), dtype: str = "float32") -> Corpus:
    """Rows ``[start, start + count)`` (``count < 0``: to the end) of the file on ``device``: fp32
    (normalised when ``normalize``), or for ``dtype="float16"`` fp16 as stored plus the fp32 row scale
    that normalises them."""
    import numpy as np

    if dtype not in DTYPES:
        raise ValueError("load_corpus: dtype must be 'float32' or 'float16'")
    arr, path, st = open_corpus(uri)
    total, dim = int(arr.shape[0]), int(arr.shape[1])
    start = max(0, min(int(start), total))
    count = total - start if count < 0 else max(0, min(int(count), total - start))
    key = (path, st.st_mtime_ns, st.st_size, start, count, bool(normalize), str(device), dtype)
    with _lock:
        hit = _cache.get(key)
        if hit is not None:
            _cache.move_to_end(key)
            return Corpus(hit[0], start, total, True, hit[1])
    if dtype == "float16":
        if count * dim * 2 + (count * 4 if normalize else 0) > max_bytes():  # before any allocation
            raise ValueError(F16_ERRORS["corpus_too_large_f16"])
        vec, scale = _load_f16(arr, start, count, bool(normalize), device)
    else:
        if count * dim * 4 > max_bytes():  # before any allocation
            raise ValueError(ERRORS["corpus_too_large"])
        host = torch.from_numpy(np.array(arr[start:start + count], order="C"))  # a copy: only this slice is read
        vec = host.to(device).to(torch.float32)  # float16 is widened once, here
        if not bool(torch.isfinite(vec).all()):
            raise ValueError(ERRORS["corpus_nonfinite"])
        if normalize:
            vec = normalize_rows(vec)
        vec, scale = vec.contiguous(), None
    with _lock:
        _cache[key] = (vec, scale)
        _cache.move_to_end(key)
        while len(_cache) > lru_capacity():
            _cache.popitem(last=False)
    return Corpus(vec, start, total, False, scale)


def load_labels(uri: Any, start: int = 0, count: int = -1, device: torch.device = torch.device("cpu"),
                total: Optional[int] = None) -> torch.Tensor:
    """Labels ``[start, start + count)`` (``count < 0``: to the end) of a 1-D ``int32`` or ``int64``
    ``.npy`` on ``device`` as int64; ``total``: the rows the file must have (one label per corpus
    row). The slices stay in an LRU of their own, with the vector LRU's capacity and key form."""
    import numpy as np

    try:
        path = os.path.realpath(local_path(uri))
        st = os.stat(path)
        arr = np.load(path, mmap_mode="r", allow_pickle=False)
    except (OSError, ValueError, EOFError):
        raise ValueError(LABEL_ERRORS["labels_file"]) from None
    if not isinstance(arr, np.ndarray) or arr.ndim != 1 or arr.dtype.str not in ("<i4", "<i8") \
            or (total is not None and arr.shape[0] != total):
        raise ValueError(LABEL_ERRORS["labels_file"])
    rows = int(arr.shape[0])
    start = max(0, min(int(start), rows))
    count = rows - start if count < 0 else max(0, min(int(count), rows - start))
    key = (path, st.st_mtime_ns, st.st_size, start, count, str(device))
    with _lock:
        hit = _label_cache.get(key)
        if hit is not None:
            _label_cache.move_to_end(key)
            _label_stats["hits"] += 1
            return hit
    lab = torch.from_numpy(np.array(arr[start:start + count], dtype=np.int64, order="C")).to(device).contiguous()
    with _lock:
        _label_stats["loads"] += 1
        _label_cache[key] = lab
        _label_cache.move_to_end(key)
        while len(_label_cache) > lru_capacity():
            _label_cache.popitem(last=False)
    return lab


def clear_cache() -> None:
    with _lock:
        _cache.clear()
        _label_cache.clear()


def cache_info() -> Dict[str, Any]:
    """``entries``, ``capacity`` and ``resident_bytes`` speak of the vectors; the ``label_*`` keys of the
    label LRU."""
    with _lock:
        return {"entries": [k[0] for k in _cache], "capacity": lru_capacity(),
                "resident_bytes": sum(t.numel() * t.element_size() for v in _cache.values() for t in v
                                      if isinstance(t, torch.Tensor)),  # an IVF entry (runtime/ivf.py) ends in two scalars
                "label_entries": [k[0] for k in _label_cache],
                "label_bytes": sum(t.numel() * t.element_size() for t in _label_cache.values()),
                "label_hits": _label_stats["hits"], "label_loads": _label_stats["loads"]}


def search(qvecs: torch.Tensor, corpus: torch.Tensor, k: int, id_base: int = 0,
           row_scale: Optional[torch.Tensor] = None, mask=None) -> Tuple[torch.Tensor, torch.Tensor]:
    """(scores ``[nq, kk]`` fp32, ids ``[nq, kk]`` int64) of the fp32 ``qvecs [nq, dim]`` against
    ``corpus [rows, dim]`` (fp32, or fp16 with its optional ``row_scale [rows]``) on the corpus's
    device, ordered by (score desc, id asc). An empty slice
    (a DP rank beyond the corpus) gives ``kk = 0``. A shape the kernel does not take is an error,
    never a detour through PyTorch. ``mask`` (an ``ops.RowMask`` of the slice, on its device): only
    its rows, ``kk = min(k, mask.count)``."""
    from .. import ops

    q = qvecs.to(device=corpus.device, dtype=torch.float32).contiguous()
    if corpus.shape[0] == 0:
        return (torch.empty((q.shape[0], 0), dtype=torch.float32, device=corpus.device),
                torch.empty((q.shape[0], 0), dtype=torch.int64, device=corpus.device))
    if mask is not None:  # its own calls, so that the unfiltered ones stay as they were
        if not corpus.is_cuda:
            return ops.sim_topk_ref(q, corpus, k, id_base, row_scale=row_scale, mask=mask)
        return ops.sim_topk(q, corpus, k, id_base, row_scale=row_scale, mask=mask)
    if not corpus.is_cuda:
        return ops.sim_topk_ref(q, corpus, k, id_base, row_scale=row_scale)
    return ops.sim_topk(q, corpus, k, id_base, row_scale=row_scale)


def merge_topk(scores: torch.Tensor, ids: torch.Tensor, k: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """The best ``k`` columns of every row of ``scores`` / ``ids [nq, m]`` in the (score desc, id asc)
    order: two stable sorts, the minor key first. Padding is ``(-inf, 2^62)`` and sorts last."""
    by_id = torch.sort(ids, dim=1, stable=True).indices
    s1, i1 = torch.gather(scores, 1, by_id), torch.gather(ids, 1, by_id)
    by_score = torch.sort(s1 + 0.0, dim=1, descending=True, stable=True).indices[:, :k]
    return torch.gather(s1, 1, by_score), torch.gather(i1, 1, by_score)
