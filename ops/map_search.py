"""``map_search`` — top-k similarity search over ``map_embed`` vectors on MI355X.

"Which corpus rows are nearest to this text?": the queries (texts embedded by the model, or
vectors given as numbers) are scored against a corpus (an ``.npy`` of ``map_embed``
``output: "npy"``, kept resident on the device, or texts embedded on the fly) by
``agent_tpu_amd/ops/search.py``: an exact fp32 similarity GEMM whose score matrix is never written,
with the top-k taken in its epilogue (see map_search.CONTRACT.md). ``filter`` restricts the search to
an allow-list or deny-list of row ids, or to the rows whose label (``corpus_labels_uri``) is in a set
or a range: the rows become a bit mask on the device and the kernel applies it in its epilogue.
``index`` asks for an approximate search through an inverted-file (IVF) index: the resident corpus sorted by
k-means cluster (``agent_tpu_amd/runtime/ivf.py``), every query scored against the rows of the ``nprobe``
clusters nearest to it only (``ops.sim_topk_ivf``); the scores stay exact and the ids are the original rows.
``compression`` keeps the corpus product-quantized (``agent_tpu_amd/runtime/pq.py``): ``subvectors`` bytes per row
instead of ``4 dim``, scored from a per-query table of sub-vector dot products (``ops.sim_topk_pq``); the scores
are approximate.

Under ``torchrun`` every rank embeds the queries, searches its slice of the corpus, and rank 0
merges the per-rank lists in the same total order (score descending, id ascending). Errors are
``ValueError`` s with the fixed messages of :data:`ERRORS`; there is no fallback stub.
"""
from __future__ import annotations

import math
import os
from typing import Any, Dict, List, NamedTuple, Optional

from . import _jobs, register_batch_op, register_op

OP_NAME = "map_search"
MAX_TOP_K = 32
PAD_ID = 2 ** 62  # id of the (-inf) padding of a rank's list that is shorter than top_k

#: every input error of the op (each listed in map_search.CONTRACT.md)
ERRORS: Dict[str, str] = {
    "missing_queries": 'payload missing required key: "queries" (or "query_vectors")',
    "missing_corpus": 'payload missing required key: "corpus_uri" (or "corpus_texts")',
    "queries": "payload.queries must be a list of strings",
    "query_vectors": "payload.query_vectors must be a list of equal-length, non-empty lists of finite numbers",
    "corpus_texts": "payload.corpus_texts must be a list of strings and needs payload.queries (a model embeds both)",
    "top_k": "payload.top_k must be an integer from 1 to 32",
    "metric": "payload.metric must be 'cosine' or 'dot'",
    "pooling": "payload.pooling must be 'mean' or 'cls'",
    "min_score": "payload.min_score must be a finite number",
    "corpus_file": "corpus_uri must be a local 2-D float32 or float16 .npy file",
    "corpus_empty": "corpus has no rows",
    "corpus_nonfinite": "corpus holds non-finite values",
    "dim": "corpus dim differs from the query dim (the model's hidden size or the query_vectors' length)",
    "corpus_too_large": "corpus slice exceeds SEARCH_INDEX_MAX_GB of float32",
}
#: those of ``corpus_dtype`` and of a float16-resident corpus (also in the contract)
F16_ERRORS: Dict[str, str] = {
    "corpus_dtype": "payload.corpus_dtype must be 'float32' or 'float16'",
    "corpus_dtype_env": "SEARCH_INDEX_DTYPE must be 'float32' or 'float16'",
    "corpus_f16_range": "corpus values exceed the float16 range",
    "corpus_too_large_f16": "corpus slice exceeds SEARCH_INDEX_MAX_GB of float16",
}
CORPUS_DTYPES = ("float32", "float16")
#: those of ``filter`` and ``corpus_labels_uri`` (also in the contract); ``{key}`` is ``ids`` or ``exclude_ids``
FILTER_ERRORS: Dict[str, str] = {
    "filter": "payload.filter must be an object with exactly one of 'ids', 'exclude_ids', 'labels', 'label_range'",
    "filter_ids": "payload.filter.{key} must be a list of at most 1048576 integers in [0, corpus rows)",
    "filter_labels": "payload.filter.labels must be a list of 1 to 256 integers",
    "filter_label_range": "payload.filter.label_range must be [lo, hi] with integers lo <= hi",
    "filter_labels_uri": "payload.filter on labels needs payload.corpus_labels_uri (with corpus_uri)",
    "labels_file": "corpus_labels_uri must be a local 1-D int32 or int64 .npy file with one label per corpus row",
}
FILTER_KEYS = ("ids", "exclude_ids", "labels", "label_range")
MAX_FILTER_IDS = 1048576
MAX_FILTER_LABELS = 256
#: those of ``index`` (also in the contract)
IVF_ERRORS: Dict[str, str] = {
    "index": ("payload.index must be {'type': 'ivf'} with optional integers 'clusters' in [1, min(4096, corpus rows)], "
              "'nprobe' in [1, min(32, clusters)] and 'train_iterations' in [1, 100]"),
    "index_corpus": "payload.index needs payload.corpus_uri (a resident corpus)",
    "index_metric": "payload.index needs metric 'cosine'",
    "index_f16": "payload.index needs a float32-resident corpus (corpus_dtype or SEARCH_INDEX_DTYPE is 'float16')",
    "index_filter": "payload.index cannot be combined with payload.filter",
    "index_too_large": "index build exceeds SEARCH_INDEX_MAX_GB (two float32 copies of the corpus slice)",
}
INDEX_KEYS = ("type", "clusters", "nprobe", "train_iterations")
MAX_CLUSTERS = 4096
MAX_NPROBE = 32  # sim_topk's MAX_K: the probe is a sim_topk call
MAX_TRAIN_ITERATIONS = 100
#: those of ``compression`` (also in the contract)
PQ_ERRORS: Dict[str, str] = {
    "compression": ("payload.compression must be {'type': 'pq', 'subvectors': M} with an integer M, a multiple of 4 up to "
                    "128 with corpus dim / M of 4, 8 or 16, and optional integers 'train_rows' in "
                    "[256, min(corpus rows, 1048576)] and 'train_iterations' in [1, 100]"),
    "compression_corpus": "payload.compression needs payload.corpus_uri (a resident corpus)",
    "compression_rows": "payload.compression needs a corpus of at least 256 rows",
    "compression_filter": "payload.compression cannot be combined with payload.filter",
    "compression_index": "payload.compression cannot be combined with payload.index",
    "compression_f16": "payload.compression cannot be combined with corpus_dtype 'float16' (the codes are the resident form)",
    "compression_too_large": "compressed corpus slice exceeds SEARCH_INDEX_MAX_GB of codes",
}
COMPRESSION_KEYS = ("type", "subvectors", "train_rows", "train_iterations")
MAX_SUBVECTORS = 128
MIN_PQ_ROWS = 256
MAX_PQ_TRAIN_ROWS = 1048576


class Options(NamedTuple):
    top_k: int
    metric: str
    pooling: str
    min_score: Optional[float]
    corpus_dtype: str = "float32"  # residency of a corpus_uri corpus on the device
    filter: Optional[tuple] = None  # canonical: (key, sorted unique values or the (lo, hi) pair)
    labels_uri: Optional[str] = None  # corpus_labels_uri, kept only when a label filter uses it
    index: Optional[tuple] = None  # canonical: (clusters or None, nprobe or None, train_iterations)
    compression: Optional[tuple] = None  # canonical: (subvectors, train_rows or None, train_iterations)


def _number(x: Any) -> bool:
    return isinstance(x, (int, float)) and not isinstance(x, bool) and math.isfinite(x)


def _int64(x: Any) -> bool:
    return isinstance(x, int) and not isinstance(x, bool) and -2 ** 63 <= x < 2 ** 63


def parse_filter(payload: Dict[str, Any]):
    """``payload.filter`` in canonical form, ``(key, values)``, and the label file it needs (or None):
    everything about it that can be refused without the corpus."""
    f = payload["filter"]
    if not isinstance(f, dict) or len(f) != 1 or next(iter(f)) not in FILTER_KEYS:
        raise ValueError(FILTER_ERRORS["filter"])
    (key, v), = f.items()
    if key in ("ids", "exclude_ids"):
        if not isinstance(v, list) or len(v) > MAX_FILTER_IDS or not all(_int64(x) and x >= 0 for x in v):
            raise ValueError(FILTER_ERRORS["filter_ids"].format(key=key))
        return (key, tuple(sorted(set(v)))), None
    if key == "labels":
        if not isinstance(v, list) or not 1 <= len(v) <= MAX_FILTER_LABELS or not all(_int64(x) for x in v):
            raise ValueError(FILTER_ERRORS["filter_labels"])
        canon = (key, tuple(sorted(set(v))))
    else:
        if not isinstance(v, (list, tuple)) or len(v) != 2 or not all(_int64(x) for x in v) or v[0] > v[1]:
            raise ValueError(FILTER_ERRORS["filter_label_range"])
        canon = (key, (v[0], v[1]))
    if "corpus_uri" not in payload or "corpus_labels_uri" not in payload:
        raise ValueError(FILTER_ERRORS["filter_labels_uri"])
    uri = payload["corpus_labels_uri"]
    if not isinstance(uri, str) or not uri or ("://" in uri and not uri.startswith("file://")):
        raise ValueError(FILTER_ERRORS["labels_file"])
    return canon, uri


def parse_index(payload: Dict[str, Any], opt: Options) -> tuple:
    """``payload.index`` in canonical form, ``(clusters or None, nprobe or None, train_iterations)``: everything
    about it that can be refused without the corpus (:func:`resolve_index` does the rest)."""
    ix = payload["index"]
    if not isinstance(ix, dict) or ix.get("type") != "ivf" or not set(ix) <= set(INDEX_KEYS):
        raise ValueError(IVF_ERRORS["index"])

    def integer(key, hi, default):
        if key not in ix:
            return default
        v = ix[key]
        if not isinstance(v, int) or isinstance(v, bool) or not 1 <= v <= hi:
            raise ValueError(IVF_ERRORS["index"])
        return v

    canon = (integer("clusters", MAX_CLUSTERS, None), integer("nprobe", MAX_NPROBE, None),
             integer("train_iterations", MAX_TRAIN_ITERATIONS, 10))
    if canon[0] is not None and canon[1] is not None and canon[1] > canon[0]:
        raise ValueError(IVF_ERRORS["index"])
    if "corpus_uri" not in payload:
        raise ValueError(IVF_ERRORS["index_corpus"])
    if opt.metric != "cosine":
        raise ValueError(IVF_ERRORS["index_metric"])
    if opt.corpus_dtype != "float32":
        raise ValueError(IVF_ERRORS["index_f16"])
    if "filter" in payload:
        raise ValueError(IVF_ERRORS["index_filter"])
    return canon


def resolve_index(index: tuple, total: int) -> tuple:
    """(clusters, nprobe, train_iterations) of a canonical ``index`` for a corpus of ``total`` rows: the
    defaults ``ceil(sqrt(total))`` (clamped to ``[1, min(4096, total)]``) and ``min(8, clusters)``, and the
    bounds that need the corpus."""
    from agent_tpu_amd.runtime.ivf import default_clusters

    clusters, nprobe, t = index
    if clusters is None:
        clusters = default_clusters(total)
    elif clusters > total:
        raise ValueError(IVF_ERRORS["index"])
    if nprobe is None:
        nprobe = min(8, clusters)
    elif nprobe > clusters:
        raise ValueError(IVF_ERRORS["index"])
    return clusters, nprobe, t


def parse_compression(payload: Dict[str, Any]) -> tuple:
    """``payload.compression`` in canonical form, ``(subvectors, train_rows or None, train_iterations)``: everything
    about it that can be refused without the corpus (:func:`resolve_compression` does the rest)."""
    cp = payload["compression"]
    if not isinstance(cp, dict) or cp.get("type") != "pq" or not set(cp) <= set(COMPRESSION_KEYS):
        raise ValueError(PQ_ERRORS["compression"])

    def integer(key, lo, hi, default):
        if key not in cp:
            return default
        v = cp[key]
        if not isinstance(v, int) or isinstance(v, bool) or not lo <= v <= hi:
            raise ValueError(PQ_ERRORS["compression"])
        return v

    canon = (integer("subvectors", 4, MAX_SUBVECTORS, None), integer("train_rows", MIN_PQ_ROWS, MAX_PQ_TRAIN_ROWS, None),
             integer("train_iterations", 1, MAX_TRAIN_ITERATIONS, 10))
    if canon[0] is None or canon[0] % 4:
        raise ValueError(PQ_ERRORS["compression"])
    if "corpus_uri" not in payload:
        raise ValueError(PQ_ERRORS["compression_corpus"])
    if payload.get("corpus_dtype") == "float16":  # an explicit one; the environment's default does not apply to codes
        raise ValueError(PQ_ERRORS["compression_f16"])
    if "filter" in payload:
        raise ValueError(PQ_ERRORS["compression_filter"])
    if "index" in payload:
        raise ValueError(PQ_ERRORS["compression_index"])
    return canon


def resolve_compression(compression: tuple, total: int, dim: int) -> tuple:
    """(subvectors, train_rows, train_iterations) of a canonical ``compression`` for a corpus of ``total`` rows of
    ``dim`` columns: the default ``train_rows = min(total, 65536)`` and the bounds that need the corpus."""
    from agent_tpu_amd.ops import pq_ok
    from agent_tpu_amd.runtime.pq import default_train_rows

    M, T, t = compression
    if total < MIN_PQ_ROWS:
        raise ValueError(PQ_ERRORS["compression_rows"])
    if not pq_ok(dim, M):
        raise ValueError(PQ_ERRORS["compression"])
    if T is None:
        T = default_train_rows(total)
    elif T > total:
        raise ValueError(PQ_ERRORS["compression"])
    return M, T, t


def options(payload: Dict[str, Any]) -> Options:
    """The validated optional keys; raises the op's ``ValueError`` s before any device work."""
    top_k = payload.get("top_k", 10)
    if not isinstance(top_k, int) or isinstance(top_k, bool) or not 1 <= top_k <= MAX_TOP_K:
        raise ValueError(ERRORS["top_k"])
    metric = payload.get("metric", "cosine")
    if metric not in ("cosine", "dot"):
        raise ValueError(ERRORS["metric"])
    pooling = payload.get("pooling", "mean")
    if pooling not in ("mean", "cls"):
        raise ValueError(ERRORS["pooling"])
    min_score = payload.get("min_score")
    if min_score is not None and not _number(min_score):
        raise ValueError(ERRORS["min_score"])
    if "corpus_dtype" in payload:  # the payload wins: the environment is not looked at
        corpus_dtype = payload["corpus_dtype"]
        if corpus_dtype not in CORPUS_DTYPES:
            raise ValueError(F16_ERRORS["corpus_dtype"])
    else:
        corpus_dtype = os.getenv("SEARCH_INDEX_DTYPE", "float32")
        if corpus_dtype not in CORPUS_DTYPES:
            raise ValueError(F16_ERRORS["corpus_dtype_env"])
    return Options(top_k, metric, pooling, None if min_score is None else float(min_score), corpus_dtype)


def check_payload(payload: Dict[str, Any]) -> Options:
    """Everything that can be refused without a device or a file: options, then the query and
    corpus forms."""
    opt = options(payload)
    if "queries" in payload:
        if not isinstance(payload["queries"], list):
            raise ValueError(ERRORS["queries"])
    elif "query_vectors" in payload:
        qv = payload["query_vectors"]
        ok = isinstance(qv, list) and all(isinstance(v, list) and v for v in qv)
        ok = ok and len({len(v) for v in qv}) <= 1 and all(_number(x) for v in qv for x in v)
        if not ok:
            raise ValueError(ERRORS["query_vectors"])
    else:
        raise ValueError(ERRORS["missing_queries"])
    if "corpus_uri" in payload:
        from agent_tpu_amd.runtime.search import local_path

        local_path(payload["corpus_uri"])  # a remote or non-string uri: ERRORS["corpus_file"]
    elif "corpus_texts" in payload:
        if not isinstance(payload["corpus_texts"], list) or "queries" not in payload:
            raise ValueError(ERRORS["corpus_texts"])
    else:
        raise ValueError(ERRORS["missing_corpus"])
    if "filter" in payload:  # a job without one keeps its Options, its code path and its result keys
        flt, labels_uri = parse_filter(payload)
        opt = opt._replace(filter=flt, labels_uri=labels_uri)
    if "index" in payload:  # likewise: a job without one is untouched
        opt = opt._replace(index=parse_index(payload, opt))
    if "compression" in payload:  # likewise
        opt = opt._replace(compression=parse_compression(payload))
    return opt


def _texts(rows: List[Any]) -> List[str]:
    return ["" if t is None else str(t) for t in rows]


def slice_mask(flt, labels_uri, total: int, s_r: int, n_r: int, device):
    """The ``ops.RowMask`` of rows ``[s_r, s_r + n_r)`` of a corpus of ``total`` rows for the canonical
    filter ``flt`` (None for an empty slice): ids go in as they are, with the slice start as the
    builder's base; labels are loaded for the slice only."""
    from agent_tpu_amd import ops
    from agent_tpu_amd.runtime import search as rs

    key, vals = flt
    if key in ("ids", "exclude_ids"):
        if vals and vals[-1] >= total:  # sorted: the largest decides; the same on every rank
            raise ValueError(FILTER_ERRORS["filter_ids"].format(key=key))
        if n_r == 0:
            return None
        return ops.row_mask_from_ids(list(vals), n_r, base=s_r, exclude=key == "exclude_ids", device=device)
    labels = rs.load_labels(labels_uri, s_r, n_r, device, total)  # every rank checks the file against total
    if n_r == 0:
        return None
    if key == "labels":
        return ops.row_mask_from_labels(labels, values=list(vals))
    return ops.row_mask_from_labels(labels, lo=vals[0], hi=vals[1])


def search_queries(h, device, qvecs, payload: Dict[str, Any], top_k: int, metric: str, pooling: str,
                   rank: int, ws: int, corpus_dtype: str = "float32", flt=None, labels_uri=None):
    """Every rank: this rank's slice of the corpus (resident as ``corpus_dtype`` in the ``corpus_uri``
    form) searched for all ``qvecs [nq, dim]`` (host or device fp32, already normalised for
    cosine), the per-rank lists padded to ``top_k``,
    all-gathered and merged. -> (scores ``[nq, kk]``, ids ``[nq, kk]`` on the host, corpus rows,
    index_cached or None, filter_rows or None) on rank 0, None elsewhere. Local errors are exchanged
    before the collective, so a bad corpus fails every rank together with the single-process message.
    With a filter ``flt`` (canonical form) every rank masks its own slice; the ranks' counts of allowed
    rows travel with the error exchange, and their sum is ``filter_rows``."""
    import torch

    from agent_tpu_amd.parallel.dp import all_gather_rows, split_range
    from agent_tpu_amd.parallel.dp_ops import exchange_errors, maybe_inject_fault
    from agent_tpu_amd.runtime import search as rs

    cosine = metric == "cosine"
    exc, s, i, total, cached, scale, allowed = None, None, None, 0, None, None, 0
    nq, dim = int(qvecs.shape[0]), int(qvecs.shape[1])
    try:
        if "corpus_uri" in payload:
            total, cdim = rs.corpus_shape(payload["corpus_uri"])
            if cdim != dim:
                raise ValueError(ERRORS["dim"])
            s_r, n_r = split_range(0, total, ws, rank)
            corpus = rs.load_corpus(payload["corpus_uri"], s_r, n_r, cosine, device, corpus_dtype)
            vec, cached, scale = corpus.vectors, corpus.cached, corpus.scale
        else:  # corpus_texts: each rank embeds its slice; ids index the list; nothing is cached
            texts = _texts(payload["corpus_texts"])
            total = len(texts)
            if total == 0:
                raise ValueError(ERRORS["corpus_empty"])
            s_r, n_r = split_range(0, total, ws, rank)
            vec = h.engine.embed_texts(texts[s_r:s_r + n_r], pooling, cosine).emb.to(device)
        maybe_inject_fault("search")
        if flt is None:
            s, i = rs.search(qvecs, vec, top_k, id_base=s_r, row_scale=scale)
        else:
            mask = slice_mask(flt, labels_uri, total, s_r, n_r, vec.device)
            allowed = mask.count if mask is not None else 0
            s, i = rs.search(qvecs, vec, top_k, id_base=s_r, row_scale=scale, mask=mask)
        if s.shape[1] < top_k:  # a slice shorter than top_k: pad, so every rank gathers [nq, top_k]
            pad = top_k - s.shape[1]
            s = torch.cat([s, torch.full((nq, pad), float("-inf"), dtype=s.dtype, device=s.device)], 1)
            i = torch.cat([i, torch.full((nq, pad), PAD_ID, dtype=i.dtype, device=i.device)], 1)
    except Exception as e:
        exc = e
    filter_rows = None
    if flt is None:
        counts = exchange_errors(exc, nq if s is not None else 0)
    else:  # (rows, allowed rows of the slice) in the same object exchange
        extras = exchange_errors(exc, (nq if s is not None else 0, allowed))
        counts, filter_rows = [e[0] for e in extras], sum(e[1] for e in extras)
    s, i = all_gather_rows(s.contiguous(), i.contiguous(), counts=counts)
    if rank != 0:
        return None
    s, i = s.cpu(), i.cpu()
    if ws > 1:  # [ws * nq, top_k] in rank order -> every query's ws lists side by side -> merged
        s = s.view(ws, nq, top_k).permute(1, 0, 2).reshape(nq, ws * top_k)
        i = i.view(ws, nq, top_k).permute(1, 0, 2).reshape(nq, ws * top_k)
        s, i = rs.merge_topk(s, i, top_k)
    kk = min(top_k, total if filter_rows is None else filter_rows)
    return s[:, :kk], i[:, :kk], total, cached, filter_rows


def search_queries_ivf(device, qvecs, payload: Dict[str, Any], top_k: int, index: tuple, rank: int, ws: int):
    """:func:`search_queries` through an IVF index (``runtime/ivf.py``): every rank probes with the same global
    centroids and searches its own cluster-sorted slice with ``id_base`` = the slice start; the lists, already
    padded to ``top_k``, are all-gathered and merged as the exact ones are. The union of the ranks' probed rows
    is the probed clusters of the whole corpus, so the result has the same bits for every world size. The build
    contains collectives: the ranks' hit / miss flags travel with the error exchange, and all rebuild if any
    missed. -> (scores, ids on the host, padded to ``top_k``; corpus rows; index_cached; the result's ``index``
    dict) on rank 0, None elsewhere."""
    from agent_tpu_amd.parallel.dp import all_gather_rows, split_range
    from agent_tpu_amd.parallel.dp_ops import exchange_errors, maybe_inject_fault
    from agent_tpu_amd.runtime import ivf
    from agent_tpu_amd.runtime import search as rs

    exc, total, key, hit, corpus, s_r = None, 0, None, None, None, 0
    nq, dim = int(qvecs.shape[0]), int(qvecs.shape[1])
    try:
        total, cdim = rs.corpus_shape(payload["corpus_uri"])
        if cdim != dim:
            raise ValueError(ERRORS["dim"])
        clusters, nprobe, t = resolve_index(index, total)
        s_r, n_r = split_range(0, total, ws, rank)
        key, hit, corpus = ivf.open_index(payload["corpus_uri"], s_r, n_r, device, clusters, t)
    except Exception as e:
        exc = e
    hits = exchange_errors(exc, hit is not None)  # raises on every rank together
    if all(hits):
        idx = hit
    else:  # a collective: every rank builds, a rank that had the entry from its own rows
        x = corpus.vectors if corpus is not None else ivf.original_rows(hit)
        idx = ivf.build_index(key, x, clusters, t, rank, ws, s_r, total)
    s, i = None, None
    try:
        maybe_inject_fault("search")
        s, i, _ = ivf.search(qvecs, idx, top_k, nprobe, id_base=s_r)
    except Exception as e:
        exc = e
    counts = exchange_errors(exc, nq if s is not None else 0)
    s, i = all_gather_rows(s.contiguous(), i.contiguous(), counts=counts)
    if rank != 0:
        return None
    s, i = s.cpu(), i.cpu()
    if ws > 1:  # as search_queries: every query's ws lists side by side -> merged; the padding sorts last
        s = s.view(ws, nq, top_k).permute(1, 0, 2).reshape(nq, ws * top_k)
        i = i.view(ws, nq, top_k).permute(1, 0, 2).reshape(nq, ws * top_k)
        s, i = rs.merge_topk(s, i, top_k)
    info = {"type": "ivf", "clusters": clusters, "nprobe": nprobe, "train_iterations": idx.iterations,
            "converged": idx.converged}
    return s, i, total, idx.cached, info


def search_queries_pq(device, qvecs, payload: Dict[str, Any], top_k: int, metric: str, compression: tuple, rank: int,
                      ws: int):
    """:func:`search_queries` over a product-quantized corpus (``runtime/pq.py``): every rank trains the same
    codebooks from the same sample of the file (no collective), encodes its own slice chunk by chunk and scans its
    codes with ``id_base`` = the slice start; the lists are padded to ``top_k``, all-gathered and merged as the exact
    ones are. A row's ADC score depends on the query, the codebooks and the row's codes only, so the result has the
    same bits for every world size. -> (scores, ids on the host; corpus rows; index_cached; the result's
    ``compression`` dict) on rank 0, None elsewhere."""
    import torch

    from agent_tpu_amd.parallel.dp import all_gather_rows, split_range
    from agent_tpu_amd.parallel.dp_ops import exchange_errors, maybe_inject_fault
    from agent_tpu_amd.runtime import pq
    from agent_tpu_amd.runtime import search as rs

    exc, s, i, total, cached, info = None, None, None, 0, None, None
    nq, dim = int(qvecs.shape[0]), int(qvecs.shape[1])
    try:
        total, cdim = rs.corpus_shape(payload["corpus_uri"])
        if cdim != dim:
            raise ValueError(ERRORS["dim"])
        M, T, t = resolve_compression(compression, total, cdim)
        s_r, n_r = split_range(0, total, ws, rank)
        idx = pq.load_index(payload["corpus_uri"], s_r, n_r, device, M, T, t, metric == "cosine")
        cached = idx.cached
        info = {"type": "pq", "subvectors": M, "train_rows": T, "train_iterations": t, "bytes_per_row": M}
        maybe_inject_fault("search")
        s, i = pq.search(qvecs, idx, top_k, id_base=s_r)
        if s.shape[1] < top_k:  # a slice shorter than top_k: pad, so every rank gathers [nq, top_k]
            pad = top_k - s.shape[1]
            s = torch.cat([s, torch.full((nq, pad), float("-inf"), dtype=s.dtype, device=s.device)], 1)
            i = torch.cat([i, torch.full((nq, pad), PAD_ID, dtype=i.dtype, device=i.device)], 1)
    except Exception as e:
        exc = e
    counts = exchange_errors(exc, nq if s is not None else 0)
    s, i = all_gather_rows(s.contiguous(), i.contiguous(), counts=counts)
    if rank != 0:
        return None
    s, i = s.cpu(), i.cpu()
    if ws > 1:  # as search_queries: every query's ws lists side by side -> merged; the padding sorts last
        s = s.view(ws, nq, top_k).permute(1, 0, 2).reshape(nq, ws * top_k)
        i = i.view(ws, nq, top_k).permute(1, 0, 2).reshape(nq, ws * top_k)
        s, i = rs.merge_topk(s, i, top_k)
    kk = min(top_k, total)
    return s[:, :kk], i[:, :kk], total, cached, info


def embed_queries(h, device, payload: Dict[str, Any], queries: Optional[List[str]], metric: str, pooling: str):
    """``[nq, dim]`` fp32 query vectors: the model's embeddings of ``queries``, or ``query_vectors``
    on the device (normalised there for cosine)."""
    import torch

    from agent_tpu_amd.runtime.search import normalize_rows

    if queries is not None:
        return h.engine.embed_texts(queries, pooling, metric == "cosine").emb
    rows = payload["query_vectors"]
    qv = torch.tensor(rows, dtype=torch.float32).reshape(len(rows), len(rows[0]) if rows else 0).to(device)
    return normalize_rows(qv) if metric == "cosine" and len(rows) else qv


def result(h, scores, ids, payload: Dict[str, Any], top_k: int, total: int, dim: int, cached: Optional[bool],
           ws: int, filter_rows: Optional[int] = None, index_info: Optional[Dict[str, Any]] = None,
           compression_info: Optional[Dict[str, Any]] = None) -> Dict[str, Any]:
    """One job's result from its rows of the merged lists (rank 0): the first ``top_k`` entries (with
    a total order a prefix of the top-K is the top-k), then the ``min_score`` cut on the host.
    ``filter_rows``: the corpus rows that passed the job's filter (None: no filter). ``index_info``: the
    ``index`` key of a job with an index (None: no index); its lists end where the padding begins."""
    opt = options(payload)
    kk = min(top_k, total if filter_rows is None else filter_rows)
    ids_l, sc_l = ids[:, :kk].tolist(), scores[:, :kk].tolist()
    if index_info is not None:  # a query whose probed clusters hold fewer than top_k rows: a shorter list
        keep = [sum(1 for x in row if x != PAD_ID) for row in ids_l]
        ids_l = [row[:m] for row, m in zip(ids_l, keep)]
        sc_l = [row[:m] for row, m in zip(sc_l, keep)]
    if opt.min_score is not None:
        keep = [[j for j, v in enumerate(row) if v >= opt.min_score] for row in sc_l]
        ids_l = [[row[j] for j in ks] for row, ks in zip(ids_l, keep)]
        sc_l = [[row[j] for j in ks] for row, ks in zip(sc_l, keep)]
    n = len(ids_l)
    elapsed_ms, rate = _jobs.timing(payload, n)
    out: Dict[str, Any] = {"ok": True, "op": payload.get("_op", OP_NAME), "query_count": n, "corpus_rows": total,
                           "dim": dim, "top_k": top_k, "metric": opt.metric, "elapsed_ms": elapsed_ms,
                           "queries_per_sec": rate}
    if h is not None:
        out.update(model_path=h.model_path, pooling=opt.pooling)
    if ws > 1:
        out["dp_world_size"] = ws
    if cached is not None:
        out["index_cached"] = bool(cached)
    # default-path results keep their keys; a compressed corpus is resident as codes, whatever the default dtype
    if "corpus_uri" in payload and opt.corpus_dtype != "float32" and compression_info is None:
        out["corpus_dtype"] = opt.corpus_dtype
    if filter_rows is not None:
        out["filter_rows"] = int(filter_rows)
    if index_info is not None:
        out["index"] = dict(index_info)
    if compression_info is not None:
        out["compression"] = dict(compression_info)
    out.update(ids=ids_l, scores=sc_l)
    return out


def _handle_and_device(payload: Dict[str, Any]):
    """The model (a collective load under DP) when the job has ``queries``, and the device."""
    from ._gpu_runtime import device_for_rank, get_gpu_handle, get_model_path

    if "queries" in payload:
        h = get_gpu_handle(get_model_path(payload.get("model_path")))
        return h, h.engine.device
    return None, device_for_rank()


def search_one(payload: Dict[str, Any], rank: int, ws: int) -> Optional[Dict[str, Any]]:
    """One job (every rank calls it)."""
    opt = check_payload(payload)  # the same payload on every rank: all raise together
    h, device = _handle_and_device(payload)
    queries = _texts(payload["queries"]) if "queries" in payload else None
    nq = len(queries) if queries is not None else len(payload["query_vectors"])
    if "corpus_texts" in payload and not payload["corpus_texts"]:
        raise ValueError(ERRORS["corpus_empty"])
    qv = embed_queries(h, device, payload, queries, opt.metric, opt.pooling)
    if nq == 0:  # nothing to search for; the corpus is still checked
        import torch

        dim = h.cfg.hidden if h is not None else 0
        qv = torch.zeros((0, dim), dtype=torch.float32) if h is not None else None
        if qv is None:
            raise ValueError(ERRORS["query_vectors"])
    if opt.index is not None:  # its own path, so that a job without an index stays as it was
        got = search_queries_ivf(device, qv, payload, opt.top_k, opt.index, rank, ws)
        if got is None:
            return None
        s, i, total, cached, info = got
        return result(h, s, i, payload, opt.top_k, total, int(qv.shape[1]), cached, ws, index_info=info)
    if opt.compression is not None:  # likewise
        got = search_queries_pq(device, qv, payload, opt.top_k, opt.metric, opt.compression, rank, ws)
        if got is None:
            return None
        s, i, total, cached, info = got
        return result(h, s, i, payload, opt.top_k, total, int(qv.shape[1]), cached, ws, compression_info=info)
    got = search_queries(h, device, qv, payload, opt.top_k, opt.metric, opt.pooling, rank, ws, opt.corpus_dtype,
                         opt.filter, opt.labels_uri)
    if got is None:
        return None
    s, i, total, cached, filter_rows = got
    return result(h, s, i, payload, opt.top_k, total, int(qv.shape[1]), cached, ws, filter_rows)


def search_batch(payloads: List[Dict[str, Any]], rank: int, ws: int) -> Optional[List[Any]]:
    """The ``queries`` + ``corpus_uri`` jobs of one lease that share (model, pooling, metric, corpus,
    corpus_dtype, canonical filter and its label file, canonical index, canonical compression) as one engine
    call (every rank calls it): one embed of the concatenated queries, one search at the
    group's largest ``top_k``; each job takes the first ``top_k`` entries of its own rows."""
    out: List[Any] = [None] * len(payloads)
    jobs = []
    for n, p in enumerate(payloads):  # same payloads on every rank: same validation outcome
        try:
            jobs.append((n, check_payload(p), _texts(p["queries"])))
        except Exception as exc:
            out[n] = ("err", exc)
    if jobs:
        first = payloads[jobs[0][0]]
        key = jobs[0][1]
        h, device = _handle_and_device(first)
        K = max(opt.top_k for _, opt, _ in jobs)
        texts = [t for _, _, ts in jobs for t in ts]
        try:
            if device.type == "cuda":
                qv = h.engine.embed_texts(texts, key.pooling, key.metric == "cosine").emb
            else:
                # the fp32 PyTorch encoder of a CPU engine rounds a row differently in another batch
                # (BLAS blocking): one embed per job there, so every job keeps its single-job bits
                import torch

                qv = torch.cat([h.engine.embed_texts(ts, key.pooling, key.metric == "cosine").emb for _, _, ts in jobs])
            if key.index is not None:  # the group shares the canonical index, nprobe included
                got = search_queries_ivf(device, qv, first, K, key.index, rank, ws)
                got = None if got is None else got[:4] + (None, got[4], None)
            elif key.compression is not None:  # the group shares the canonical compression
                got = search_queries_pq(device, qv, first, K, key.metric, key.compression, rank, ws)
                got = None if got is None else got[:4] + (None, None, got[4])
            else:
                got = search_queries(h, device, qv, first, K, key.metric, key.pooling, rank, ws, key.corpus_dtype,
                                     key.filter, key.labels_uri)
                got = None if got is None else got + (None, None)
        except Exception as exc:  # a bad corpus is bad for every job of the group
            for n, _, _ in jobs:
                out[n] = ("err", exc)
            return out if rank == 0 else None
        if got is not None:
            s, i, total, cached, filter_rows, info, cinfo = got
            pos = 0
            for n, opt, ts in jobs:
                out[n] = ("ok", result(h, s[pos:pos + len(ts)], i[pos:pos + len(ts)], payloads[n], opt.top_k, total,
                                       int(qv.shape[1]), cached, ws, filter_rows, info, cinfo))
                pos += len(ts)
    return out if rank == 0 else None


@register_batch_op("map_search")
def map_search_batch(payloads: List[Dict[str, Any]]) -> List[Any]:
    """Batch handler: ``queries`` + ``corpus_uri`` jobs that share (model_path, pooling, metric,
    corpus_uri, corpus_dtype, with a ``filter`` its canonical form and label file, and with an ``index`` its
    canonical (clusters, train_iterations) and nprobe, and with a ``compression`` its canonical tuple) go to the device
    together; ``corpus_texts`` jobs, ``query_vectors`` jobs and malformed payloads take the
    single-job path."""

    def key(p):
        if "queries" not in p or "corpus_uri" not in p:
            raise KeyError("queries")  # not batchable
        opt = check_payload(p)
        group = p.get("model_path"), opt.pooling, opt.metric, p["corpus_uri"], opt.corpus_dtype
        if opt.index is not None:  # (clusters, train_iterations) name the index; jobs that differ in nprobe probe
            clusters, nprobe, t = opt.index  # other rows per query, so they stay separate groups
            return group + ("ivf", clusters, t, nprobe)
        if opt.compression is not None:  # the canonical tuple names the codebooks and the codes
            return group + ("pq",) + opt.compression
        return group if opt.filter is None else group + (opt.filter, opt.labels_uri)  # equal filters share a search

    return _jobs.lease_batch(payloads, OP_NAME, "map_search_batch", key, run)


def run(payload: Dict[str, Any], ctx: Dict[str, Any] = None) -> Dict[str, Any]:
    return _jobs.run_single(payload, OP_NAME, OP_NAME, check_payload)


@register_op("map_search")
def map_search(payload: Dict[str, Any], ctx: Dict[str, Any] = None) -> Dict[str, Any]:
    return run(payload, ctx)
