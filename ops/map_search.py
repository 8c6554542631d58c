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
``index`` of type ``ivfpq`` combines the two below (``agent_tpu_amd/runtime/ivfpq.py``): coarse clusters with
product-quantization codes of the residuals, every query scored against the codes of the clusters it probes only
(``ops.sim_topk_ivfpq``).
``compression`` keeps the corpus product-quantized (``agent_tpu_amd/runtime/pq.py``): ``subvectors`` bytes per row
instead of ``4 dim``, scored from a per-query table of sub-vector dot products (``ops.sim_topk_pq``); the scores
are approximate. ``compression`` of type ``binary`` keeps one bit per dimension instead (``agent_tpu_amd/runtime/binary.py``):
``dim / 8`` bytes per row, scored by the Hamming distance against the query's bits (``ops.sim_topk_binary``); with
``refine`` its shortlist is re-scored exactly.
``depth`` (33 to 1024, in place of ``top_k``) asks for deep result lists, the input of re-rankers and late-interaction
scoring: the same exact search through ``ops.sim_topk_wide``, whose selection is a threshold filter and a sorted
candidate buffer instead of ``sim_topk``'s register lists.

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
#: those of ``compression: {"type": "binary"}`` (also in the contract)
BINARY_ERRORS: Dict[str, str] = {
    "binary": "payload.compression of type 'binary' must be {'type': 'binary'} with an optional 'threshold' of 'zero' or 'mean'",
    "binary_corpus": "payload.compression of type 'binary' needs payload.corpus_uri (a resident corpus)",
    "binary_f16": ("payload.compression of type 'binary' cannot be combined with corpus_dtype 'float16' (the bits are the "
                   "resident form)"),
    "binary_filter": "payload.compression of type 'binary' cannot be combined with payload.filter",
    "binary_index": "payload.compression of type 'binary' cannot be combined with payload.index",
    "binary_dim": "payload.compression of type 'binary' needs a corpus dim that is a multiple of 64 from 64 to 1024",
    "binary_too_large": "binary corpus slice exceeds SEARCH_INDEX_MAX_GB of codes",
}
BINARY_KEYS = ("type", "threshold")
BINARY_THRESHOLDS = ("zero", "mean")
#: those of ``index: {"type": "ivfpq"}`` (also in the contract)
IVFPQ_ERRORS: Dict[str, str] = {
    "ivfpq": ("payload.index of type 'ivfpq' must have an integer 'subvectors', a multiple of 4 up to 128 with corpus "
              "dim / subvectors of 4, 8 or 16, and optional integers 'clusters' in [1, min(4096, train_rows)], 'nprobe' "
              "in [1, min(32, clusters)], 'train_rows' in [256, min(corpus rows, 1048576)] and 'train_iterations' in "
              "[1, 100]"),
    "ivfpq_corpus": "payload.index of type 'ivfpq' needs payload.corpus_uri (a resident corpus)",
    "ivfpq_metric": "payload.index of type 'ivfpq' needs metric 'cosine'",
    "ivfpq_dim": "payload.index of type 'ivfpq' needs a corpus dim that is a multiple of 64 from 64 to 1024",
    "ivfpq_rows": "payload.index of type 'ivfpq' needs a corpus of at least 256 rows",
    "ivfpq_filter": "payload.index of type 'ivfpq' cannot be combined with payload.filter",
    "ivfpq_compression": "payload.index of type 'ivfpq' cannot be combined with payload.compression (it holds the codes)",
    "ivfpq_f16": "payload.index of type 'ivfpq' cannot be combined with corpus_dtype 'float16' (the codes are the resident form)",
    "ivfpq_too_large": "ivfpq index slice exceeds SEARCH_INDEX_MAX_GB of codes and row ids",
}
IVFPQ_KEYS = ("type", "subvectors", "clusters", "nprobe", "train_rows", "train_iterations")
#: those of ``refine`` (also in the contract)
REFINE_ERRORS: Dict[str, str] = {
    "refine": ("payload.refine must be {'candidates': R} with an integer R, a multiple of 32 from 32 to 8192 and at "
               "least top_k, and optional 'vectors' of 'float16' or 'float32' and 'store' of 'host' or 'device'"),
    "refine_compression": "payload.refine needs payload.compression (it re-scores the compressed search's shortlist)",
    "refine_filter": "payload.refine cannot be combined with payload.filter",
    "refine_index": "payload.refine cannot be combined with payload.index",
    "refine_too_large": ("refine store of the corpus slice exceeds SEARCH_REFINE_MAX_GB of pinned host memory "
                         "(store 'device': SEARCH_INDEX_MAX_GB together with the codes)"),
}
REFINE_KEYS = ("candidates", "vectors", "store")
REFINE_VECTORS = ("float16", "float32")
REFINE_STORES = ("host", "device")
MAX_REFINE_CANDIDATES = 8192  # 32 * MAX_SPLITS: one list of 32 per segment
#: those of ``diversify`` (also in the contract)
DIVERSIFY_ERRORS: Dict[str, str] = {
    "diversify": ("payload.diversify must be an object with optional 'lambda', a number from 0 to 1, and 'candidates', an "
                  "integer from max(top_k, 2) to 32"),
    "diversify_index": "payload.diversify cannot be combined with payload.index",
    "diversify_compression": "payload.diversify cannot be combined with payload.compression",
}
DIVERSIFY_KEYS = ("lambda", "candidates")
MAX_DIVERSIFY_CANDIDATES = 32  # MAX_TOP_K: the candidates are one sim_topk list
#: those of ``depth`` (also in the contract)
DEPTH_ERRORS: Dict[str, str] = {
    "depth": "payload.depth must be an integer from 33 to 1024, given without top_k",
    "depth_combined": "payload.depth cannot be combined with filter, index, compression, refine or diversify",
}
MAX_DEPTH = 1024  # ops.WIDE_MAX_K: the list is one sim_topk_wide call
DEPTH_EXCLUDES = ("filter", "index", "compression", "refine", "diversify")


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
    ivfpq: Optional[tuple] = None  # canonical: (clusters or None, nprobe or None, subvectors, train_rows or None, iterations)
    refine: Optional[tuple] = None  # canonical: (candidates, vectors, store)
    binary: Optional[tuple] = None  # canonical: (threshold,)
    diversify: Optional[tuple] = None  # canonical: (lambda, candidates)
    depth: Optional[int] = None  # the list length of a deep search (33 .. 1024), in place of top_k


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


def parse_ivfpq(payload: Dict[str, Any], opt: Options) -> tuple:
    """``payload.index`` of type ``ivfpq`` in canonical form, ``(clusters or None, nprobe or None, subvectors,
    train_rows or None, train_iterations)``: everything about it that can be refused without the corpus
    (:func:`resolve_ivfpq` does the rest)."""
    ix = payload["index"]
    if not set(ix) <= set(IVFPQ_KEYS):
        raise ValueError(IVFPQ_ERRORS["ivfpq"])

    def integer(key, lo, hi, default):
        if key not in ix:
            return default
        v = ix[key]
        if not isinstance(v, int) or isinstance(v, bool) or not lo <= v <= hi:
            raise ValueError(IVFPQ_ERRORS["ivfpq"])
        return v

    canon = (integer("clusters", 1, MAX_CLUSTERS, None), integer("nprobe", 1, MAX_NPROBE, None),
             integer("subvectors", 4, MAX_SUBVECTORS, None), integer("train_rows", MIN_PQ_ROWS, MAX_PQ_TRAIN_ROWS, None),
             integer("train_iterations", 1, MAX_TRAIN_ITERATIONS, 10))
    if canon[2] is None or canon[2] % 4 or (canon[0] is not None and canon[1] is not None and canon[1] > canon[0]):
        raise ValueError(IVFPQ_ERRORS["ivfpq"])
    if "corpus_uri" not in payload:
        raise ValueError(IVFPQ_ERRORS["ivfpq_corpus"])
    if opt.metric != "cosine":
        raise ValueError(IVFPQ_ERRORS["ivfpq_metric"])
    if payload.get("corpus_dtype") == "float16":  # an explicit one; the environment's default does not apply to codes
        raise ValueError(IVFPQ_ERRORS["ivfpq_f16"])
    if "filter" in payload:
        raise ValueError(IVFPQ_ERRORS["ivfpq_filter"])
    if "compression" in payload:
        raise ValueError(IVFPQ_ERRORS["ivfpq_compression"])
    return canon


def resolve_ivfpq(ivfpq: tuple, total: int, dim: int) -> tuple:
    """(clusters, nprobe, subvectors, train_rows, train_iterations) of a canonical ``ivfpq`` for a corpus of ``total``
    rows of ``dim`` columns: PQ's default ``train_rows = min(total, 65536)``, IVF's defaults ``ceil(sqrt(total))``
    clusters (at most ``train_rows``: the centroids are trained on the sample) and ``nprobe = min(8, clusters)``, and
    the bounds that need the corpus."""
    from agent_tpu_amd.ops import pq_ok, sim_topk_ok
    from agent_tpu_amd.runtime.ivf import default_clusters
    from agent_tpu_amd.runtime.pq import default_train_rows

    clusters, nprobe, M, T, t = ivfpq
    if total < MIN_PQ_ROWS:
        raise ValueError(IVFPQ_ERRORS["ivfpq_rows"])
    if not sim_topk_ok(dim, 1):
        raise ValueError(IVFPQ_ERRORS["ivfpq_dim"])
    if not pq_ok(dim, M):
        raise ValueError(IVFPQ_ERRORS["ivfpq"])
    if T is None:
        T = default_train_rows(total)
    elif T > total:
        raise ValueError(IVFPQ_ERRORS["ivfpq"])
    if clusters is None:
        clusters = min(default_clusters(total), T)
    elif clusters > T:
        raise ValueError(IVFPQ_ERRORS["ivfpq"])
    if nprobe is None:
        nprobe = min(8, clusters)
    elif nprobe > clusters:
        raise ValueError(IVFPQ_ERRORS["ivfpq"])
    return clusters, nprobe, M, T, t


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


def parse_binary(payload: Dict[str, Any]) -> tuple:
    """``payload.compression`` of type ``binary`` in canonical form, ``(threshold,)``: everything about it that can be
    refused without the corpus (the corpus dim is checked when the file is opened, before any device work)."""
    cp = payload["compression"]
    if not set(cp) <= set(BINARY_KEYS) or cp.get("threshold", "zero") not in BINARY_THRESHOLDS:
        raise ValueError(BINARY_ERRORS["binary"])
    if "corpus_uri" not in payload:
        raise ValueError(BINARY_ERRORS["binary_corpus"])
    if payload.get("corpus_dtype") == "float16":  # an explicit one; the environment's default does not apply to codes
        raise ValueError(BINARY_ERRORS["binary_f16"])
    if "filter" in payload:
        raise ValueError(BINARY_ERRORS["binary_filter"])
    if "index" in payload:
        raise ValueError(BINARY_ERRORS["binary_index"])
    return (cp.get("threshold", "zero"),)


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


def parse_refine(payload: Dict[str, Any], opt: Options) -> tuple:
    """``payload.refine`` in canonical form, ``(candidates, vectors, store)``; all of it can be refused without the
    corpus."""
    rf = payload["refine"]
    if not isinstance(rf, dict) or not set(rf) <= set(REFINE_KEYS):
        raise ValueError(REFINE_ERRORS["refine"])
    R, vectors, store = rf.get("candidates"), rf.get("vectors", "float16"), rf.get("store", "host")
    if not isinstance(R, int) or isinstance(R, bool) or R % 32 or not max(32, opt.top_k) <= R <= MAX_REFINE_CANDIDATES \
            or vectors not in REFINE_VECTORS or store not in REFINE_STORES:
        raise ValueError(REFINE_ERRORS["refine"])
    if "filter" in payload:
        raise ValueError(REFINE_ERRORS["refine_filter"])
    if "index" in payload:
        raise ValueError(REFINE_ERRORS["refine_index"])
    if "compression" not in payload:
        raise ValueError(REFINE_ERRORS["refine_compression"])
    return R, vectors, store


def parse_diversify(payload: Dict[str, Any], opt: Options) -> tuple:
    """``payload.diversify`` in canonical form, ``(lambda, candidates)``; all of it can be refused without the corpus."""
    dv = payload["diversify"]
    if not isinstance(dv, dict) or not set(dv) <= set(DIVERSIFY_KEYS):
        raise ValueError(DIVERSIFY_ERRORS["diversify"])
    lam, R = dv.get("lambda", 0.5), dv.get("candidates", MAX_DIVERSIFY_CANDIDATES)
    if not _number(lam) or not 0 <= lam <= 1 or not isinstance(R, int) or isinstance(R, bool) \
            or not max(opt.top_k, 2) <= R <= MAX_DIVERSIFY_CANDIDATES:
        raise ValueError(DIVERSIFY_ERRORS["diversify"])
    if "index" in payload:  # their rows are not resident in the original order
        raise ValueError(DIVERSIFY_ERRORS["diversify_index"])
    if "compression" in payload:
        raise ValueError(DIVERSIFY_ERRORS["diversify_compression"])
    return float(lam), R


def parse_depth(payload: Dict[str, Any]) -> int:
    """``payload.depth``; all of it can be refused without the corpus."""
    d = payload["depth"]
    if not isinstance(d, int) or isinstance(d, bool) or not MAX_TOP_K < d <= MAX_DEPTH or "top_k" in payload:
        raise ValueError(DEPTH_ERRORS["depth"])
    if any(key in payload for key in DEPTH_EXCLUDES):
        raise ValueError(DEPTH_ERRORS["depth_combined"])
    return d


def list_length(opt: Options) -> int:
    """The entries a job asks for per query: its ``depth``, or its ``top_k``."""
    return opt.top_k if opt.depth is None else opt.depth


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
    """Everything that can be refused without a device or a file: :func:`check_forms`, then ``diversify``, so that
    every other error comes first."""
    opt = check_forms(payload)
    if "diversify" in payload:  # a job without one keeps its Options, its code path and its result keys
        opt = opt._replace(diversify=parse_diversify(payload, opt))
    return opt


def check_forms(payload: Dict[str, Any]) -> Options:
    """Options, then the query and corpus forms, then the keys that choose a search path."""
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
    if "depth" in payload:  # a job without one keeps its Options, its code path and its result keys; it joins none
        return opt._replace(depth=parse_depth(payload))  # of the keys below
    if "filter" in payload:  # a job without one keeps its Options, its code path and its result keys
        flt, labels_uri = parse_filter(payload)
        opt = opt._replace(filter=flt, labels_uri=labels_uri)
    if "refine" in payload:  # likewise; refused before the forms it cannot join are looked at
        opt = opt._replace(refine=parse_refine(payload, opt))
    if isinstance(payload.get("index"), dict) and payload["index"].get("type") == "ivfpq":  # a third path of its own
        return opt._replace(ivfpq=parse_ivfpq(payload, opt))
    if "index" in payload:  # likewise: a job without one is untouched
        opt = opt._replace(index=parse_index(payload, opt))
    cp = payload.get("compression")
    if isinstance(cp, dict) and isinstance(cp.get("type"), str) and cp["type"] == "binary":  # a path of its own beside PQ
        return opt._replace(binary=parse_binary(payload))
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
                   rank: int, ws: int, corpus_dtype: str = "float32", flt=None, labels_uri=None, diversify=None):
    """Every rank: this rank's slice of the corpus (resident as ``corpus_dtype`` in the ``corpus_uri``
    form) searched for all ``qvecs [nq, dim]`` (host or device fp32, already normalised for
    cosine), the per-rank lists padded to ``top_k``,
    all-gathered and merged. -> (scores ``[nq, kk]``, ids ``[nq, kk]`` on the host, corpus rows,
    index_cached or None, filter_rows or None) on rank 0, None elsewhere. Local errors are exchanged
    before the collective, so a bad corpus fails every rank together with the single-process message.
    With a filter ``flt`` (canonical form) every rank masks its own slice; the ranks' counts of allowed
    rows travel with the error exchange, and their sum is ``filter_rows``.
    With ``diversify`` (canonical form) the search runs at ``k = candidates`` and :func:`diversify_lists` picks
    ``top_k`` of every query's merged list; the tuple gains the picks' ``mmr`` values."""
    import torch

    from agent_tpu_amd.parallel.dp import all_gather_rows, split_range
    from agent_tpu_amd.parallel.dp_ops import exchange_errors, maybe_inject_fault
    from agent_tpu_amd.runtime import search as rs

    cosine = metric == "cosine"
    want = top_k
    if diversify is not None:  # the candidates: the (filtered) top-R
        top_k = diversify[1]
    exc, s, i, total, cached, scale, allowed, vec, s_r = None, None, None, 0, None, None, 0, None, 0
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
    if diversify is not None:  # its own tail, on every rank
        picks = diversify_lists(s, i, vec, scale, s_r, total, want, diversify, rank, ws)
        if picks is None:
            return None
        kk = min(want, total if filter_rows is None else filter_rows)
        pi, ps, pm = (t[:, :kk].cpu() for t in picks)
        return ps, pi, total, cached, filter_rows, pm
    if rank != 0:
        return None
    s, i = s.cpu(), i.cpu()
    if ws > 1:  # [ws * nq, top_k] in rank order -> every query's ws lists side by side -> merged
        s = s.view(ws, nq, top_k).permute(1, 0, 2).reshape(nq, ws * top_k)
        i = i.view(ws, nq, top_k).permute(1, 0, 2).reshape(nq, ws * top_k)
        s, i = rs.merge_topk(s, i, top_k)
    kk = min(top_k, total if filter_rows is None else filter_rows)
    return s[:, :kk], i[:, :kk], total, cached, filter_rows


def diversify_lists(s, i, vec, scale, s_r: int, total: int, top_k: int, diversify: tuple, rank: int, ws: int):
    """Every rank, after the all-gather of the ranks' top-``candidates`` lists ``s`` / ``i [ws * nq, R]``: the MMR picks
    of every query's merged list -> (ids, scores, mmr) ``[nq, top_k]`` on rank 0, None elsewhere. One process selects
    straight from its resident rows. Under DP every rank holds the gathered lists, so every rank computes the same
    merged ids; each copies the rows of its own slice into a ``[nq * R, dim]`` buffer (``ops.rows_gather``: zeros for
    the other slots), the buffers are gathered, and rank 0 takes each slot from its owning rank by select and runs
    the selection with that buffer as the store and its slot numbers as ids (the slots in ascending id, so that ties
    break as they do over the ids), then maps the picks back. A row's bits are the same wherever it was gathered, so
    the result equals the single-process one for every world size."""
    import torch

    from agent_tpu_amd import ops
    from agent_tpu_amd.parallel.dp import all_gather_rows, split_range
    from agent_tpu_amd.runtime import search as rs

    lam, R = diversify
    if ws == 1:
        return rs.diversify(s, i, vec, top_k, lam, id_base=s_r, row_scale=scale)
    nq = s.shape[0] // ws
    s = s.view(ws, nq, R).permute(1, 0, 2).reshape(nq, ws * R)
    i = i.view(ws, nq, R).permute(1, 0, 2).reshape(nq, ws * R)
    s, i = rs.merge_topk(s, i, R)  # [nq, R]: the same on every rank
    i, by_id = torch.sort(i, dim=1, stable=True)  # ascending id: rank 0's slot numbers then break ties as the ids do
    s = torch.gather(s, 1, by_id)
    flat = i.reshape(-1).to(vec.device).contiguous()
    if vec.shape[0]:
        rows, sc = ops.rows_gather(flat, vec, id_base=s_r, row_scale=scale)
    else:  # a rank beyond the corpus owns no slot
        rows, sc = vec.new_zeros((flat.numel(), vec.shape[1])), None
    if scale is None:
        (rows,) = all_gather_rows(rows, counts=[flat.numel()] * ws)
    else:
        sc = sc if sc is not None else torch.ones((flat.numel(),), dtype=torch.float32, device=vec.device)
        rows, sc = all_gather_rows(rows, sc, counts=[flat.numel()] * ws)
    if rank != 0:
        return None
    rows = rows.view(ws, flat.numel(), -1)
    store, st_scale = rows[0].clone(), (sc.view(ws, -1)[0].clone() if scale is not None else None)
    for r in range(1, ws):
        lo, n = split_range(0, total, ws, r)
        own = (flat >= lo) & (flat < lo + n)
        store = torch.where(own[:, None], rows[r], store)
        if st_scale is not None:
            st_scale = torch.where(own, sc.view(ws, -1)[r], st_scale)
    slot = torch.arange(flat.numel(), dtype=torch.int64, device=flat.device)
    cand = torch.where(flat == PAD_ID, flat, slot).view(nq, R)
    pi, ps, pm = rs.diversify(s, cand, store.contiguous(), top_k, lam, row_scale=st_scale)
    pad = pi == PAD_ID
    pi = torch.where(pad, pi, flat[torch.where(pad, torch.zeros_like(pi), pi)]) if flat.numel() else pi
    return pi, ps, pm


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
                      ws: int, refine: Optional[tuple] = None):
    """:func:`search_queries` over a product-quantized corpus (``runtime/pq.py``): every rank trains the same
    codebooks from the same sample of the file (no collective), encodes its own slice chunk by chunk and scans its
    codes with ``id_base`` = the slice start; the lists are padded to ``top_k``, all-gathered and merged as the exact
    ones are. A row's ADC score depends on the query, the codebooks and the row's codes only, so the result has the
    same bits for every world size. -> (scores, ids on the host; corpus rows; index_cached; the result's
    ``compression`` dict; its ``refine`` dict or None) on rank 0, None elsewhere.

    With ``refine`` (canonical form) every rank keeps the originals of its slice beside the codes
    (``runtime/refine.py``), shortlists ``candidates`` rows of its own slice and re-scores them exactly; the lists
    that are gathered hold exact scores. The shortlist is per rank slice: the result is a function of the payload
    and the world size."""
    import torch

    from agent_tpu_amd.ops import shortlist_rows
    from agent_tpu_amd.parallel.dp import all_gather_rows, split_range
    from agent_tpu_amd.parallel.dp_ops import exchange_errors, maybe_inject_fault
    from agent_tpu_amd.runtime import pq
    from agent_tpu_amd.runtime import refine as rfn
    from agent_tpu_amd.runtime import search as rs

    exc, s, i, total, cached, info, rinfo = None, None, None, 0, None, None, None
    nq, dim = int(qvecs.shape[0]), int(qvecs.shape[1])
    try:
        total, cdim = rs.corpus_shape(payload["corpus_uri"])
        if cdim != dim:
            raise ValueError(ERRORS["dim"])
        M, T, t = resolve_compression(compression, total, cdim)
        s_r, n_r = split_range(0, total, ws, rank)
        info = {"type": "pq", "subvectors": M, "train_rows": T, "train_iterations": t, "bytes_per_row": M}
        if refine is None:
            idx = pq.load_index(payload["corpus_uri"], s_r, n_r, device, M, T, t, metric == "cosine")
        else:
            idx = pq.load_index(payload["corpus_uri"], s_r, n_r, device, M, T, t, metric == "cosine", refine=refine[1:])
            rows = sum(shortlist_rows(n, refine[0] // 32) for n in (split_range(0, total, ws, r)[1] for r in range(ws)) if n)
            rinfo = {"candidates": refine[0], "vectors": refine[1], "store": refine[2], "rescored_rows": rows}
        cached = idx.cached
        maybe_inject_fault("search")
        if refine is None:
            s, i = pq.search(qvecs, idx, top_k, id_base=s_r)
        else:
            s, i, _ = rfn.search(qvecs, idx, top_k, refine[0], id_base=s_r)
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
    return s[:, :kk], i[:, :kk], total, cached, info, rinfo


def search_queries_binary(device, qvecs, payload: Dict[str, Any], top_k: int, metric: str, binary: tuple, rank: int,
                          ws: int, refine: Optional[tuple] = None):
    """:func:`search_queries` over a binary corpus (``runtime/binary.py``), run as :func:`search_queries_pq`: every rank
    derives the same threshold from the same sample of the file (no collective), packs its own slice chunk by chunk
    and scans its bits with ``id_base`` = the slice start; the lists are padded to ``top_k``, all-gathered and merged
    as the exact ones are. A row's score is an integer that depends on the query's and the row's bits only, so the
    result has the same bits for every world size. With ``refine`` every rank shortlists ``candidates`` rows of its
    own slice and re-scores them exactly, as for PQ. -> (scores, ids on the host; corpus rows; index_cached; the
    result's ``compression`` dict; its ``refine`` dict or None) on rank 0, None elsewhere."""
    import torch

    from agent_tpu_amd.ops import binary_ok, shortlist_rows
    from agent_tpu_amd.parallel.dp import all_gather_rows, split_range
    from agent_tpu_amd.parallel.dp_ops import exchange_errors, maybe_inject_fault
    from agent_tpu_amd.runtime import binary as rb
    from agent_tpu_amd.runtime import search as rs

    exc, s, i, total, cached, info, rinfo = None, None, None, 0, None, None, None
    nq, dim = int(qvecs.shape[0]), int(qvecs.shape[1])
    try:
        total, cdim = rs.corpus_shape(payload["corpus_uri"])
        if cdim != dim:
            raise ValueError(ERRORS["dim"])
        if not binary_ok(cdim):
            raise ValueError(BINARY_ERRORS["binary_dim"])
        s_r, n_r = split_range(0, total, ws, rank)
        info = {"type": "binary", "threshold": binary[0], "bits": cdim, "bytes_per_row": cdim // 8}
        idx = rb.load_index(payload["corpus_uri"], s_r, n_r, device, binary[0], metric == "cosine",
                            refine=None if refine is None else refine[1:])
        if refine is not None:
            rows = sum(shortlist_rows(n, refine[0] // 32) for n in (split_range(0, total, ws, r)[1] for r in range(ws)) if n)
            rinfo = {"candidates": refine[0], "vectors": refine[1], "store": refine[2], "rescored_rows": rows}
        cached = idx.cached
        maybe_inject_fault("search")
        if refine is None:
            s, i = rb.search(qvecs, idx, top_k, id_base=s_r)
        else:
            s, i, _ = rb.search_refined(qvecs, idx, top_k, refine[0], id_base=s_r)
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
    return s[:, :kk], i[:, :kk], total, cached, info, rinfo


def search_queries_ivfpq(device, qvecs, payload: Dict[str, Any], top_k: int, ivfpq: tuple, rank: int, ws: int):
    """:func:`search_queries` through an IVF-PQ index (``runtime/ivfpq.py``), run as :func:`search_queries_pq`: every
    rank trains the same centroids and codebooks from the same sample of the file (no collective), encodes its own
    slice chunk by chunk and scans the probed clusters of its slice with ``id_base`` = the slice start; the lists,
    already padded to ``top_k``, are all-gathered and merged. A row's score depends on the query, the centroids, the
    codebooks and the row's codes only, and the union of the ranks' probed rows is the probed clusters of the whole
    corpus, so the result has the same bits for every world size. -> (scores, ids on the host, padded to ``top_k``;
    corpus rows; index_cached; the result's ``index`` dict) on rank 0, None elsewhere."""
    from agent_tpu_amd.parallel.dp import all_gather_rows, split_range
    from agent_tpu_amd.parallel.dp_ops import exchange_errors, maybe_inject_fault
    from agent_tpu_amd.runtime import ivfpq as rt
    from agent_tpu_amd.runtime import search as rs

    exc, s, i, total, cached, info = None, None, None, 0, None, None
    nq, dim = int(qvecs.shape[0]), int(qvecs.shape[1])
    try:
        total, cdim = rs.corpus_shape(payload["corpus_uri"])
        if cdim != dim:
            raise ValueError(ERRORS["dim"])
        clusters, nprobe, M, T, t = resolve_ivfpq(ivfpq, total, cdim)
        s_r, n_r = split_range(0, total, ws, rank)
        idx = rt.load_index(payload["corpus_uri"], s_r, n_r, device, clusters, M, T, t)
        cached = idx.cached
        info = {"type": "ivfpq", "clusters": clusters, "nprobe": nprobe, "subvectors": M, "train_rows": T,
                "train_iterations": t, "converged": idx.converged, "bytes_per_row": M + 4}
        maybe_inject_fault("search")
        s, i, _ = rt.search(qvecs, idx, top_k, nprobe, id_base=s_r)
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
    return s, i, total, cached, info


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
           compression_info: Optional[Dict[str, Any]] = None, refine_info: Optional[Dict[str, Any]] = None,
           mmr=None) -> Dict[str, Any]:
    """One job's result from its rows of the merged lists (rank 0): the first ``top_k`` entries (with
    a total order a prefix of the top-K is the top-k), then the ``min_score`` cut on the host.
    ``filter_rows``: the corpus rows that passed the job's filter (None: no filter). ``index_info``: the
    ``index`` key of a job with an index (None: no index); its lists end where the padding begins. ``mmr``: the
    picks' MMR values of a job with ``diversify`` (None: none); its lists are in pick order, and a prefix of the
    greedy picks is the shorter job's picks."""
    opt = options(payload)
    kk = min(top_k, total if filter_rows is None else filter_rows)
    ids_l, sc_l = ids[:, :kk].tolist(), scores[:, :kk].tolist()
    mmr_l = mmr[:, :kk].tolist() if mmr is not None else None
    if index_info is not None:  # a query whose probed clusters hold fewer than top_k rows: a shorter list
        keep = [sum(1 for x in row if x != PAD_ID) for row in ids_l]
        ids_l = [row[:m] for row, m in zip(ids_l, keep)]
        sc_l = [row[:m] for row, m in zip(sc_l, keep)]
    if opt.min_score is not None:
        keep = [[j for j, v in enumerate(row) if v >= opt.min_score] for row in sc_l]
        ids_l = [[row[j] for j in ks] for row, ks in zip(ids_l, keep)]
        sc_l = [[row[j] for j in ks] for row, ks in zip(sc_l, keep)]
        if mmr_l is not None:
            mmr_l = [[row[j] for j in ks] for row, ks in zip(mmr_l, keep)]
    n = len(ids_l)
    elapsed_ms, rate = _jobs.timing(payload, n)
    out: Dict[str, Any] = {"ok": True, "op": payload.get("_op", OP_NAME), "query_count": n, "corpus_rows": total,
                           "dim": dim, "top_k": top_k, "metric": opt.metric, "elapsed_ms": elapsed_ms,
                           "queries_per_sec": rate}
    if "depth" in payload:  # a deep search: top_k above is its list length
        out["depth"] = top_k
    if h is not None:
        out.update(model_path=h.model_path, pooling=opt.pooling)
    if ws > 1:
        out["dp_world_size"] = ws
    if cached is not None:
        out["index_cached"] = bool(cached)
    # default-path results keep their keys; a compressed corpus is resident as codes, whatever the default dtype
    codes_resident = compression_info is not None or (index_info or {}).get("type") == "ivfpq"
    if "corpus_uri" in payload and opt.corpus_dtype != "float32" and not codes_resident:
        out["corpus_dtype"] = opt.corpus_dtype
    if filter_rows is not None:
        out["filter_rows"] = int(filter_rows)
    if index_info is not None:
        out["index"] = dict(index_info)
    if compression_info is not None:
        out["compression"] = dict(compression_info)
    if refine_info is not None:
        out["refine"] = dict(refine_info)
    out.update(ids=ids_l, scores=sc_l)
    if mmr_l is not None:
        lam, R = parse_diversify(payload, opt)
        out.update(mmr_scores=mmr_l, diversify={"lambda": lam, "candidates": R})
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
    if opt.ivfpq is not None:  # likewise
        got = search_queries_ivfpq(device, qv, payload, opt.top_k, opt.ivfpq, rank, ws)
        if got is None:
            return None
        s, i, total, cached, info = got
        return result(h, s, i, payload, opt.top_k, total, int(qv.shape[1]), cached, ws, index_info=info)
    if opt.compression is not None:  # likewise
        got = search_queries_pq(device, qv, payload, opt.top_k, opt.metric, opt.compression, rank, ws, opt.refine)
        if got is None:
            return None
        s, i, total, cached, info, rinfo = got
        return result(h, s, i, payload, opt.top_k, total, int(qv.shape[1]), cached, ws, compression_info=info,
                      refine_info=rinfo)
    if opt.binary is not None:  # likewise
        got = search_queries_binary(device, qv, payload, opt.top_k, opt.metric, opt.binary, rank, ws, opt.refine)
        if got is None:
            return None
        s, i, total, cached, info, rinfo = got
        return result(h, s, i, payload, opt.top_k, total, int(qv.shape[1]), cached, ws, compression_info=info,
                      refine_info=rinfo)
    got = search_queries(h, device, qv, payload, list_length(opt), opt.metric, opt.pooling, rank, ws, opt.corpus_dtype,
                         opt.filter, opt.labels_uri, opt.diversify)
    if got is None:
        return None
    s, i, total, cached, filter_rows = got[:5]
    return result(h, s, i, payload, list_length(opt), total, int(qv.shape[1]), cached, ws, filter_rows,
                  mmr=got[5] if opt.diversify is not None else None)


def search_batch(payloads: List[Dict[str, Any]], rank: int, ws: int) -> Optional[List[Any]]:
    """The ``queries`` + ``corpus_uri`` jobs of one lease that share (model, pooling, metric, corpus,
    corpus_dtype, canonical filter and its label file, canonical index, canonical compression) as one engine
    call (every rank calls it): one embed of the concatenated queries, one search at the
    group's largest ``top_k``; each job takes the first ``top_k`` entries of its own rows. A ``diversify`` group
    (equal canonical ``(lambda, candidates)``) selects once at its largest ``top_k``: a prefix of the greedy picks is
    the shorter job's picks."""
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
        mmr = None
        h, device = _handle_and_device(first)
        K = max(list_length(opt) for _, opt, _ in jobs)  # a depth group shares its depth
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
                got = None if got is None else got[:4] + (None, got[4], None, None)
            elif key.ivfpq is not None:  # the group shares the canonical ivfpq, nprobe included
                got = search_queries_ivfpq(device, qv, first, K, key.ivfpq, rank, ws)
                got = None if got is None else got[:4] + (None, got[4], None, None)
            elif key.compression is not None:  # the group shares the canonical compression and the canonical refine
                got = search_queries_pq(device, qv, first, K, key.metric, key.compression, rank, ws, key.refine)
                got = None if got is None else got[:4] + (None, None, got[4], got[5])
            elif key.binary is not None:  # the group shares the threshold and the canonical refine
                got = search_queries_binary(device, qv, first, K, key.metric, key.binary, rank, ws, key.refine)
                got = None if got is None else got[:4] + (None, None, got[4], got[5])
            else:
                got = search_queries(h, device, qv, first, K, key.metric, key.pooling, rank, ws, key.corpus_dtype,
                                     key.filter, key.labels_uri, key.diversify)
                if got is not None and key.diversify is not None:  # the group's picks at its largest top_k
                    mmr, got = got[5], got[:5]
                got = None if got is None else got + (None, None, None)
        except Exception as exc:  # a bad corpus is bad for every job of the group
            for n, _, _ in jobs:
                out[n] = ("err", exc)
            return out if rank == 0 else None
        if got is not None:
            s, i, total, cached, filter_rows, info, cinfo, rinfo = got
            pos = 0
            for n, opt, ts in jobs:
                out[n] = ("ok", result(h, s[pos:pos + len(ts)], i[pos:pos + len(ts)], payloads[n], list_length(opt), total,
                                       int(qv.shape[1]), cached, ws, filter_rows, info, cinfo, rinfo,
                                       None if mmr is None else mmr[pos:pos + len(ts)]))
                pos += len(ts)
    return out if rank == 0 else None


@register_batch_op("map_search")
def map_search_batch(payloads: List[Dict[str, Any]]) -> List[Any]:
    """Batch handler: ``queries`` + ``corpus_uri`` jobs that share (model_path, pooling, metric,
    corpus_uri, corpus_dtype, with a ``filter`` its canonical form and label file, and with an ``index`` its
    canonical (clusters, train_iterations) and nprobe, with a ``compression`` its canonical tuple, and with a ``depth``
    the depth) go to the device together; ``corpus_texts`` jobs, ``query_vectors`` jobs and malformed payloads take the
    single-job path."""

    def key(p):
        if "queries" not in p or "corpus_uri" not in p:
            raise KeyError("queries")  # not batchable
        opt = check_payload(p)
        group = p.get("model_path"), opt.pooling, opt.metric, p["corpus_uri"], opt.corpus_dtype
        if opt.index is not None:  # (clusters, train_iterations) name the index; jobs that differ in nprobe probe
            clusters, nprobe, t = opt.index  # other rows per query, so they stay separate groups
            return group + ("ivf", clusters, t, nprobe)
        if opt.ivfpq is not None:  # (clusters, subvectors, train_rows, train_iterations) name the index; nprobe
            clusters, nprobe, M, T, t = opt.ivfpq  # separates groups, as for IVF
            return group + ("ivfpq", clusters, M, T, t, nprobe)
        if opt.compression is not None:  # the canonical tuple names the codebooks and the codes; jobs that differ in
            if opt.refine is not None:  # refine re-score other shortlists from other stores: separate groups
                return group + ("pq",) + opt.compression + ("refine",) + opt.refine
            return group + ("pq",) + opt.compression
        if opt.binary is not None:  # the threshold names the bits; binary jobs never group with PQ jobs
            return group + ("binary",) + opt.binary + ((("refine",) + opt.refine) if opt.refine is not None else ())
        if opt.depth is not None:  # jobs of different depths do not share a search
            return group + (("depth", opt.depth),)
        if opt.diversify is not None:  # the canonical (lambda, candidates): one selection at the group's largest top_k
            group = group + (("diversify",) + opt.diversify,)
        return group if opt.filter is None else group + (opt.filter, opt.labels_uri)  # equal filters share a search

    return _jobs.lease_batch(payloads, OP_NAME, "map_search_batch", key, run)


def run(payload: Dict[str, Any], ctx: Dict[str, Any] = None) -> Dict[str, Any]:
    return _jobs.run_single(payload, OP_NAME, OP_NAME, check_payload)


@register_op("map_search")
def map_search(payload: Dict[str, Any], ctx: Dict[str, Any] = None) -> Dict[str, Any]:
    return run(payload, ctx)
