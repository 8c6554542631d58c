"""``map_search`` — top-k similarity search over ``map_embed`` vectors on MI355X.

"Which corpus rows are nearest to this text?": the queries (texts embedded by the model, or
vectors given as numbers) are scored against a corpus (an ``.npy`` of ``map_embed``
``output: "npy"``, kept resident on the device, or texts embedded on the fly) by
``agent_tpu_amd/ops/search.py``: an exact fp32 similarity GEMM whose score matrix is never written,
with the top-k taken in its epilogue (see map_search.CONTRACT.md).

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


class Options(NamedTuple):
    top_k: int
    metric: str
    pooling: str
    min_score: Optional[float]
    corpus_dtype: str = "float32"  # residency of a corpus_uri corpus on the device


def _number(x: Any) -> bool:
    return isinstance(x, (int, float)) and not isinstance(x, bool) and math.isfinite(x)


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
    return opt


def _texts(rows: List[Any]) -> List[str]:
    return ["" if t is None else str(t) for t in rows]


def search_queries(h, device, qvecs, payload: Dict[str, Any], top_k: int, metric: str, pooling: str,
                   rank: int, ws: int, corpus_dtype: str = "float32"):
    """Every rank: this rank's slice of the corpus (resident as ``corpus_dtype`` in the ``corpus_uri``
    form) searched for all ``qvecs [nq, dim]`` (host or device fp32, already normalised for
    cosine), the per-rank lists padded to ``top_k``,
    all-gathered and merged. -> (scores ``[nq, kk]``, ids ``[nq, kk]`` on the host, corpus rows,
    index_cached or None) on rank 0, None elsewhere. Local errors are exchanged before the
    collective, so a bad corpus fails every rank together with the single-process message."""
    import torch

    from agent_tpu_amd.parallel.dp import all_gather_rows, split_range
    from agent_tpu_amd.parallel.dp_ops import exchange_errors, maybe_inject_fault
    from agent_tpu_amd.runtime import search as rs

    cosine = metric == "cosine"
    exc, s, i, total, cached, scale = None, None, None, 0, None, None
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
        s, i = rs.search(qvecs, vec, top_k, id_base=s_r, row_scale=scale)
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
    if ws > 1:  # [ws * nq, top_k] in rank order -> every query's ws lists side by side -> merged
        s = s.view(ws, nq, top_k).permute(1, 0, 2).reshape(nq, ws * top_k)
        i = i.view(ws, nq, top_k).permute(1, 0, 2).reshape(nq, ws * top_k)
        s, i = rs.merge_topk(s, i, top_k)
    kk = min(top_k, total)
    return s[:, :kk], i[:, :kk], total, cached


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
           ws: int) -> Dict[str, Any]:
    """One job's result from its rows of the merged lists (rank 0): the first ``top_k`` entries (with
    a total order a prefix of the top-K is the top-k), then the ``min_score`` cut on the host."""
    opt = options(payload)
    kk = min(top_k, total)
    ids_l, sc_l = ids[:, :kk].tolist(), scores[:, :kk].tolist()
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
    if "corpus_uri" in payload and opt.corpus_dtype != "float32":  # default-path results keep their keys
        out["corpus_dtype"] = opt.corpus_dtype
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
    got = search_queries(h, device, qv, payload, opt.top_k, opt.metric, opt.pooling, rank, ws, opt.corpus_dtype)
    if got is None:
        return None
    s, i, total, cached = got
    return result(h, s, i, payload, opt.top_k, total, int(qv.shape[1]), cached, ws)


def search_batch(payloads: List[Dict[str, Any]], rank: int, ws: int) -> Optional[List[Any]]:
    """The ``queries`` + ``corpus_uri`` jobs of one lease that share (model, pooling, metric, corpus,
    corpus_dtype) as one engine call (every rank calls it): one embed of the concatenated queries,
    one search at the
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
            got = search_queries(h, device, qv, first, K, key.metric, key.pooling, rank, ws, key.corpus_dtype)
        except Exception as exc:  # a bad corpus is bad for every job of the group
            for n, _, _ in jobs:
                out[n] = ("err", exc)
            return out if rank == 0 else None
        if got is not None:
            s, i, total, cached = got
            pos = 0
            for n, opt, ts in jobs:
                out[n] = ("ok", result(h, s[pos:pos + len(ts)], i[pos:pos + len(ts)], payloads[n], opt.top_k, total,
                                       int(qv.shape[1]), cached, ws))
                pos += len(ts)
    return out if rank == 0 else None


@register_batch_op("map_search")
def map_search_batch(payloads: List[Dict[str, Any]]) -> List[Any]:
    """Batch handler: ``queries`` + ``corpus_uri`` jobs that share (model_path, pooling, metric,
    corpus_uri, corpus_dtype) go to the device together; ``corpus_texts`` jobs, ``query_vectors`` jobs
    and malformed
    payloads take the single-job path."""

    def key(p):
        if "queries" not in p or "corpus_uri" not in p:
            raise KeyError("queries")  # not batchable
        opt = check_payload(p)
        return p.get("model_path"), opt.pooling, opt.metric, p["corpus_uri"], opt.corpus_dtype

    return _jobs.lease_batch(payloads, OP_NAME, "map_search_batch", key, run)


def run(payload: Dict[str, Any], ctx: Dict[str, Any] = None) -> Dict[str, Any]:
    return _jobs.run_single(payload, OP_NAME, OP_NAME, check_payload)


@register_op("map_search")
def map_search(payload: Dict[str, Any], ctx: Dict[str, Any] = None) -> Dict[str, Any]:
    return run(payload, ctx)
