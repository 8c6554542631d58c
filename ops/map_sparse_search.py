"""``map_sparse_search`` — top-k search of learned sparse (SPLADE) term weights on MI355X: the lexical half of
hybrid retrieval, over the vectors ``map_sparse_embed`` writes (``output: "npz"``).

The corpus is a CSR ``.npz`` (rows x vocabulary, fp32 weights); it becomes a resident inverted index
(``agent_tpu_amd/runtime/sparse_index.py``) whose scan kernel reads only the postings of a query's own terms
(``agent_tpu_amd/ops/sparse_index.py`` has the exact score definition: integer sums, so a result has the same bits in
any batch and for every world size). Two query forms (see map_sparse_search.CONTRACT.md):

1. ``queries``: texts, encoded by the MLM-head model of ``model_path`` (``engine.sparse_rows``);
2. ``query_terms``: ``[{"token_ids": [...], "weights": [...]}, ...]``; no model is loaded.

Under ``torchrun`` every rank scans its slice of the rows; the per-rank lists are all-gathered and merged on rank 0
in the total order (score descending, id ascending). Errors are ``ValueError`` s with the fixed messages of
:data:`ERRORS`; there is no fallback stub.
"""
from __future__ import annotations

import math
from typing import Any, Dict, List, NamedTuple, Optional, Tuple

from agent_tpu_amd.runtime.sparse_index import ERRORS as INDEX_ERRORS

from . import _jobs, register_batch_op, register_op
from ._common import is_int

OP_NAME = "map_sparse_search"
MAX_K = 32
MAX_QUERY_TERMS = 1024
MAX_WEIGHT = 256.0

#: every input error of the op (each listed in map_sparse_search.CONTRACT.md)
ERRORS: Dict[str, str] = dict(INDEX_ERRORS, **{
    "corpus": 'payload missing required key: "corpus_uri"',
    "missing": 'payload missing required key: "queries" (or "query_terms")',
    "both": 'payload must have "queries" or "query_terms", not both',
    "queries": "payload.queries must be a list of strings",
    "query_terms": 'payload.query_terms must be a list of {"token_ids": [int, ...], "weights": [number, ...]} '
                   "of equal lengths, at most 1024 terms each",
    "token_ids": "query token ids must be distinct non-negative integers below the corpus vocabulary",
    "weights": "query weights must be finite numbers in (0, 256]",
    "top_k": "payload.top_k must be an integer in [1, 32]",
    "max_query_terms": "payload.max_query_terms must be an integer in [1, 1024]",
    "mlm": "model has no MLM head",
    "vocab": "model vocabulary differs from the corpus vocabulary",
})


class Options(NamedTuple):
    top_k: int
    max_query_terms: int
    texts: Optional[List[str]]  # the ``queries`` form
    terms: Optional[List[Tuple[List[int], List[float]]]]  # the ``query_terms`` form


def check_payload(payload: Dict[str, Any]) -> Options:
    """The validated payload; raises the op's ``ValueError`` s before any device work."""
    if "corpus_uri" not in payload:
        raise ValueError(ERRORS["corpus"])
    if "queries" not in payload and "query_terms" not in payload:
        raise ValueError(ERRORS["missing"])
    if "queries" in payload and "query_terms" in payload:
        raise ValueError(ERRORS["both"])
    k = payload.get("top_k", 10)
    if not is_int(k) or not 1 <= k <= MAX_K:
        raise ValueError(ERRORS["top_k"])
    m = payload.get("max_query_terms", 256)
    if not is_int(m) or not 1 <= m <= MAX_QUERY_TERMS:
        raise ValueError(ERRORS["max_query_terms"])
    if "queries" in payload:
        qs = payload["queries"]
        if not isinstance(qs, list) or not all(isinstance(q, str) for q in qs):
            raise ValueError(ERRORS["queries"])
        return Options(k, m, list(qs), None)
    qt, terms = payload["query_terms"], []
    if not isinstance(qt, list):
        raise ValueError(ERRORS["query_terms"])
    for q in qt:
        ids, ws = (q.get("token_ids"), q.get("weights")) if isinstance(q, dict) else (None, None)
        if not isinstance(ids, list) or not isinstance(ws, list) or len(ids) != len(ws) or len(ids) > MAX_QUERY_TERMS:
            raise ValueError(ERRORS["query_terms"])
        if not all(is_int(t) and 0 <= t < 2 ** 31 - 1 for t in ids) or len(set(ids)) != len(ids):
            raise ValueError(ERRORS["token_ids"])
        if not all(isinstance(w, (int, float)) and not isinstance(w, bool) and math.isfinite(w)
                   and 0 < w <= MAX_WEIGHT for w in ws):
            raise ValueError(ERRORS["weights"])
        terms.append((list(ids), [float(w) for w in ws]))
    return Options(k, m, None, terms)


def _handle_and_device(payload: Dict[str, Any]):
    """The model (a collective load under DP) when the job has ``queries``, and the device."""
    from ._gpu_runtime import device_for_rank, get_gpu_handle, get_model_path

    if "queries" in payload:
        h = get_gpu_handle(get_model_path(payload.get("model_path")))
        return h, h.engine.device
    return None, device_for_rank()


def query_rows(h, device, jobs: List[Tuple[int, Options]], vocab: int):
    """The group's queries as CSR on ``device``: (q_ptr int64 ``[nq + 1]``, q_tok int32, q_w fp32)."""
    import torch

    if h is not None:
        if not getattr(h.spec, "mlm", False):
            raise ValueError(ERRORS["mlm"])
        if int(h.cfg.vocab_size) != vocab:
            raise ValueError(ERRORS["vocab"])
        texts = [t for _, opt in jobs for t in opt.texts]
        tok, _, w, _ = h.engine.sparse_rows(texts, jobs[0][1].max_query_terms)
        live = tok >= 0  # the slots past a text's terms hold -1; the order inside a row is kept
        q_ptr = torch.zeros((len(texts) + 1,), dtype=torch.int64, device=tok.device)
        q_ptr[1:] = torch.cumsum(live.sum(1), 0)
        return q_ptr, tok[live].contiguous(), w[live].contiguous()
    terms = [q for _, opt in jobs for q in opt.terms]
    if any(t >= vocab for ids, _ in terms for t in ids):
        raise ValueError(ERRORS["token_ids"])
    q_ptr = torch.tensor(_jobs.offsets([ids for ids, _ in terms]), dtype=torch.int64)
    q_tok = torch.tensor([t for ids, _ in terms for t in ids], dtype=torch.int32)
    q_w = torch.tensor([w for _, ws in terms for w in ws], dtype=torch.float32)
    if q_w.numel() and float(q_w.min()) <= 0:  # a positive double that rounds to fp32 zero
        raise ValueError(ERRORS["weights"])
    return q_ptr.to(device), q_tok.to(device), q_w.to(device)


def search_rows(h, device, jobs: List[Tuple[int, Options]], uri: Any, top_k: int, rank: int, ws: int):
    """Every rank scans its ``split_range`` slice of the rows with ``id_base`` = the slice start; the padded lists are
    all-gathered and merged on rank 0 in the total order. A row's score is an integer sum that depends on the query
    and the row only, so the result has the same bits for every world size. -> (scores, ids on the host, the index
    entry) on rank 0, None elsewhere."""
    from agent_tpu_amd.parallel.dp import all_gather_rows, split_range
    from agent_tpu_amd.parallel.dp_ops import exchange_errors, maybe_inject_fault
    from agent_tpu_amd.runtime import search as rs
    from agent_tpu_amd.runtime import sparse_index as rsi

    exc, s, i, res, nq = None, None, None, None, 0
    try:
        total, vocab = rsi.corpus_meta(uri)[:2]  # the archive's headers: nothing else is read on a cache hit
        s_r, n_r = split_range(0, total, ws, rank)
        res = rsi.load_index(uri, s_r, n_r, device)
        q_ptr, q_tok, q_w = query_rows(h, device, jobs, vocab)
        nq = int(q_ptr.numel()) - 1
        maybe_inject_fault("search")
        s, i, _ = rsi.search(res, q_ptr, q_tok, q_w, top_k, id_base=s_r)
    except Exception as e:
        exc = e
    counts = exchange_errors(exc, nq if s is not None else 0)
    s, i = all_gather_rows(s.contiguous(), i.contiguous(), counts=counts)
    if rank != 0:
        return None
    s, i = s.cpu(), i.cpu()
    if ws > 1:  # every query's ws lists side by side -> merged; the padding sorts last
        s = s.view(ws, nq, top_k).permute(1, 0, 2).reshape(nq, ws * top_k)
        i = i.view(ws, nq, top_k).permute(1, 0, 2).reshape(nq, ws * top_k)
        s, i = rs.merge_topk(s, i, top_k)
    return s, i, res


def result(h, s, i, res, opt: Options, payload: Dict[str, Any], ws: int) -> Dict[str, Any]:
    """One job's result from its rows of the group's lists (rank 0): the first ``top_k`` columns."""
    nq = int(s.shape[0])
    elapsed_ms, rate = _jobs.timing(payload, nq)
    out = {"ok": True, "op": payload.get("_op", OP_NAME), "row_count": nq, "corpus_rows": res.total,
           "vocab_size": res.vocab, "top_k": opt.top_k, "nnz": res.nnz, "index_cached": bool(res.cached),
           "elapsed_ms": elapsed_ms, "rows_per_sec": rate}
    if h is not None:
        out["model_path"] = h.model_path
    if ws > 1:
        out["dp_world_size"] = ws
    rows = []
    for sv, iv in zip(s[:, :opt.top_k].tolist(), i[:, :opt.top_k].tolist()):
        n = sum(1 for v in sv if v > float("-inf"))  # the padding is a suffix
        rows.append({"ids": iv[:n], "scores": sv[:n], "hits": n})
    out["results"] = rows
    return out


def search_batch(payloads: List[Dict[str, Any]], rank: int, ws: int) -> Optional[List[Any]]:
    """The jobs of one lease that share (model, corpus, max_query_terms, query form) as one scan at the group's
    largest ``top_k`` (every rank calls it; a single job is a batch of one). A query's list does not depend on the
    queries it shares a batch with, so each job gets exactly its single-job result; a bad payload gets its own
    error entry."""
    out, jobs = _jobs.validated(payloads, lambda p: (check_payload(p),))
    if jobs:
        first = payloads[jobs[0][0]]
        K = max(opt.top_k for _, opt in jobs)
        try:
            h, device = _handle_and_device(first)
            got = search_rows(h, device, jobs, first["corpus_uri"], K, rank, ws)
        except Exception as exc:  # a bad corpus or model is bad for every job of the group
            for n, _ in jobs:
                out[n] = ("err", exc)
            return out if rank == 0 else None
        if got is not None:
            s, i, res = got
            pos = 0
            for n, opt in jobs:
                nq = len(opt.texts if opt.texts is not None else opt.terms)
                out[n] = ("ok", result(h, s[pos:pos + nq], i[pos:pos + nq], res, opt, payloads[n], ws))
                pos += nq
    return out if rank == 0 else None


def search_one(payload: Dict[str, Any], rank: int, ws: int) -> Optional[Dict[str, Any]]:
    """One job (every rank calls it): a batch of one, its entry unwrapped."""
    res = search_batch([payload], rank, ws)
    if rank != 0:
        return None
    kind, value = res[0]
    if kind == "err":
        raise value
    return value


@register_batch_op("map_sparse_search")
def map_sparse_search_batch(payloads: List[Dict[str, Any]]) -> List[Any]:
    """Batch handler: jobs that share (model_path, corpus_uri, max_query_terms, query form) go to the device
    together; malformed payloads take the single-job path and fail alone."""

    def key(p):
        opt = check_payload(p)
        return p.get("model_path") if opt.texts is not None else None, p["corpus_uri"], opt.max_query_terms, \
            opt.texts is not None

    return _jobs.lease_batch(payloads, OP_NAME, "map_sparse_search_batch", key, run)


def run(payload: Dict[str, Any], ctx: Dict[str, Any] = None) -> Dict[str, Any]:
    return _jobs.run_single(payload, OP_NAME, OP_NAME, check_payload)


@register_op("map_sparse_search")
def map_sparse_search(payload: Dict[str, Any], ctx: Dict[str, Any] = None) -> Dict[str, Any]:
    return run(payload, ctx)
