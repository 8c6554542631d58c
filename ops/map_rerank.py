"""``map_rerank`` — cross-encoder re-ranking of (query, passage) pairs on MI355X.

The second stage of a retrieval stack: the model reads each query together with each of its
candidate passages as ``[CLS] query [SEP] passage [SEP]`` (pair rows assembled on the GPU,
``agent_tpu_amd/ops/rerank.py``) and its classifier logit is the pair's relevance score; every
query's own candidates are then ranked on the device (score descending, index ascending). Two
payload forms (see map_rerank.CONTRACT.md):

1. one query: ``{"query": "...", "passages": ["...", ...]}``;
2. several: ``{"queries": ["...", ...], "passages": [["...", ...], ...]}``, one list per query.

Under ``torchrun`` the pairs are split over every GPU of the node, the per-rank scores are
all-gathered and rank 0 ranks them. Errors are ``ValueError`` s with the fixed messages of
:data:`ERRORS`; there is no fallback stub.
"""
from __future__ import annotations

import time
from typing import Any, Dict, List, NamedTuple, Optional, Tuple

from . import register_batch_op, register_op

OP_NAME = "map_rerank"
MAX_TOP_K = 32

#: every input error of the op (each listed in map_rerank.CONTRACT.md)
ERRORS: Dict[str, str] = {
    "missing": 'payload missing required keys: "query" (or "queries") and "passages"',
    "both": 'payload must have "query" or "queries", not both',
    "query": "payload.query must be a string",
    "queries": "payload.queries must be a list of strings",
    "passages": "payload.passages must be a list of strings",
    "passage_lists": "payload.passages must be a list of lists of strings, one list per query",
    "top_k": "payload.top_k must be an integer in [1, 32]",
    "max_query_tokens": "payload.max_query_tokens must be an integer in [1, seq_len - 4]",
    "label": "payload.label must be an integer in [0, num_labels)",
    "activation": "payload.activation must be 'none' or 'sigmoid'",
    "return_scores": "payload.return_scores must be a boolean",
    "min_score": "payload.min_score must be a number",
    "head": "model has no classifier head",
}


class Options(NamedTuple):
    top_k: int
    max_query_tokens: Optional[int]  # None: the engine's default, min(32, (seq_len - 3) // 2)
    label: int
    activation: str
    return_scores: bool
    min_score: Optional[float]


def _is_int(v: Any) -> bool:
    return isinstance(v, int) and not isinstance(v, bool)


def options(payload: Dict[str, Any]) -> Options:
    """The validated optional keys; raises the op's ``ValueError`` s before any device work. The
    bounds that depend on the model (``label``, ``max_query_tokens``) are checked by
    :func:`check_model` once it is loaded."""
    top_k = payload.get("top_k", 10)
    if not _is_int(top_k) or not 1 <= top_k <= MAX_TOP_K:
        raise ValueError(ERRORS["top_k"])
    mq = payload.get("max_query_tokens")
    if mq is not None and (not _is_int(mq) or mq < 1):
        raise ValueError(ERRORS["max_query_tokens"])
    label = payload.get("label", 0)
    if not _is_int(label) or label < 0:
        raise ValueError(ERRORS["label"])
    activation = payload.get("activation", "none")
    if activation not in ("none", "sigmoid"):
        raise ValueError(ERRORS["activation"])
    return_scores = payload.get("return_scores", False)
    if not isinstance(return_scores, bool):
        raise ValueError(ERRORS["return_scores"])
    min_score = payload.get("min_score")
    if min_score is not None:
        if isinstance(min_score, bool) or not isinstance(min_score, (int, float)) or min_score != min_score:
            raise ValueError(ERRORS["min_score"])
        min_score = float(min_score)
    return Options(top_k, mq, label, activation, return_scores, min_score)


def check_pairs(payload: Dict[str, Any]) -> Tuple[List[str], List[List[str]]]:
    """``(queries, passages per query)`` of either payload form."""
    if "passages" not in payload or ("query" not in payload and "queries" not in payload):
        raise ValueError(ERRORS["missing"])
    if "query" in payload and "queries" in payload:
        raise ValueError(ERRORS["both"])
    passages = payload["passages"]
    if "query" in payload:
        if not isinstance(payload["query"], str):
            raise ValueError(ERRORS["query"])
        if not isinstance(passages, list) or not all(isinstance(p, str) for p in passages):
            raise ValueError(ERRORS["passages"])
        return [payload["query"]], [list(passages)]
    queries = payload["queries"]
    if not isinstance(queries, list) or not all(isinstance(q, str) for q in queries):
        raise ValueError(ERRORS["queries"])
    if (not isinstance(passages, list) or len(passages) != len(queries)
            or not all(isinstance(ps, list) and all(isinstance(p, str) for p in ps) for ps in passages)):
        raise ValueError(ERRORS["passage_lists"])
    return list(queries), [list(ps) for ps in passages]


def check_model(h, opt: Options) -> None:
    """The model-dependent bounds (the same handle on every rank: all raise together)."""
    if not getattr(h.spec, "head", True):
        raise ValueError(ERRORS["head"])
    if opt.label >= h.cfg.num_labels:
        raise ValueError(ERRORS["label"])
    S = h.engine.S
    if S < 5 or (opt.max_query_tokens is not None and opt.max_query_tokens > S - 4):
        raise ValueError(ERRORS["max_query_tokens"])


def result(h, opt: Options, queries: List[str], groups: List[List[str]], idx, val, raw, payload: Dict[str, Any],
           extra: Dict[str, Any]) -> Dict[str, Any]:
    """One job's result from the host rows ``idx [Q, >= top_k]`` / ``val`` (ranked, after the
    activation) and its raw scores ``raw [P]`` in input order (rank 0)."""
    ranked = []
    for q in range(len(queries)):
        row = []
        for i, s in zip(idx[q, :opt.top_k].tolist(), val[q, :opt.top_k].tolist()):
            if i < 0 or (opt.min_score is not None and s < opt.min_score):
                break  # the list is sorted: nothing after a padding entry or a score under min_score
            row.append({"index": int(i), "score": float(s)})
        ranked.append(row)
    n = int(raw.numel())
    dt = time.time() - float(payload.get("_t0", time.time()))
    out = {"ok": True, "op": payload.get("_op", OP_NAME), "model_path": h.model_path, "query_count": len(queries),
           "pair_count": n, "top_k": opt.top_k, "label": opt.label, "activation": opt.activation,
           "elapsed_ms": dt * 1000.0, "pairs_per_sec": (n / dt) if dt > 0 else None}
    out.update(extra)
    out["ranked"] = ranked
    if opt.return_scores:
        flat, pos, out["scores"] = raw.tolist(), 0, []
        for ps in groups:
            out["scores"].append(flat[pos:pos + len(ps)])
            pos += len(ps)
    return out


def rerank_batch(h, payloads: List[Dict[str, Any]], rank: int, ws: int) -> Optional[List[Any]]:
    """The jobs of one lease that share (model, max_query_tokens, label) as one engine call (every
    rank calls it; a single job is a batch of one): their pairs concatenated, split contiguously
    over the DP ranks, the scores all-gathered, ranked on rank 0 at the largest ``top_k``. A prefix
    of a total order is the smaller top-k, so each job gets exactly its single-job result; a bad
    payload gets its own error entry."""
    from agent_tpu_amd.parallel.dp import all_gather_rows, split_range
    from agent_tpu_amd.parallel.dp_ops import exchange_errors, maybe_inject_fault

    out: List[Any] = [None] * len(payloads)
    jobs = []
    for i, p in enumerate(payloads):  # same payloads on every rank: same validation outcome
        try:
            opt = options(p)
            queries, groups = check_pairs(p)
            check_model(h, opt)
            jobs.append((i, opt, queries, groups))
        except Exception as exc:
            out[i] = ("err", exc)
    if jobs:
        key = jobs[0][1]
        queries = [q for _, _, qs, _ in jobs for q in qs]
        passages = [p for _, _, _, gs in jobs for g in gs for p in g]
        goff = [0]
        for _, _, _, gs in jobs:
            for g in gs:
                goff.append(goff[-1] + len(g))
        exc, scores = None, None
        try:
            s_r, n_r = split_range(0, len(passages), ws, rank)
            maybe_inject_fault("rerank")
            # this rank's rows of every group; a query with none of them here costs nothing
            local = [min(max(g - s_r, 0), n_r) for g in goff]
            scores = h.engine.score_pairs(queries, passages[s_r:s_r + n_r], local, key.max_query_tokens, key.label)
        except Exception as e:
            exc = e
        counts = exchange_errors(exc, int(scores.shape[0]) if scores is not None else 0)
        (scores,) = all_gather_rows(scores, counts=counts)
        if rank == 0:
            k = max(opt.top_k for _, opt, _, _ in jobs)
            res = h.engine.rank_scores(scores, goff, k)
            q0 = 0
            for i, opt, qs, gs in jobs:
                try:
                    idx, val = res.idx[q0:q0 + len(qs)], res.score[q0:q0 + len(qs)]
                    if opt.activation == "sigmoid":
                        import torch

                        val = torch.where(idx >= 0, torch.sigmoid(val), val)  # fp32, after the ranking
                    raw = res.scores[goff[q0]:goff[q0 + len(qs)]]
                    out[i] = ("ok", result(h, opt, qs, gs, idx, val, raw, payloads[i],
                                           {"dp_world_size": ws} if ws > 1 else {}))
                except Exception as e:
                    out[i] = ("err", e)
                q0 += len(qs)
    return out if rank == 0 else None


@register_batch_op("map_rerank")
def map_rerank_batch(payloads: List[Dict[str, Any]]) -> List[Any]:
    """Batch handler: jobs that share (model_path, max_query_tokens, label) go to the device together;
    malformed payloads take the single-job path and fail alone."""
    from agent_tpu_amd.parallel.dp_ops import dispatch

    t0 = time.time()
    out: List[Any] = [None] * len(payloads)
    groups: Dict[Any, List[int]] = {}
    for i, p in enumerate(payloads):
        p = p or {}
        try:
            opt = options(p)
            check_pairs(p)
            groups.setdefault((p.get("model_path"), opt.max_query_tokens, opt.label), []).append(i)
        except Exception:
            try:
                out[i] = ("ok", run(p))
            except Exception as exc:
                out[i] = ("err", exc)
    for idxs in groups.values():
        descs = [dict(payloads[i], _op=OP_NAME, _t0=t0) for i in idxs]
        try:
            res = dispatch("map_rerank_batch", {"payloads": descs})
        except Exception as exc:
            res = [("err", exc)] * len(idxs)
        for i, entry in zip(idxs, res):
            out[i] = entry
    return out


def run(payload: Dict[str, Any], ctx: Dict[str, Any] = None) -> Dict[str, Any]:
    payload = payload or {}
    t0 = time.time()
    from agent_tpu_amd.parallel.dp_ops import dispatch

    options(payload)  # validated before any device work
    check_pairs(payload)
    return dispatch("map_rerank", dict(payload, _op=OP_NAME, _t0=t0))


@register_op("map_rerank")
def map_rerank(payload: Dict[str, Any], ctx: Dict[str, Any] = None) -> Dict[str, Any]:
    return run(payload, ctx)
