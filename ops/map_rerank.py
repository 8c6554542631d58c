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

from typing import Any, Dict, List, NamedTuple, Optional, Tuple

from . import _jobs, register_batch_op, register_op
from ._common import is_int

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


def options(payload: Dict[str, Any]) -> Options:
    """The validated optional keys; raises the op's ``ValueError`` s before any device work. The
    bounds that depend on the model (``label``, ``max_query_tokens``) are checked by
    :func:`check_model` once it is loaded."""
    top_k = payload.get("top_k", 10)
    if not is_int(top_k) or not 1 <= top_k <= MAX_TOP_K:
        raise ValueError(ERRORS["top_k"])
    mq = payload.get("max_query_tokens")
    if mq is not None and (not is_int(mq) or mq < 1):
        raise ValueError(ERRORS["max_query_tokens"])
    label = payload.get("label", 0)
    if not is_int(label) or label < 0:
        raise ValueError(ERRORS["label"])
    activation = payload.get("activation", "none")
    if activation not in ("none", "sigmoid"):
        raise ValueError(ERRORS["activation"])
    return_scores = payload.get("return_scores", False)
    if not isinstance(return_scores, bool):
        raise ValueError(ERRORS["return_scores"])
    min_score = _jobs.number_or_none(payload, "min_score", ERRORS["min_score"])
    return Options(top_k, mq, label, activation, return_scores, min_score)


def check_pairs(payload: Dict[str, Any]) -> Tuple[List[str], List[List[str]]]:
    """``(queries, passages per query)`` of either payload form."""
    return _jobs.pairs_of(payload, "query", "queries", ERRORS)


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
    elapsed_ms, rate = _jobs.timing(payload, n)
    out = {"ok": True, "op": payload.get("_op", OP_NAME), "model_path": h.model_path, "query_count": len(queries),
           "pair_count": n, "top_k": opt.top_k, "label": opt.label, "activation": opt.activation,
           "elapsed_ms": elapsed_ms, "pairs_per_sec": rate}
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

    def check(p):
        opt = options(p)
        queries, groups = check_pairs(p)
        check_model(h, opt)
        return opt, queries, groups

    out, jobs = _jobs.validated(payloads, check)
    if jobs:
        key = jobs[0][1]
        queries = [q for _, _, qs, _ in jobs for q in qs]
        passages = [p for _, _, _, gs in jobs for g in gs for p in g]
        goff = _jobs.offsets([g for _, _, _, gs in jobs for g in gs])

        def compute(s_r, n_r):
            # this rank's rows of every group; a query with none of them here costs nothing
            local = [min(max(g - s_r, 0), n_r) for g in goff]
            return (h.engine.score_pairs(queries, passages[s_r:s_r + n_r], local, key.max_query_tokens, key.label),)

        (scores,) = _jobs.shard_and_gather("rerank", len(passages), rank, ws, compute)
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

    def key(p):
        opt = options(p)
        check_pairs(p)
        return p.get("model_path"), opt.max_query_tokens, opt.label

    return _jobs.lease_batch(payloads, OP_NAME, "map_rerank_batch", key, run)


def run(payload: Dict[str, Any], ctx: Dict[str, Any] = None) -> Dict[str, Any]:
    return _jobs.run_single(payload, OP_NAME, OP_NAME, lambda p: (options(p), check_pairs(p)))


@register_op("map_rerank")
def map_rerank(payload: Dict[str, Any], ctx: Dict[str, Any] = None) -> Dict[str, Any]:
    return run(payload, ctx)
