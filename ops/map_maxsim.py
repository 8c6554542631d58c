"""``map_maxsim`` — late-interaction (ColBERT) scoring of queries against passages on MI355X.

The stage between ``map_embed`` + ``map_search`` (one vector per text) and ``map_rerank`` (one encoder row
per pair): the encoder reads every query and every passage once, alone, and keeps one unit vector per
token; a pair's score is the sum over the query's tokens of the best dot product with any passage token
(``agent_tpu_amd/ops/maxsim.py``). Every query's candidates are then ranked on the device (score
descending, index ascending). Three payload forms (see map_maxsim.CONTRACT.md):

1. one query: ``{"query": "...", "passages": ["...", ...]}``;
2. several: ``{"queries": ["...", ...], "passages": [["...", ...], ...]}``, one list per query;
3. shared: ``{"queries": ["...", ...], "shared_passages": ["...", ...]}``, every query against every passage.

Under ``torchrun`` the passages are split over every GPU of the node (every rank encodes all queries), the
per-rank scores are all-gathered and rank 0 ranks them; a score depends on its own two texts only, so the
results are bit-identical for every world size. Errors are ``ValueError`` s with the fixed messages of
:data:`ERRORS`; there is no fallback stub.
"""
from __future__ import annotations

from typing import Any, Dict, List, NamedTuple, Optional, Tuple

from . import _jobs, register_batch_op, register_op
from ._common import is_int

OP_NAME = "map_maxsim"
MAX_TOP_K = 32

#: every input error of the op (each listed in map_maxsim.CONTRACT.md)
ERRORS: Dict[str, str] = {
    "missing": 'payload missing required keys: "query" (or "queries") and "passages" (or "shared_passages")',
    "both": 'payload must have "query" or "queries", not both',
    "forms": 'payload must have "passages" or "shared_passages", not both',
    "query": "payload.query must be a string",
    "queries": "payload.queries must be a list of strings",
    "passages": "payload.passages must be a list of strings",
    "passage_lists": "payload.passages must be a list of lists of strings, one list per query",
    "shared_passages": "payload.shared_passages must be a list of strings",
    "shared_queries": 'payload.shared_passages needs "queries": a list of strings',
    "top_k": "payload.top_k must be an integer in [1, 32]",
    "return_scores": "payload.return_scores must be a boolean",
    "min_score": "payload.min_score must be a number",
    "normalize": "payload.normalize_by_query_length must be a boolean",
    "dim": "model's token vectors must have a width that is a multiple of 64 in [64, 1024]",
    "too_many": "too many queries for the token-vector buffer",
}


class Options(NamedTuple):
    top_k: int
    return_scores: bool
    min_score: Optional[float]
    normalize: bool


def options(payload: Dict[str, Any]) -> Options:
    """The validated optional keys; raises the op's ``ValueError`` s before any device work."""
    top_k = payload.get("top_k", 10)
    if not is_int(top_k) or not 1 <= top_k <= MAX_TOP_K:
        raise ValueError(ERRORS["top_k"])
    return_scores = payload.get("return_scores", False)
    if not isinstance(return_scores, bool):
        raise ValueError(ERRORS["return_scores"])
    min_score = _jobs.number_or_none(payload, "min_score", ERRORS["min_score"])
    normalize = payload.get("normalize_by_query_length", False)
    if not isinstance(normalize, bool):
        raise ValueError(ERRORS["normalize"])
    return Options(top_k, return_scores, min_score, normalize)


def check_form(payload: Dict[str, Any]) -> Tuple[str, List[str], Any]:
    """``("pairs", queries, passages per query)`` or ``("shared", queries, passages)``."""
    if "shared_passages" not in payload:
        return ("pairs",) + _jobs.pairs_of(payload, "query", "queries", ERRORS)
    if "passages" in payload:
        raise ValueError(ERRORS["forms"])
    queries, shared = payload.get("queries"), payload["shared_passages"]
    if "query" in payload or not isinstance(queries, list) or not all(isinstance(q, str) for q in queries):
        raise ValueError(ERRORS["shared_queries"])
    if not isinstance(shared, list) or not all(isinstance(p, str) for p in shared):
        raise ValueError(ERRORS["shared_passages"])
    return "shared", list(queries), list(shared)


def check_model(h) -> None:
    """The model-dependent bound (the same handle on every rank: all raise together)."""
    from agent_tpu_amd import ops as dev_ops

    if not dev_ops.maxsim_ok(h.engine.late_dim):
        raise ValueError(ERRORS["dim"])


def result(h, opt: Options, form: str, queries: List[str], groups: List[List[str]], idx, val, raw, lens_q,
           payload: Dict[str, Any], extra: Dict[str, Any]) -> Dict[str, Any]:
    """One job's result from the host rows ``idx [Q, >= top_k]`` / ``val`` (ranked), its raw scores ``raw [P]``
    in input order and the queries' token counts ``lens_q [Q]`` (rank 0)."""
    import torch

    if opt.normalize:  # fp32, on the host, after the ranking (a positive divisor per query: the order holds)
        val = val / lens_q.to(torch.float32).view(-1, 1)
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
           "pair_count": n, "top_k": opt.top_k, "dim": int(h.engine.late_dim), "form": form,
           "elapsed_ms": elapsed_ms, "pairs_per_sec": rate}
    out.update(extra)
    out["ranked"] = ranked
    if opt.return_scores:
        pos, out["scores"] = 0, []
        for q, ps in enumerate(groups):
            s = raw[pos:pos + len(ps)]
            out["scores"].append((s / lens_q[q].to(torch.float32) if opt.normalize else s).tolist())
            pos += len(ps)
    return out


def _pairs_jobs(h, jobs, payloads, out, rank: int, ws: int) -> None:
    """The pair-form jobs as one engine call: their passages concatenated, split contiguously over the DP
    ranks with local offsets, the scores all-gathered, ranked on rank 0 at the largest ``top_k`` (a prefix
    of a total order is the smaller top-k, so each job gets exactly its single-job result)."""
    queries = [q for _, _, _, qs, _ in jobs for q in qs]
    passages = [p for _, _, _, _, gs in jobs for g in gs for p in g]
    goff = _jobs.offsets([g for _, _, _, _, gs in jobs for g in gs])

    def compute(s_r, n_r):
        local = [min(max(g - s_r, 0), n_r) for g in goff]  # this rank's rows of every group
        return (h.engine.maxsim_scores(queries, passages[s_r:s_r + n_r], local),)

    (scores,) = _jobs.shard_and_gather("maxsim", len(passages), rank, ws, compute)
    if rank != 0:
        return
    lens_q = h.engine.maxsim_lens_q.cpu()  # every rank encoded all queries
    res = h.engine.rank_scores(scores, goff, max(opt.top_k for _, opt, _, _, _ in jobs))
    q0 = 0
    for i, opt, form, qs, gs in jobs:
        try:
            raw = res.scores[goff[q0]:goff[q0 + len(qs)]]
            out[i] = ("ok", result(h, opt, form, qs, gs, res.idx[q0:q0 + len(qs)], res.score[q0:q0 + len(qs)], raw,
                                   lens_q[q0:q0 + len(qs)], payloads[i], {"dp_world_size": ws} if ws > 1 else {}))
        except Exception as e:
            out[i] = ("err", e)
        q0 += len(qs)


def _shared_job(h, job, payload, rank: int, ws: int):
    """One shared-form job: ``shared_passages`` split contiguously over the DP ranks, a rank returning its
    ``[n_r, Q]`` block (transposed, so the all-gather concatenates along rows); rank 0 transposes and ranks."""
    _, opt, form, queries, shared = job
    Q, N = len(queries), len(shared)

    def compute(s_r, n_r):
        return (h.engine.maxsim_scores(queries, shared[s_r:s_r + n_r]).t().contiguous(),)

    (block,) = _jobs.shard_and_gather("maxsim", N, rank, ws, compute)
    if rank != 0:
        return None
    lens_q = h.engine.maxsim_lens_q.cpu()
    scores = block.view(N, Q).t().contiguous().view(-1)  # [Q * N], query-major
    res = h.engine.rank_scores(scores, [q * N for q in range(Q + 1)], opt.top_k)
    return result(h, opt, form, queries, [shared] * Q, res.idx, res.score, res.scores, lens_q, payload,
                  {"dp_world_size": ws} if ws > 1 else {})


def maxsim_batch(h, payloads: List[Dict[str, Any]], rank: int, ws: int) -> Optional[List[Any]]:
    """The jobs of one lease that share the model (every rank calls it; a single job is a batch of one):
    the pair-form jobs as one engine call, the shared-form jobs one by one; a bad payload gets its own
    error entry."""

    def check(p):
        opt = options(p)
        form, queries, groups = check_form(p)
        check_model(h)
        return opt, form, queries, groups

    out, jobs = _jobs.validated(payloads, check)
    pairs = [j for j in jobs if j[2] == "pairs"]
    if pairs:
        try:
            _pairs_jobs(h, pairs, payloads, out, rank, ws)
        except Exception as e:
            for j in pairs:
                out[j[0]] = ("err", e)
    for j in jobs:
        if j[2] == "shared":
            try:
                out[j[0]] = ("ok", _shared_job(h, j, payloads[j[0]], rank, ws))
            except Exception as e:
                out[j[0]] = ("err", e)
    return out if rank == 0 else None


@register_batch_op("map_maxsim")
def map_maxsim_batch(payloads: List[Dict[str, Any]]) -> List[Any]:
    """Batch handler: jobs that share ``model_path`` go to the device together (the pair-form ones as one
    engine call); malformed payloads take the single-job path and fail alone."""

    def key(p):
        options(p)
        check_form(p)
        return p.get("model_path")

    return _jobs.lease_batch(payloads, OP_NAME, "map_maxsim_batch", key, run)


def run(payload: Dict[str, Any], ctx: Dict[str, Any] = None) -> Dict[str, Any]:
    return _jobs.run_single(payload, OP_NAME, OP_NAME, lambda p: (options(p), check_form(p)))


@register_op("map_maxsim")
def map_maxsim(payload: Dict[str, Any], ctx: Dict[str, Any] = None) -> Dict[str, Any]:
    return run(payload, ctx)
