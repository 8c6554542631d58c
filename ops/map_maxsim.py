"""``map_maxsim`` — late-interaction (ColBERT) scoring of queries against passages on MI355X.

The stage between ``map_embed`` + ``map_search`` (one vector per text) and ``map_rerank`` (one encoder row
per pair): the encoder reads every query and every passage once, alone, and keeps one unit vector per
token; a pair's score is the sum over the query's tokens of the best dot product with any passage token
(``agent_tpu_amd/ops/maxsim.py``). Every query's candidates are then ranked on the device (score
descending, index ascending). Three payload forms (see map_maxsim.CONTRACT.md):

1. one query: ``{"query": "...", "passages": ["...", ...]}``;
2. several: ``{"queries": ["...", ...], "passages": [["...", ...], ...]}``, one list per query;
3. shared: ``{"queries": ["...", ...], "shared_passages": ["...", ...]}``, every query against every passage.

Two more forms work on a resident token-vector index (``agent_tpu_amd/runtime/maxsim_index.py``), so that the
passages go through the encoder once and a query call encodes only the queries:

4. build: ``{"passages": ["...", ...], "index_out": {"uri": path, "dtype": "float16"}}`` writes the index;
5. index: ``{"queries": [...], "index_uri": path}`` ranks every query against the whole index, or with
   ``"candidates": [[id, ...], ...]`` against its own list of passage ids.

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


#: those of the index forms (also in the contract); ``ERRORS`` keeps exactly its keys
INDEX_ERRORS: Dict[str, str] = {
    "index_out": ('payload.index_out must be {"uri": a local path, "dtype": "float16" or "float32"} beside '
                  '"passages": a list of strings, without a query or an index_uri'),
    "index_forms": 'payload.index_uri cannot be combined with "passages" or "shared_passages"',
    "index_query": 'payload.index_uri needs "query": a string, or "queries": a list of strings',
    "candidates": "payload.candidates must be a list of lists of integers, one list per query",
    "candidates_range": "payload.candidates ids must lie in [0, passage count of the index)",
    "candidates_repeat": "payload.candidates must not repeat an id within a query",
    "index_scores": "payload.return_scores needs payload.candidates when an index is queried",
    "index_file": "index_uri must be a local 2-D float32 or float16 .npy file of token vectors",
    "offsets_file": "index offsets must be a local 1-D int64 .npy file next to index_uri (<name>.offsets.npy), "
                    "starting at 0, strictly increasing and ending at the token count",
    "index_nonfinite": "index holds non-finite values",
    "index_dim": "index width is not the model's token-vector width",
    "index_too_large": "index slice exceeds SEARCH_INDEX_MAX_GB",
}
INDEX_DTYPES = ("float16", "float32")
PAD_ID = 2 ** 62  # id of the (-inf) padding of a rank's list that is shorter than top_k (merge_topk's)


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
    """``("pairs", queries, passages per query)``, ``("shared", queries, passages)``, ``("build", [], (passages,
    uri, dtype))`` or ``("index", queries, (uri, candidates or None))``."""
    if "index_out" in payload:
        return _check_build(payload)
    if "index_uri" in payload:
        return _check_index(payload)
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


def _check_build(payload: Dict[str, Any]) -> Tuple[str, List[str], Any]:
    spec, passages = payload["index_out"], payload.get("passages")
    if (not isinstance(spec, dict) or set(spec) - {"uri", "dtype"} or not isinstance(spec.get("uri"), str)
            or not spec["uri"] or ("://" in spec["uri"] and not spec["uri"].startswith("file://"))
            or spec.get("dtype", "float16") not in INDEX_DTYPES
            or any(k in payload for k in ("query", "queries", "shared_passages", "index_uri", "candidates"))
            or not isinstance(passages, list) or not all(isinstance(p, str) for p in passages)):
        raise ValueError(INDEX_ERRORS["index_out"])
    return "build", [], (list(passages), spec["uri"], spec.get("dtype", "float16"))


def _check_index(payload: Dict[str, Any]) -> Tuple[str, List[str], Any]:
    if "passages" in payload or "shared_passages" in payload:
        raise ValueError(INDEX_ERRORS["index_forms"])
    if "query" in payload and "queries" in payload:
        raise ValueError(ERRORS["both"])
    if "query" in payload:
        if not isinstance(payload["query"], str):
            raise ValueError(ERRORS["query"])
        queries = [payload["query"]]
    elif "queries" in payload:
        queries = payload["queries"]
        if not isinstance(queries, list) or not all(isinstance(q, str) for q in queries):
            raise ValueError(ERRORS["queries"])
    else:
        raise ValueError(INDEX_ERRORS["index_query"])
    cand = payload.get("candidates")
    if cand is None:
        if payload.get("return_scores", False):
            raise ValueError(INDEX_ERRORS["index_scores"])
        return "index", list(queries), (payload["index_uri"], None)
    if (not isinstance(cand, list) or len(cand) != len(queries)
            or not all(isinstance(c, list) and all(is_int(i) for i in c) for c in cand)):
        raise ValueError(INDEX_ERRORS["candidates"])
    if any(len(set(c)) != len(c) for c in cand):
        raise ValueError(INDEX_ERRORS["candidates_repeat"])
    return "index", list(queries), (payload["index_uri"], [list(c) for c in cand])


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


def _build_job(h, job, payload, rank: int, ws: int):
    """One build job: the passages split contiguously over the DP ranks, the packed rows all-gathered in rank
    order and then the lengths; rank 0 writes both files."""
    from agent_tpu_amd.parallel.dp import all_gather_rows
    from agent_tpu_amd.runtime import maxsim_index as mi

    passages, uri, dtype = job[4]
    box = {}

    def compute(s_r, n_r):
        tok, box["lens"] = h.engine.maxsim_build(passages[s_r:s_r + n_r])
        return (tok,)

    (tok,) = _jobs.shard_and_gather("maxsim", len(passages), rank, ws, compute)
    (lens,) = all_gather_rows(box["lens"])
    if rank != 0:
        return None
    info = mi.write_index(uri, tok, lens, dtype)
    elapsed_ms, rate = _jobs.timing(payload, len(passages))
    out = {"ok": True, "op": payload.get("_op", OP_NAME), "model_path": h.model_path, "form": "build",
           "elapsed_ms": elapsed_ms, "passages_per_sec": rate}
    out.update(info)
    if ws > 1:
        out["dp_world_size"] = ws
    return out


def _open_index(h, uri, rank: int, ws: int):
    """This rank's contiguous share of the index's passages, resident on the engine's device."""
    from agent_tpu_amd.parallel.dp import split_range
    from agent_tpu_amd.runtime import maxsim_index as mi

    total, _, dim, _ = mi.index_shape(uri)
    if dim != h.engine.late_dim:
        raise ValueError(INDEX_ERRORS["index_dim"])
    s_r, n_r = split_range(0, total, ws, rank)
    return mi.load_index(uri, s_r, n_r, h.engine.device)


def _index_extra(index, ws: int, pairs: int, payload) -> Dict[str, Any]:
    elapsed_ms, rate = _jobs.timing(payload, pairs)
    extra = {"pair_count": pairs, "elapsed_ms": elapsed_ms, "pairs_per_sec": rate, "passage_count": index.total,
             "index_dtype": index.dtype, "index_cached": index.cached}
    if ws > 1:
        extra["dp_world_size"] = ws
    return extra


def _index_jobs(h, jobs, payloads, out, rank: int, ws: int) -> None:
    """The whole-index jobs that share an index as one engine call at the largest ``top_k``: every rank ranks
    its own slice with ``group_topk``, the per-rank lists (ids rebased to the file, padded with ``(-inf, 2^62)``)
    are all-gathered and rank 0 merges them in the same total order (``runtime.search.merge_topk``)."""
    import torch

    from agent_tpu_amd.runtime.search import merge_topk

    queries = [q for _, _, _, qs, _ in jobs for q in qs]
    k = max(opt.top_k for _, opt, _, _, _ in jobs)
    Q, box = len(queries), {}

    def compute(s_r, n_r):
        index = box["index"] = _open_index(h, jobs[0][4][0], rank, ws)
        res = h.engine.maxsim_index_rank(queries, index, None, k)
        ids = torch.where(res.idx >= 0, res.idx.to(torch.int64) + index.start, torch.full_like(res.idx, PAD_ID, dtype=torch.int64))
        val = torch.where(res.idx >= 0, res.score, torch.full_like(res.score, float("-inf")))
        return val.reshape(-1).to(h.engine.device), ids.reshape(-1).to(h.engine.device)

    val, ids = _jobs.shard_and_gather("maxsim", Q * k, rank, ws, compute)
    if rank != 0:
        return
    index = box["index"]
    lens_q = h.engine.maxsim_lens_q.cpu()
    val, ids = val.cpu().view(ws, Q, k).transpose(0, 1).reshape(Q, ws * k), ids.cpu().view(ws, Q, k).transpose(0, 1).reshape(Q, ws * k)
    val, ids = merge_topk(val, ids, k)
    idx = torch.where(ids == PAD_ID, torch.full_like(ids, -1), ids)
    q0 = 0
    for i, opt, form, qs, _ in jobs:
        try:
            n = len(qs)
            out[i] = ("ok", result(h, opt, form, qs, [[]] * n, idx[q0:q0 + n], val[q0:q0 + n], torch.empty(0),
                                   lens_q[q0:q0 + n], payloads[i], _index_extra(index, ws, n * index.total, payloads[i])))
        except Exception as e:
            out[i] = ("err", e)
        q0 += len(qs)


def _candidates_job(h, job, payload, rank: int, ws: int):
    """One candidates job: every rank fills its ``[Q, C]`` block (``-inf`` outside its slice), the blocks are
    all-gathered and combined by an element-wise maximum (exact: each candidate is in one slice); rank 0 ranks
    every query's own list. ``index`` in ``ranked`` is the passage id; ties go to the earlier list position."""
    import torch

    _, opt, form, queries, (uri, cand) = job
    Q, box = len(queries), {}
    C = max([len(c) for c in cand], default=0)

    def compute(s_r, n_r):
        index = box["index"] = _open_index(h, uri, rank, ws)
        if any(not 0 <= i < index.total for c in cand for i in c):
            raise ValueError(INDEX_ERRORS["candidates_range"])
        return (h.engine.maxsim_index_scores(queries, index, cand).reshape(-1),)

    (block,) = _jobs.shard_and_gather("maxsim", Q * C, rank, ws, compute)
    if rank != 0:
        return None
    index = box["index"]
    lens_q = h.engine.maxsim_lens_q.cpu()
    block = block.view(ws, Q, C).amax(0) if Q * C else block.view(Q, C)
    flat = torch.cat([block[q, :len(c)] for q, c in enumerate(cand)]) if Q else block.view(-1)
    res = h.engine.rank_scores(flat, _jobs.offsets(cand), opt.top_k)
    out = result(h, opt, form, queries, cand, res.idx, res.score, res.scores, lens_q, payload,
                 _index_extra(index, ws, int(flat.numel()), payload))
    for q, row in enumerate(out["ranked"]):
        for e in row:
            e["index"] = int(cand[q][e["index"]])
    return out


def maxsim_batch(h, payloads: List[Dict[str, Any]], rank: int, ws: int) -> Optional[List[Any]]:
    """The jobs of one lease that share the model (every rank calls it; a single job is a batch of one):
    the pair-form jobs as one engine call, the whole-index jobs of one index as one, the shared-form, build and
    candidates jobs one by one; a bad payload gets its own error entry."""

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
    whole: Dict[Any, list] = {}
    for j in jobs:
        if j[2] == "index" and j[4][1] is None:
            whole.setdefault(j[4][0], []).append(j)
    for group in whole.values():
        try:
            _index_jobs(h, group, payloads, out, rank, ws)
        except Exception as e:
            for j in group:
                out[j[0]] = ("err", e)
    single = {"shared": _shared_job, "build": _build_job, "index": _candidates_job}
    for j in jobs:
        if j[2] in single and not (j[2] == "index" and j[4][1] is None):
            try:
                out[j[0]] = ("ok", single[j[2]](h, j, payloads[j[0]], rank, ws))
            except Exception as e:
                out[j[0]] = ("err", e)
    return out if rank == 0 else None


@register_batch_op("map_maxsim")
def map_maxsim_batch(payloads: List[Dict[str, Any]]) -> List[Any]:
    """Batch handler: jobs that share ``model_path`` and ``index_uri`` go to the device together (the pair-form
    ones as one engine call, the whole-index ones as one); malformed payloads take the single-job path and fail
    alone."""

    def key(p):
        options(p)
        check_form(p)
        return p.get("model_path"), p.get("index_uri")

    return _jobs.lease_batch(payloads, OP_NAME, "map_maxsim_batch", key, run)


def run(payload: Dict[str, Any], ctx: Dict[str, Any] = None) -> Dict[str, Any]:
    return _jobs.run_single(payload, OP_NAME, OP_NAME, lambda p: (options(p), check_form(p)))


@register_op("map_maxsim")
def map_maxsim(payload: Dict[str, Any], ctx: Dict[str, Any] = None) -> Dict[str, Any]:
    return run(payload, ctx)
