"""``map_answer`` — extractive question answering over (question, passage) pairs on MI355X.

The third stage of a retrieval stack, the *reader*: the model (``BertForQuestionAnswering``) reads each
question together with each of its passages as ``[CLS] question [SEP] passage [SEP]`` (the pair rows of
``map_rerank``), a span head gives every token a start and an end logit, and the best answer spans of
each passage, then of each question over all of its passages, are selected on the GPU
(``agent_tpu_amd/ops/span.py``, ``group_topk``). The host maps the returned token spans to character
offsets of the passage. With ``doc_stride`` a passage longer than its row is read in overlapping windows
("atpu-window v1") instead of being cut at the row's end. Two payload forms (see map_answer.CONTRACT.md):

1. one question: ``{"question": "...", "passages": ["...", ...]}``;
2. several: ``{"questions": ["...", ...], "passages": [["...", ...], ...]}``, one list per question.

Under ``torchrun`` the pairs are split over every GPU of the node, the per-rank span rows are
all-gathered and rank 0 ranks them. Errors are ``ValueError`` s with the fixed messages of
:data:`ERRORS`; there is no fallback stub.
"""
from __future__ import annotations

import math
from typing import Any, Dict, List, NamedTuple, Optional, Tuple

from . import _jobs, register_batch_op, register_op
from ._common import is_int

OP_NAME = "map_answer"
MAX_TOP_K = 32

#: every input error of the op (each listed in map_answer.CONTRACT.md)
ERRORS: Dict[str, str] = {
    "missing": 'payload missing required keys: "question" (or "questions") and "passages"',
    "both": 'payload must have "question" or "questions", not both',
    "question": "payload.question must be a string",
    "questions": "payload.questions must be a list of strings",
    "passages": "payload.passages must be a list of strings",
    "passage_lists": "payload.passages must be a list of lists of strings, one list per question",
    "top_k": "payload.top_k must be an integer in [1, 32]",
    "max_answer_tokens": "payload.max_answer_tokens must be an integer in [1, seq_len - 3]",
    "max_query_tokens": "payload.max_query_tokens must be an integer in [1, seq_len - 4]",
    "min_score_over_null": "payload.min_score_over_null must be a number",
    "return_null_scores": "payload.return_null_scores must be a boolean",
    "qa": "model has no QA head",
}

#: the input errors of the ``doc_stride`` key (also in map_answer.CONTRACT.md); kept apart from
#: :data:`ERRORS`, whose keys are the errors of a payload without it
WINDOW_ERRORS: Dict[str, str] = {
    "doc_stride": "payload.doc_stride must be an integer in [1, seq_len - 3]",
}


class Options(NamedTuple):
    top_k: int
    max_answer_tokens: int
    max_query_tokens: Optional[int]  # None: the engine's default, min(32, (seq_len - 3) // 2)
    min_score_over_null: Optional[float]
    return_null_scores: bool
    doc_stride: Optional[int] = None  # None: one row per pair, the passage cut at the row's end


def options(payload: Dict[str, Any]) -> Options:
    """The validated optional keys; raises the op's ``ValueError`` s before any device work. The bounds
    that depend on the model (``max_answer_tokens``, ``max_query_tokens``) are checked by
    :func:`check_model` once it is loaded."""
    top_k = payload.get("top_k", 3)
    if not is_int(top_k) or not 1 <= top_k <= MAX_TOP_K:
        raise ValueError(ERRORS["top_k"])
    ma = payload.get("max_answer_tokens", 30)
    if not is_int(ma) or ma < 1:
        raise ValueError(ERRORS["max_answer_tokens"])
    mq = payload.get("max_query_tokens")
    if mq is not None and (not is_int(mq) or mq < 1):
        raise ValueError(ERRORS["max_query_tokens"])
    margin = _jobs.number_or_none(payload, "min_score_over_null", ERRORS["min_score_over_null"])
    nulls = payload.get("return_null_scores", False)
    if not isinstance(nulls, bool):
        raise ValueError(ERRORS["return_null_scores"])
    stride = payload.get("doc_stride")
    if stride is not None and (not is_int(stride) or stride < 1):
        raise ValueError(WINDOW_ERRORS["doc_stride"])
    return Options(top_k, ma, mq, margin, nulls, stride)


def check_pairs(payload: Dict[str, Any]) -> Tuple[List[str], List[List[str]]]:
    """``(questions, passages per question)`` of either payload form."""
    return _jobs.pairs_of(payload, "question", "questions", ERRORS)


def check_model(h, opt: Options) -> None:
    """The model-dependent bounds (the same handle on every rank: all raise together)."""
    if not getattr(h.spec, "qa", False):
        raise ValueError(ERRORS["qa"])
    S = h.engine.S
    if S < 5 or (opt.max_query_tokens is not None and opt.max_query_tokens > S - 4):
        raise ValueError(ERRORS["max_query_tokens"])
    if opt.max_answer_tokens > S - 3:
        raise ValueError(ERRORS["max_answer_tokens"])
    if opt.doc_stride is not None and opt.doc_stride > S - 3:
        raise ValueError(WINDOW_ERRORS["doc_stride"])


def result(h, opt: Options, questions: List[str], groups: List[List[str]], answers: List[List[Dict[str, Any]]],
           null, payload: Dict[str, Any], extra: Dict[str, Any]) -> Dict[str, Any]:
    """One job's result from the ranked ``answers`` of its questions (at least ``top_k`` each where there
    are that many, best first) and its pairs' ``null`` scores in input order (rank 0)."""
    out_answers = []
    for row in answers:
        kept = [a for a in row[:opt.top_k]
                if opt.min_score_over_null is None or a["score"] - a["null_score"] >= opt.min_score_over_null]
        # softmax over the question's returned scores, on the host in fp64
        top = max((a["score"] for a in kept), default=0.0)
        ex = [math.exp(a["score"] - top) for a in kept]
        den = math.fsum(ex)
        out_answers.append([{"passage": int(a["passage"]), "start": int(a["start"]), "end": int(a["end"]),
                             "text": a["text"], "score": float(a["score"]), "null_score": float(a["null_score"]),
                             "probability": e / den} for a, e in zip(kept, ex)])
    n = sum(len(g) for g in groups)
    elapsed_ms, rate = _jobs.timing(payload, n)
    out = {"ok": True, "op": payload.get("_op", OP_NAME), "model_path": h.model_path, "query_count": len(questions),
           "pair_count": n, "top_k": opt.top_k, "max_answer_tokens": opt.max_answer_tokens,
           "elapsed_ms": elapsed_ms, "pairs_per_sec": rate}
    out.update(extra)
    out["answers"] = out_answers
    if opt.return_null_scores:
        flat, pos, out["null_scores"] = null.tolist(), 0, []
        for ps in groups:
            out["null_scores"].append(flat[pos:pos + len(ps)])
            pos += len(ps)
    return out


def answer_batch(h, payloads: List[Dict[str, Any]], rank: int, ws: int) -> Optional[List[Any]]:
    """The jobs of one lease that share (model, max_query_tokens, max_answer_tokens, doc_stride) as one engine call
    (every rank calls it; a single job is a batch of one): their pairs concatenated, split contiguously
    over the DP ranks, the span / score / null rows all-gathered, ranked on rank 0 at the largest
    ``top_k``. A prefix of a total order is the smaller top-k, both among a pair's spans and among a
    question's, so each job gets exactly its single-job result; a bad payload gets its own error entry."""

    def check(p):
        opt = options(p)
        questions, groups = check_pairs(p)
        check_model(h, opt)
        return opt, questions, groups

    out, jobs = _jobs.validated(payloads, check)
    if jobs:
        key = jobs[0][1]
        k = max(opt.top_k for _, opt, _, _ in jobs)
        questions = [q for _, _, qs, _ in jobs for q in qs]
        passages = [p for _, _, _, gs in jobs for g in gs for p in g]
        goff = _jobs.offsets([g for _, _, _, gs in jobs for g in gs])

        def compute(s_r, n_r):
            # this rank's rows of every group; a question with none of them here costs nothing
            local = [min(max(g - s_r, 0), n_r) for g in goff]
            rows = h.engine.span_pairs(questions, passages[s_r:s_r + n_r], local, k, key.max_answer_tokens,
                                       key.max_query_tokens, key.doc_stride)
            if key.doc_stride is not None:  # every pair's window count travels with its rows
                rows = tuple(rows) + (h.engine.window_counts,)
            return rows

        span, score, null, *wcount = _jobs.shard_and_gather("answer", len(passages), rank, ws, compute)
        if rank == 0:
            # windowed spans are tokens of the whole passage (cut at max_row_bytes), not of one row
            res = h.engine.rank_spans(span, score, null, passages, goff, k,
                                      token_cap=None if key.doc_stride is None else h.engine.max_row_bytes)
            wcount = wcount[0].tolist() if wcount else None
            q0 = 0
            for i, opt, qs, gs in jobs:
                try:
                    extra: Dict[str, Any] = {"dp_world_size": ws} if ws > 1 else {}
                    if wcount is not None:
                        extra.update(doc_stride=opt.doc_stride,
                                     window_count=int(sum(wcount[goff[q0]:goff[q0 + len(qs)]])))
                    out[i] = ("ok", result(h, opt, qs, gs, res.answers[q0:q0 + len(qs)],
                                           res.null[goff[q0]:goff[q0 + len(qs)]], payloads[i], extra))
                except Exception as e:
                    out[i] = ("err", e)
                q0 += len(qs)
    return out if rank == 0 else None


@register_batch_op("map_answer")
def map_answer_batch(payloads: List[Dict[str, Any]]) -> List[Any]:
    """Batch handler: jobs that share (model_path, max_query_tokens, max_answer_tokens, doc_stride) go to the device
    together; malformed payloads take the single-job path and fail alone."""

    def key(p):
        opt = options(p)
        check_pairs(p)
        return p.get("model_path"), opt.max_query_tokens, opt.max_answer_tokens, opt.doc_stride

    return _jobs.lease_batch(payloads, OP_NAME, "map_answer_batch", key, run)


def run(payload: Dict[str, Any], ctx: Dict[str, Any] = None) -> Dict[str, Any]:
    return _jobs.run_single(payload, OP_NAME, OP_NAME, lambda p: (options(p), check_pairs(p)))


@register_op("map_answer")
def map_answer(payload: Dict[str, Any], ctx: Dict[str, Any] = None) -> Dict[str, Any]:
    return run(payload, ctx)
