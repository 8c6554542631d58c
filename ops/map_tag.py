"""``map_tag`` — token classification (named entities, PII spans, tags) over texts on MI355X.

The model (``BertForTokenClassification``) reads each text as ``[CLS] text [SEP]``, a linear head gives
every token a label, and the labels are grouped into entities on the GPU (``agent_tpu_amd/ops/tag.py``):
per text a few entity records come back instead of a logits tensor. The host maps the records' token
positions to character offsets of the text. Two payload forms (see map_tag.CONTRACT.md):

1. one text: ``{"text": "..."}``;
2. several: ``{"texts": ["...", ...]}``.

Under ``torchrun`` the texts are split over every GPU of the node, the per-rank records are
all-gathered and rank 0 maps them. Errors are ``ValueError`` s with the fixed messages of
:data:`ERRORS`; there is no fallback stub.
"""
from __future__ import annotations

from typing import Any, Dict, List, NamedTuple, Optional

from . import _jobs, register_batch_op, register_op
from ._common import is_int

OP_NAME = "map_tag"
MAX_ENTITIES = 512
AGGREGATIONS = ("simple", "first", "none")

#: every input error of the op (each listed in map_tag.CONTRACT.md)
ERRORS: Dict[str, str] = {
    "missing": 'payload missing required key: "text" (or "texts")',
    "both": 'payload must have "text" or "texts", not both',
    "text": "payload.text must be a string",
    "texts": "payload.texts must be a list of strings",
    "aggregation": 'payload.aggregation must be "simple", "first" or "none"',
    "max_entities": "payload.max_entities must be an integer in [1, 512]",
    "min_score": "payload.min_score must be a number",
    "tags": "model has no tag head",
    "vocab": 'aggregation "first" needs a model with a WordPiece vocabulary',
}


class Options(NamedTuple):
    aggregation: str
    max_entities: int
    min_score: Optional[float]


def options(payload: Dict[str, Any]) -> Options:
    """The validated optional keys; raises the op's ``ValueError`` s before any device work."""
    agg = payload.get("aggregation", "simple")
    if not isinstance(agg, str) or agg not in AGGREGATIONS:
        raise ValueError(ERRORS["aggregation"])
    E = payload.get("max_entities", 64)
    if not is_int(E) or not 1 <= E <= MAX_ENTITIES:
        raise ValueError(ERRORS["max_entities"])
    return Options(agg, E, _jobs.number_or_none(payload, "min_score", ERRORS["min_score"]))


def check_texts(payload: Dict[str, Any]) -> List[str]:
    """The texts of either payload form."""
    return _jobs.texts_of(payload, ERRORS)


def check_model(h, opt: Options) -> None:
    """What depends on the model (the same handle on every rank: all raise together)."""
    if not getattr(h.spec, "tags", 0):
        raise ValueError(ERRORS["tags"])
    if opt.aggregation == "first" and h.engine.vocab is None:
        raise ValueError(ERRORS["vocab"])


def result(h, opt: Options, texts: List[str], entities: List[List[Dict[str, Any]]], counts: List[int],
           payload: Dict[str, Any], extra: Dict[str, Any]) -> Dict[str, Any]:
    """One job's result from the mapped ``entities`` and true ``counts`` of its texts (rank 0)."""
    kept = [[e for e in row if opt.min_score is None or e["score"] >= opt.min_score] for row in entities]
    n = len(texts)
    elapsed_ms, rate = _jobs.timing(payload, n)
    out = {"ok": True, "op": payload.get("_op", OP_NAME), "model_path": h.model_path, "row_count": n,
           "aggregation": opt.aggregation, "max_entities": opt.max_entities,
           "elapsed_ms": elapsed_ms, "rows_per_sec": rate}
    out.update(extra)
    out["entities"] = kept
    out["entity_counts"] = [int(c) for c in counts]
    out["truncated"] = [i for i, c in enumerate(counts) if c > opt.max_entities]
    return out


def tag_batch(h, payloads: List[Dict[str, Any]], rank: int, ws: int) -> Optional[List[Any]]:
    """The jobs of one lease that share (model, aggregation, max_entities) as one engine call (every rank
    calls it; a single job is a batch of one): their texts concatenated, split contiguously over the DP
    ranks, the ent / ent_sum / count rows all-gathered and mapped on rank 0. A row's records do not
    depend on the rows it shares a batch with, so each job gets exactly its single-job result; a bad
    payload gets its own error entry."""

    def check(p):
        opt = options(p)
        texts = check_texts(p)
        check_model(h, opt)
        return opt, texts

    out, jobs = _jobs.validated(payloads, check)
    if jobs:
        key = jobs[0][1]
        texts = [t for _, _, ts in jobs for t in ts]
        ent, ent_sum, count = _jobs.shard_and_gather(
            "tag", len(texts), rank, ws,
            lambda s_r, n_r: h.engine.tag_rows(texts[s_r:s_r + n_r], key.aggregation, key.max_entities))
        if rank == 0:
            res = h.engine.map_tags(ent, ent_sum, count, texts, key.aggregation)
            r0 = 0
            for i, opt, ts in jobs:
                try:
                    out[i] = ("ok", result(h, opt, ts, res.entities[r0:r0 + len(ts)], res.counts[r0:r0 + len(ts)],
                                           payloads[i], {"dp_world_size": ws} if ws > 1 else {}))
                except Exception as e:
                    out[i] = ("err", e)
                r0 += len(ts)
    return out if rank == 0 else None


@register_batch_op("map_tag")
def map_tag_batch(payloads: List[Dict[str, Any]]) -> List[Any]:
    """Batch handler: jobs that share (model_path, aggregation, max_entities) go to the device together;
    malformed payloads take the single-job path and fail alone."""

    def key(p):
        opt = options(p)
        check_texts(p)
        return p.get("model_path"), opt.aggregation, opt.max_entities

    return _jobs.lease_batch(payloads, OP_NAME, "map_tag_batch", key, run)


def run(payload: Dict[str, Any], ctx: Dict[str, Any] = None) -> Dict[str, Any]:
    return _jobs.run_single(payload, OP_NAME, OP_NAME, lambda p: (options(p), check_texts(p)))


@register_op("map_tag")
def map_tag(payload: Dict[str, Any], ctx: Dict[str, Any] = None) -> Dict[str, Any]:
    return run(payload, ctx)
