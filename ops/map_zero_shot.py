"""``map_zero_shot`` — zero-shot classification of texts against candidate labels on MI355X.

The labels come with the job, not with the checkpoint: an NLI model (a ``BertForSequenceClassification``
with an entailment and a contradiction class) reads each text together with one hypothesis per
candidate label, ``[CLS] text [SEP] This example is {label}. [SEP]`` (rows assembled on the GPU, the text
tokenized once per device batch however many labels it has, ``agent_tpu_amd/ops/zeroshot.py``), and the
label scores come from the entailment logits: a softmax over the text's labels, or with ``multi_label``
an entailment-vs-contradiction softmax per label. Every text's labels are scored and ranked on the
device. Two payload forms (see map_zero_shot.CONTRACT.md):

1. one text: ``{"text": "...", "candidate_labels": [...]}``;
2. several: ``{"texts": ["...", ...], "candidate_labels": [...]}``.

Under ``torchrun`` the (text, label) pairs are split over every GPU of the node, the per-rank logits are
all-gathered and rank 0 ranks them. Errors are ``ValueError`` s with the fixed messages of
:data:`ERRORS`; there is no fallback stub.
"""
from __future__ import annotations

from typing import Any, Dict, List, NamedTuple, Optional, Tuple

from . import _jobs, register_batch_op, register_op
from ._common import is_int

OP_NAME = "map_zero_shot"
MAX_LABELS = 256
DEFAULT_TEMPLATE = "This example is {}."

#: every input error of the op (each listed in map_zero_shot.CONTRACT.md)
ERRORS: Dict[str, str] = {
    "missing": 'payload missing required key: "text" (or "texts")',
    "both": 'payload must have "text" or "texts", not both',
    "text": "payload.text must be a string",
    "texts": "payload.texts must be a list of strings",
    "candidate_labels": "payload.candidate_labels must be a list of 1 to 256 non-empty strings",
    "hypothesis_template": 'payload.hypothesis_template must be a string with exactly one "{}"',
    "multi_label": "payload.multi_label must be a boolean",
    "top_k": "payload.top_k must be an integer >= 1",
    "max_hypothesis_tokens": "payload.max_hypothesis_tokens must be an integer in [1, seq_len - 4]",
    "label_ids": "payload.entailment_id and payload.contradiction_id must be distinct integers in [0, num_labels)",
    "head": "model has no classifier head",
    "labels": "model needs at least 2 labels (an entailment and a contradiction class)",
}


class Options(NamedTuple):
    labels: Tuple[str, ...]
    template: str
    multi_label: bool
    top_k: Optional[int]  # None: every label
    max_hypothesis_tokens: Optional[int]  # None: the engine's default, min(32, (seq_len - 3) // 2)
    entailment_id: Optional[int]  # None: the model's ("?nli=1" / "nli_labels"), else num_labels - 1
    contradiction_id: Optional[int]  # None: the model's, else 0


def options(payload: Dict[str, Any]) -> Options:
    """The validated keys beside the texts; raises the op's ``ValueError`` s before any device work. The
    bounds that depend on the model (the label ids, ``max_hypothesis_tokens``) are checked by
    :func:`check_model` once it is loaded."""
    labels = payload.get("candidate_labels")
    if (not isinstance(labels, list) or not 1 <= len(labels) <= MAX_LABELS
            or not all(isinstance(s, str) and s for s in labels)):
        raise ValueError(ERRORS["candidate_labels"])
    template = payload.get("hypothesis_template", DEFAULT_TEMPLATE)
    if not isinstance(template, str) or template.count("{}") != 1:
        raise ValueError(ERRORS["hypothesis_template"])
    multi = payload.get("multi_label", False)
    if not isinstance(multi, bool):
        raise ValueError(ERRORS["multi_label"])
    top_k = payload.get("top_k")
    if top_k is not None and (not is_int(top_k) or top_k < 1):
        raise ValueError(ERRORS["top_k"])
    mh = payload.get("max_hypothesis_tokens")
    if mh is not None and (not is_int(mh) or mh < 1):
        raise ValueError(ERRORS["max_hypothesis_tokens"])
    ent, con = payload.get("entailment_id"), payload.get("contradiction_id")
    for v in (ent, con):
        if v is not None and (not is_int(v) or v < 0):
            raise ValueError(ERRORS["label_ids"])
    if ent is not None and ent == con:
        raise ValueError(ERRORS["label_ids"])
    return Options(tuple(labels), template, multi, top_k, mh, ent, con)


def check_texts(payload: Dict[str, Any]) -> List[str]:
    """The texts of either payload form."""
    return _jobs.texts_of(payload, ERRORS)


def check_model(h, opt: Options) -> Tuple[int, int]:
    """The model-dependent bounds (the same handle on every rank: all raise together) -> the
    ``(entailment_id, contradiction_id)`` the job runs with."""
    if not getattr(h.spec, "head", True):
        raise ValueError(ERRORS["head"])
    C = h.cfg.num_labels
    if C < 2:
        raise ValueError(ERRORS["labels"])
    S = h.engine.S
    if S < 5 or (opt.max_hypothesis_tokens is not None and opt.max_hypothesis_tokens > S - 4):
        raise ValueError(ERRORS["max_hypothesis_tokens"])
    base = getattr(h.spec, "nli", None) or (C - 1, 0)
    ent = base[0] if opt.entailment_id is None else opt.entailment_id
    con = base[1] if opt.contradiction_id is None else opt.contradiction_id
    if not (0 <= ent < C and 0 <= con < C) or ent == con:
        raise ValueError(ERRORS["label_ids"])
    return ent, con


def hypotheses(opt: Options) -> List[str]:
    """One hypothesis per candidate label: plain replacement of the template's ``{}``."""
    return [opt.template.replace("{}", label) for label in opt.labels]


def result(h, opt: Options, ids: Tuple[int, int], texts: List[str], ranked: List[Tuple[List[int], List[float]]],
           payload: Dict[str, Any], extra: Dict[str, Any]) -> Dict[str, Any]:
    """One job's result from the ``(label indices, scores)`` of its texts, best first (rank 0)."""
    n, L = len(texts), len(opt.labels)
    k = L if opt.top_k is None else min(opt.top_k, L)
    elapsed_ms, rate = _jobs.timing(payload, n * L)
    out = {"ok": True, "op": payload.get("_op", OP_NAME), "model_path": h.model_path, "row_count": n,
           "label_count": L, "pair_count": n * L, "multi_label": opt.multi_label, "hypothesis_template": opt.template,
           "entailment_id": ids[0], "contradiction_id": ids[1], "elapsed_ms": elapsed_ms, "pairs_per_sec": rate}
    out.update(extra)
    out["results"] = [{"labels": [opt.labels[i] for i in order[:k]], "scores": [float(s) for s in score[:k]]}
                      for order, score in ranked]
    return out


def zero_shot_batch(h, payloads: List[Dict[str, Any]], rank: int, ws: int) -> Optional[List[Any]]:
    """The jobs of one lease that share (model, multi_label, max_hypothesis_tokens, entailment_id,
    contradiction_id) as one engine call (every rank calls it; a single job is a batch of one): their
    texts and hypotheses concatenated (label sets and templates may differ per job), the flat text-major
    pair list split contiguously over the DP ranks, the ``[n_r, 2]`` logits all-gathered, every text's
    labels scored and ranked on rank 0. A text's scores depend on its own logits alone, so each job gets
    exactly its single-job result; a bad payload gets its own error entry."""

    def check(p):
        opt = options(p)
        texts = check_texts(p)
        return opt, texts, check_model(h, opt)

    out, jobs = _jobs.validated(payloads, check)
    if jobs:
        key, ids = jobs[0][1], jobs[0][3]
        texts, hyps, ranges = [], [], []
        for _, opt, ts, _ in jobs:
            a = len(hyps)
            hyps.extend(hypotheses(opt))
            texts.extend(ts)
            ranges.extend([(a, len(hyps))] * len(ts))
        goff = _jobs.offsets([range(a, b) for a, b in ranges])

        def compute(s_r, n_r):
            # this rank's pairs of every text; a text with none of them here is not even tokenized
            local = []
            for t, (a, _) in enumerate(ranges):
                lo, hi = max(goff[t], s_r), min(goff[t + 1], s_r + n_r)
                local.append((a + lo - goff[t], a + hi - goff[t]) if hi > lo else (a, a))
            return (h.engine.score_premises(texts, hyps, local, key.max_hypothesis_tokens, ids[0], ids[1]),)

        (pair,) = _jobs.shard_and_gather("zero_shot", goff[-1], rank, ws, compute)
        if rank == 0:
            res = h.engine.rank_labels(pair, goff, key.multi_label)
            t0 = 0
            for i, opt, ts, job_ids in jobs:
                try:
                    ranked = [res.ranked(t) for t in range(t0, t0 + len(ts))]
                    out[i] = ("ok", result(h, opt, job_ids, ts, ranked, payloads[i],
                                           {"dp_world_size": ws} if ws > 1 else {}))
                except Exception as e:
                    out[i] = ("err", e)
                t0 += len(ts)
    return out if rank == 0 else None


@register_batch_op("map_zero_shot")
def map_zero_shot_batch(payloads: List[Dict[str, Any]]) -> List[Any]:
    """Batch handler: jobs that share (model_path, multi_label, max_hypothesis_tokens, entailment_id,
    contradiction_id) go to the device together; malformed payloads take the single-job path and fail alone."""

    def key(p):
        opt = options(p)
        check_texts(p)
        return p.get("model_path"), opt.multi_label, opt.max_hypothesis_tokens, opt.entailment_id, opt.contradiction_id

    return _jobs.lease_batch(payloads, OP_NAME, "map_zero_shot_batch", key, run)


def run(payload: Dict[str, Any], ctx: Dict[str, Any] = None) -> Dict[str, Any]:
    return _jobs.run_single(payload, OP_NAME, OP_NAME, lambda p: (options(p), check_texts(p)))


@register_op("map_zero_shot")
def map_zero_shot(payload: Dict[str, Any], ctx: Dict[str, Any] = None) -> Dict[str, Any]:
    return run(payload, ctx)
