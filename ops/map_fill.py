"""``map_fill`` — masked-token prediction (cloze completion, HF ``fill-mask``) over texts on MI355X.

The model (``BertForMaskedLM``) reads each text with its literal mask tokens replaced by ``[MASK]``, and the
vocabulary head gives every mask its most probable tokens. The rows of the mask positions are gathered on
the GPU and the ``[masks, vocabulary]`` product is reduced there to a log-sum-exp and ``top_k`` tokens per
mask (``agent_tpu_amd/ops/fill.py``): a few candidates per mask come back instead of a logits tensor. Two
payload forms (see map_fill.CONTRACT.md):

1. one text: ``{"text": "the [MASK] sat"}``;
2. several: ``{"texts": ["...", ...]}``.

Under ``torchrun`` the texts are split over every GPU of the node, the per-rank candidates are all-gathered
and rank 0 maps them. Errors are ``ValueError`` s with the fixed messages of :data:`ERRORS`; there is no
fallback stub.
"""
from __future__ import annotations

from typing import Any, Dict, List, NamedTuple, Optional, Tuple

from . import _jobs, register_batch_op, register_op
from ._common import is_int

OP_NAME = "map_fill"
MAX_TOP_K = 32
MAX_TARGETS = 32
MAX_MASKS = 16

#: every input error of the op (each listed in map_fill.CONTRACT.md)
ERRORS: Dict[str, str] = {
    "missing": 'payload missing required key: "text" (or "texts")',
    "both": 'payload must have "text" or "texts", not both',
    "text": "payload.text must be a string",
    "texts": "payload.texts must be a list of strings",
    "top_k": "payload.top_k must be an integer in [1, 32]",
    "mask_token": "payload.mask_token must be a non-empty string",
    "targets": "payload.targets must be a list of 1 to 32 token strings or integer token ids",
    "no_mask": "payload text {index} has no mask token",
    "too_many": "payload text {index} has more than 16 mask tokens",
    "mlm": "model has no MLM head",
    "mask_id": "model vocabulary has no [MASK] token",
    "target_vocab": "string targets need a model with a WordPiece vocabulary",
    "target_unknown": "payload.targets has a token that is not in the vocabulary",
}


class Options(NamedTuple):
    top_k: int
    mask_token: str
    targets: Optional[Tuple[Any, ...]]  # distinct, in payload order: token strings or integer ids


def options(payload: Dict[str, Any]) -> Options:
    """The validated optional keys; raises the op's ``ValueError`` s before any device work."""
    k = payload.get("top_k", 5)
    if not is_int(k) or not 1 <= k <= MAX_TOP_K:
        raise ValueError(ERRORS["top_k"])
    mt = payload.get("mask_token", "[MASK]")
    if not isinstance(mt, str) or not mt:
        raise ValueError(ERRORS["mask_token"])
    tg = payload.get("targets")
    if tg is not None:
        ok = isinstance(tg, list) and all((isinstance(t, str) and t) or is_int(t) for t in tg)
        if not ok:
            raise ValueError(ERRORS["targets"])
        seen, uniq = set(), []
        for t in tg:  # duplicates dropped, first occurrence kept
            if (type(t), t) not in seen:
                seen.add((type(t), t))
                uniq.append(t)
        if not 1 <= len(uniq) <= MAX_TARGETS:
            raise ValueError(ERRORS["targets"])
        tg = tuple(uniq)
    return Options(k, mt, tg)


def check_texts(payload: Dict[str, Any], opt: Options) -> List[str]:
    """The texts of either payload form; each must hold 1 to 16 mask tokens."""
    texts = _jobs.texts_of(payload, ERRORS)
    for i, t in enumerate(texts):
        n = t.count(opt.mask_token)
        if n == 0:
            raise ValueError(ERRORS["no_mask"].format(index=i))
        if n > MAX_MASKS:
            raise ValueError(ERRORS["too_many"].format(index=i))
    return texts


def check_model(h, opt: Options) -> Optional[List[int]]:
    """What depends on the model (the same handle on every rank: all raise together); the target token ids."""
    if not getattr(h.spec, "mlm", False):
        raise ValueError(ERRORS["mlm"])
    vocab = h.engine.vocab
    if vocab is not None and vocab.mask_id is None:
        raise ValueError(ERRORS["mask_id"])
    if opt.targets is None:
        return None
    tids: List[int] = []
    for t in opt.targets:
        if isinstance(t, str):
            if vocab is None:
                raise ValueError(ERRORS["target_vocab"])
            t = vocab.index.get(t.encode("utf-8"))
            if t is None:
                raise ValueError(ERRORS["target_unknown"])
        if not 0 <= t < h.cfg.vocab_size:
            raise ValueError(ERRORS["target_unknown"])
        if t not in tids:  # a string and an id may name the same token
            tids.append(int(t))
    return tids


def result(h, opt: Options, texts: List[str], fills: List[List[Dict[str, Any]]], truncated: List[Tuple[int, int]],
           payload: Dict[str, Any], extra: Dict[str, Any]) -> Dict[str, Any]:
    """One job's result from the mapped ``fills`` of its texts and its ``truncated`` (text, mask) pairs (rank 0)."""
    n = len(texts)
    elapsed_ms, rate = _jobs.timing(payload, n)
    out = {"ok": True, "op": payload.get("_op", OP_NAME), "model_path": h.model_path, "row_count": n,
           "top_k": opt.top_k, "mask_token": opt.mask_token,
           "elapsed_ms": elapsed_ms, "rows_per_sec": rate}
    out.update(extra)
    out["fills"] = fills
    out["truncated"] = [[int(i), int(j)] for i, j in truncated]
    return out


def fill_batch(h, payloads: List[Dict[str, Any]], rank: int, ws: int) -> Optional[List[Any]]:
    """The jobs of one lease that share (model, top_k, mask_token, targets) as one engine call (every rank calls
    it; a single job is a batch of one): their texts concatenated, split contiguously over the DP ranks, the
    tok / prob / pos rows all-gathered and mapped on rank 0. A text's candidates do not depend on the texts it
    shares a batch with, so each job gets exactly its single-job result; a bad payload gets its own error
    entry."""

    def check(p):
        opt = options(p)
        return opt, check_texts(p, opt), check_model(h, opt)

    out, jobs = _jobs.validated(payloads, check)
    if jobs:
        key, tids = jobs[0][1], jobs[0][3]
        texts = [t for _, _, ts, _ in jobs for t in ts]
        M = max([1] + [t.count(key.mask_token) for t in texts])  # every rank's rows have the same width
        tok, prob, pos = _jobs.shard_and_gather(
            "fill", len(texts), rank, ws,
            lambda s_r, n_r: h.engine.fill_rows(texts[s_r:s_r + n_r], key.top_k, key.mask_token, tids, max_masks=M))
        if rank == 0:
            res = h.engine.map_fills(tok, prob, pos, texts, key.mask_token)
            r0 = 0
            for i, opt, ts, _ in jobs:
                try:
                    trunc = [(a - r0, b) for a, b in res.truncated if r0 <= a < r0 + len(ts)]
                    out[i] = ("ok", result(h, opt, ts, res.fills[r0:r0 + len(ts)], trunc, payloads[i],
                                           {"dp_world_size": ws} if ws > 1 else {}))
                except Exception as e:
                    out[i] = ("err", e)
                r0 += len(ts)
    return out if rank == 0 else None


@register_batch_op("map_fill")
def map_fill_batch(payloads: List[Dict[str, Any]]) -> List[Any]:
    """Batch handler: jobs that share (model_path, top_k, mask_token, targets) go to the device together;
    malformed payloads take the single-job path and fail alone."""

    def key(p):
        opt = options(p)
        check_texts(p, opt)
        tg = None if opt.targets is None else tuple((type(t).__name__, t) for t in opt.targets)
        return p.get("model_path"), opt.top_k, opt.mask_token, tg

    return _jobs.lease_batch(payloads, OP_NAME, "map_fill_batch", key, run)


def run(payload: Dict[str, Any], ctx: Dict[str, Any] = None) -> Dict[str, Any]:
    return _jobs.run_single(payload, OP_NAME, OP_NAME, lambda p: check_texts(p, options(p)))


@register_op("map_fill")
def map_fill(payload: Dict[str, Any], ctx: Dict[str, Any] = None) -> Dict[str, Any]:
    return run(payload, ctx)
