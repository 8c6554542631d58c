"""``map_sparse_embed`` — learned sparse (SPLADE) term weights of texts on MI355X: the lexical half of hybrid
retrieval, next to ``map_embed``'s dense vectors.

The model (``BertForMaskedLM``) scores every vocabulary entry at every token of a text; a term's weight is
``log1p(relu(max over the text's tokens of its logit))``. The vocabulary product of all token rows is reduced
per text on the GPU and only the best ``max_terms`` terms of each text come back
(``agent_tpu_amd/ops/sparse.py``): no ``[tokens, vocabulary]`` logits tensor exists. Two payload forms (see
map_sparse_embed.CONTRACT.md):

1. one text: ``{"text": "..."}``;
2. several: ``{"texts": ["...", ...]}``.

``output: "npz"`` with ``output_uri`` writes the rows as a CSR ``.npz`` instead of returning the lists: the corpus
file of ``map_sparse_search``.

Under ``torchrun`` the texts are split over every GPU of the node, the per-rank term rows are all-gathered and
rank 0 maps them. Errors are ``ValueError`` s with the fixed messages of :data:`ERRORS`; there is no fallback
stub.
"""
from __future__ import annotations

import math
import os
from typing import Any, Dict, List, NamedTuple, Optional

from . import _jobs, register_batch_op, register_op
from ._common import is_int

OP_NAME = "map_sparse_embed"
MAX_TERMS = 1024

#: every input error of the op (each listed in map_sparse_embed.CONTRACT.md)
ERRORS: Dict[str, str] = {
    "missing": 'payload missing required key: "text" (or "texts")',
    "both": 'payload must have "text" or "texts", not both',
    "text": "payload.text must be a string",
    "texts": "payload.texts must be a list of strings",
    "max_terms": "payload.max_terms must be an integer in [1, 1024]",
    "min_weight": "payload.min_weight must be a finite number >= 0",
    "mlm": "model has no MLM head",
}
#: the errors of the file output (listed there too)
OUTPUT_ERRORS: Dict[str, str] = {
    "output": "payload.output must be 'terms' or 'npz'",
    "output_uri": "payload.output_uri (a local path) is required for output 'npz'",
}


class Options(NamedTuple):
    max_terms: int
    min_weight: float
    output: str = "terms"
    output_uri: Optional[str] = None


def options(payload: Dict[str, Any]) -> Options:
    """The validated optional keys; raises the op's ``ValueError`` s before any device work."""
    k = payload.get("max_terms", 256)
    if not is_int(k) or not 1 <= k <= MAX_TERMS:
        raise ValueError(ERRORS["max_terms"])
    mw = _jobs.number_or_none(payload, "min_weight", ERRORS["min_weight"])
    mw = 0.0 if mw is None else mw
    if not math.isfinite(mw) or mw < 0:
        raise ValueError(ERRORS["min_weight"])
    form = payload.get("output", "terms")
    if form not in ("terms", "npz"):
        raise ValueError(OUTPUT_ERRORS["output"])
    uri = payload.get("output_uri")
    if form == "npz" and (not isinstance(uri, str) or not uri or "://" in uri):
        raise ValueError(OUTPUT_ERRORS["output_uri"])
    return Options(k, mw, form, uri if form == "npz" else None)


def check_model(h) -> None:
    """What depends on the model (the same handle on every rank: all raise together)."""
    if not getattr(h.spec, "mlm", False):
        raise ValueError(ERRORS["mlm"])


def result(h, opt: Options, n: int, terms: List[Dict[str, Any]], nnz: List[int], payload: Dict[str, Any],
           extra: Dict[str, Any]) -> Dict[str, Any]:
    """One job's result from the mapped ``terms`` and ``nnz`` of its texts (rank 0)."""
    elapsed_ms, rate = _jobs.timing(payload, n)
    out = {"ok": True, "op": payload.get("_op", OP_NAME), "model_path": h.model_path, "row_count": n,
           "vocab_size": int(h.cfg.vocab_size), "max_terms": opt.max_terms,
           "elapsed_ms": elapsed_ms, "rows_per_sec": rate}
    out.update(extra)
    if opt.output == "npz":  # the corpus file of map_sparse_search: CSR, fp32, the tokens of a row ascending
        from agent_tpu_amd.runtime.sparse_index import save_csr

        rows = [sorted(zip(t["token_ids"], t["weights"])) for t in terms]  # min_weight is applied already
        save_csr(opt.output_uri, _jobs.offsets(rows), [t for r in rows for t, _ in r], [w for r in rows for _, w in r],
                 (n, int(h.cfg.vocab_size)))
        out.update(output_uri=opt.output_uri, shape=[n, int(h.cfg.vocab_size)], stored=sum(len(r) for r in rows),
                   bytes=os.path.getsize(opt.output_uri))
    else:
        out["terms"] = terms
    out["nnz"] = [int(c) for c in nnz]
    return out


def sparse_batch(h, payloads: List[Dict[str, Any]], rank: int, ws: int) -> Optional[List[Any]]:
    """The jobs of one lease that share (model, max_terms) as one engine call (every rank calls it; a single
    job is a batch of one): their texts concatenated, split contiguously over the DP ranks, the tok / w / nnz
    rows all-gathered and mapped on rank 0, each job with its own ``min_weight``. A text's terms do not depend
    on the texts it shares a batch with, so each job gets exactly its single-job result; a bad payload gets
    its own error entry."""

    def check(p):
        opt = options(p)
        texts = _jobs.texts_of(p, ERRORS)
        check_model(h)
        return opt, texts

    out, jobs = _jobs.validated(payloads, check)
    if jobs:
        k = jobs[0][1].max_terms
        texts = [t for _, _, ts in jobs for t in ts]

        def compute(s_r, n_r):
            tok, _, w, nnz = h.engine.sparse_rows(texts[s_r:s_r + n_r], k)
            return tok, w, nnz

        tok, w, nnz = _jobs.shard_and_gather("sparse", len(texts), rank, ws, compute)
        if rank == 0:
            r0 = 0
            for i, opt, ts in jobs:
                try:
                    a, b = r0, r0 + len(ts)
                    terms, counts = h.engine.map_terms(tok[a:b], w[a:b], nnz[a:b], opt.min_weight)
                    out[i] = ("ok", result(h, opt, len(ts), terms, counts, payloads[i],
                                           {"dp_world_size": ws} if ws > 1 else {}))
                except Exception as e:
                    out[i] = ("err", e)
                r0 += len(ts)
    return out if rank == 0 else None


@register_batch_op("map_sparse_embed")
def map_sparse_embed_batch(payloads: List[Dict[str, Any]]) -> List[Any]:
    """Batch handler: jobs that share (model_path, max_terms) go to the device together; malformed payloads
    take the single-job path and fail alone."""

    def key(p):
        opt = options(p)
        _jobs.texts_of(p, ERRORS)
        return p.get("model_path"), opt.max_terms

    return _jobs.lease_batch(payloads, OP_NAME, "map_sparse_embed_batch", key, run)


def run(payload: Dict[str, Any], ctx: Dict[str, Any] = None) -> Dict[str, Any]:
    return _jobs.run_single(payload, OP_NAME, OP_NAME, lambda p: (options(p), _jobs.texts_of(p, ERRORS)))


@register_op("map_sparse_embed")
def map_sparse_embed(payload: Dict[str, Any], ctx: Dict[str, Any] = None) -> Dict[str, Any]:
    return run(payload, ctx)
