"""``map_embed`` — sentence embeddings from the BERT encoder on MI355X.

Text to vector for search, deduplication and clustering: the rows are tokenized on the GPU,
run through the model's encoder and pooled on the device (``agent_tpu_amd/ops/pool.py``) into
one fp32 vector of the model's hidden size per row. Two payload forms
(see map_embed.CONTRACT.md):

1. text rows ``{"texts": [...]}``;
2. CSV shard ``{"source_uri", "start_row", "shard_size", "text_column"?, "dataset_id"?}`` — rows
   streamed from the native CSV index through the pinned double buffers of ``map_classify``.

Under ``torchrun`` the rows are split over every GPU of the node and the per-rank embeddings
are all-gathered to rank 0. Errors are ``ValueError`` s with the fixed messages of
:data:`ERRORS`; there is no fallback stub.
"""
from __future__ import annotations

import base64
import os
import time
from typing import Any, Dict, List, NamedTuple, Optional

from . import _jobs, register_batch_op, register_op

OP_NAME = "map_embed"

#: every input error of the op (each listed in map_embed.CONTRACT.md)
ERRORS: Dict[str, str] = {
    "missing": 'payload missing required key: "texts" (or "source_uri")',
    "texts": "payload.texts must be a list of strings",
    "pooling": "payload.pooling must be 'mean' or 'cls'",
    "normalize": "payload.normalize must be a boolean",
    "dtype": "payload.dtype must be 'float32' or 'float16'",
    "output": "payload.output must be 'rows', 'base64', 'npy' or 'summary'",
    "output_uri": "payload.output_uri (a local path) is required for output 'npy'",
    "range": "start_row must be >= 0 and shard_size > 0",
    "column": "text_column not in the CSV header",
    "too_large": "row_count * dim exceeds MAP_EMBED_MAX_JSON_VALUES: use output 'base64' or 'npy'",
}


class Options(NamedTuple):
    pooling: str
    normalize: bool
    dtype: str
    output: str
    output_uri: Optional[str]


def max_json_values() -> int:
    return int(os.getenv("MAP_EMBED_MAX_JSON_VALUES", "4194304"))


def options(payload: Dict[str, Any]) -> Options:
    """The validated optional keys; raises the op's ``ValueError`` s before any device work."""
    pooling = payload.get("pooling", "mean")
    if pooling not in ("mean", "cls"):
        raise ValueError(ERRORS["pooling"])
    normalize = payload.get("normalize", True)
    if not isinstance(normalize, bool):
        raise ValueError(ERRORS["normalize"])
    dtype = payload.get("dtype", "float32")
    if dtype not in ("float32", "float16"):
        raise ValueError(ERRORS["dtype"])
    form = payload.get("output", "rows")
    if form not in ("rows", "base64", "npy", "summary"):
        raise ValueError(ERRORS["output"])
    uri = payload.get("output_uri")
    if form == "npy":
        if not isinstance(uri, str) or not uri or "://" in uri and not uri.startswith("file://"):
            raise ValueError(ERRORS["output_uri"])
        uri = uri[len("file://"):] if uri.startswith("file://") else uri
    return Options(pooling, normalize, dtype, form, uri if form == "npy" else None)


def check_texts(payload: Dict[str, Any]) -> List[str]:
    texts = payload["texts"]
    if not isinstance(texts, list):
        raise ValueError(ERRORS["texts"])
    return ["" if t is None else str(t) for t in texts]


def check_json_size(opt: Options, rows: int, dim: int) -> None:
    if opt.output == "rows" and rows * dim > max_json_values():
        raise ValueError(ERRORS["too_large"])


def result(h, emb, payload: Dict[str, Any], extra: Dict[str, Any]) -> Dict[str, Any]:
    """The job's result from the host fp32 embeddings ``emb [n, dim]`` (rank 0)."""
    import numpy as np

    opt = options(payload)
    n, dim = int(emb.shape[0]), int(emb.shape[1])
    check_json_size(opt, n, dim)
    a32 = np.ascontiguousarray(emb.numpy(), dtype="<f4")
    arr = a32.astype("<f2") if opt.dtype == "float16" else a32
    body: Dict[str, Any] = {}
    if opt.output == "rows":
        body["embeddings"] = arr.tolist()
    elif opt.output == "base64":
        body.update(embeddings_b64=base64.b64encode(arr.tobytes()).decode("ascii"), shape=[n, dim], dtype=opt.dtype)
    elif opt.output == "npy":
        tmp = f"{opt.output_uri}.{os.getpid()}.part"
        with open(tmp, "wb") as f:
            np.save(f, arr)
        os.replace(tmp, opt.output_uri)
        body.update(output_uri=opt.output_uri, shape=[n, dim], dtype=opt.dtype, bytes=os.path.getsize(opt.output_uri))
    else:  # summary
        body["centroid"] = a32.mean(0, dtype=np.float64).tolist() if n else [0.0] * dim
        body["norm_mean"] = float(np.linalg.norm(a32.astype(np.float64), axis=1).mean()) if n else 0.0
    elapsed_ms, rate = _jobs.timing(payload, n)
    out = {"ok": True, "op": payload.get("_op", OP_NAME), "model_path": h.model_path, "row_count": n, "dim": dim,
           "pooling": opt.pooling, "normalize": opt.normalize, "elapsed_ms": elapsed_ms, "rows_per_sec": rate}
    out.update(extra)
    out.update(body)
    return out


def embed_batch(h, payloads: List[Dict[str, Any]], rank: int, ws: int) -> Optional[List[Any]]:
    """The ``texts`` jobs of one lease that share (model, pooling, normalize) as one engine call
    (every rank calls it): rows concatenated, split over the DP ranks, all-gathered. Each job
    gets exactly its single-job result; a bad payload gets its own error entry."""
    from agent_tpu_amd.parallel.dp import all_gather_rows, split_range
    from agent_tpu_amd.parallel.dp_ops import exchange_errors

    out: List[Any] = [None] * len(payloads)
    jobs = []
    for i, p in enumerate(payloads):  # same payloads on every rank: same validation outcome
        try:
            opt, texts = options(p), check_texts(p)
            check_json_size(opt, len(texts), h.cfg.hidden)
            jobs.append((i, texts))
        except Exception as exc:
            out[i] = ("err", exc)
    if jobs:
        key = options(payloads[jobs[0][0]])
        texts = [t for _, ts in jobs for t in ts]
        exc, emb = None, None
        try:
            s_r, n_r = split_range(0, len(texts), ws, rank)
            emb = h.engine.embed_texts(texts[s_r:s_r + n_r], key.pooling, key.normalize).emb
        except Exception as e:
            exc = e
        counts = exchange_errors(exc, int(emb.shape[0]) if emb is not None else 0)
        (emb,) = all_gather_rows(emb, counts=counts)
        if rank == 0:
            emb, pos = emb.cpu(), 0
            for i, ts in jobs:
                try:
                    out[i] = ("ok", result(h, emb[pos:pos + len(ts)], payloads[i],
                                           {"dp_world_size": ws} if ws > 1 else {}))
                except Exception as e:  # e.g. an unwritable output_uri: this job alone
                    out[i] = ("err", e)
                pos += len(ts)
    return out if rank == 0 else None


@register_batch_op("map_embed")
def map_embed_batch(payloads: List[Dict[str, Any]]) -> List[Any]:
    """Batch handler: ``texts`` jobs that share (model_path, pooling, normalize) go to the device
    together; CSV-shard jobs (already large) and malformed payloads take the single-job path."""

    def key(p):
        if "texts" not in p:
            raise KeyError("texts")  # not batchable
        opt = options(p)
        return p.get("model_path"), opt.pooling, opt.normalize

    return _jobs.lease_batch(payloads, OP_NAME, "map_embed_batch", key, run)


def run(payload: Dict[str, Any], ctx: Dict[str, Any] = None) -> Dict[str, Any]:
    payload = payload or {}
    t0 = time.time()
    from agent_tpu_amd.parallel.dp_ops import dispatch

    options(payload)  # validated before any device work
    if "texts" in payload:
        check_texts(payload)
        return dispatch("map_embed_rows", dict(payload, _op=OP_NAME, _t0=t0))
    if "source_uri" in payload:
        return dispatch("map_embed_csv", dict(payload, _op=OP_NAME, _t0=t0))
    raise ValueError(ERRORS["missing"])


@register_op("map_embed")
def map_embed(payload: Dict[str, Any], ctx: Dict[str, Any] = None) -> Dict[str, Any]:
    return run(payload, ctx)
