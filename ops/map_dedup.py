"""``map_dedup`` — near-duplicate groups over ``map_embed`` vectors on MI355X.

"Which rows are near-duplicates of each other, and which one row of each group should be kept?": all pairs
``i < j`` with ``score(i, j) >= threshold`` (cosine or dot product) over the rows of a ``map_embed`` ``.npy`` kept
resident on the device, over texts embedded on the fly, or over vectors given as numbers (see
map_dedup.CONTRACT.md), then the connected components of that graph. The middle is
``agent_tpu_amd/runtime/dedup.py``: an exact fp32 similarity self-join whose epilogue emits the few pairs
that pass (the score matrix is never written) and a minimum-label connected-components kernel, so the pairs,
the groups and every count have the same bits for every launch shape and every DP world size.

A dedup job is a whole-device job: it takes the single-job path (no lease batching, no stream executor).
Under ``torchrun`` every rank holds all rows and joins every ``ws``-th block of rows against them; the pairs
meet in one ragged all-gather. Errors are ``ValueError`` s with the fixed messages of :data:`ERRORS`; there is
no fallback stub.
"""
from __future__ import annotations

import math
import struct
from typing import Any, Dict, NamedTuple, Optional

from . import _jobs, register_op
from .map_cluster import _int, _matrix, _save, max_json_values

OP_NAME = "map_dedup"
MAX_PAIRS = 65536

#: every input error of the op (each listed in map_dedup.CONTRACT.md)
ERRORS: Dict[str, str] = {
    "source": 'payload needs exactly one of "vectors_uri", "texts" or "vectors"',
    "texts": "payload.texts must be a list of strings",
    "vectors": "payload.vectors must be a list of equal-length, non-empty lists of finite numbers",
    "threshold": "payload.threshold is required: a finite number (in float32)",
    "metric": "payload.metric must be 'cosine' or 'dot'",
    "pooling": "payload.pooling must be 'mean' or 'cls'",
    "max_pairs": "payload.max_pairs must be an integer from 0 to 65536",
    "output": "payload.output must be 'rows', 'npy' or 'summary'",
    "output_uri": "payload.output_uri (a local path) is required for output 'npy'",
    "too_large": "row_count exceeds MAP_EMBED_MAX_JSON_VALUES: use output 'npy' or 'summary'",
    "rows_empty": "no rows to deduplicate",
    "dim": "the vectors' dim must be a multiple of 64 from 64 to 1024",
    "corpus_file": "corpus_uri must be a local 2-D float32 or float16 .npy file",
    "corpus_empty": "corpus has no rows",
    "corpus_nonfinite": "corpus holds non-finite values",
    "corpus_too_large": "corpus slice exceeds SEARCH_INDEX_MAX_GB of float32",
}


class Options(NamedTuple):
    threshold: float  # the fp32 value
    metric: str
    pooling: str
    max_pairs: int
    output: str
    output_uri: Optional[str]


def to_fp32(t: Any) -> float:
    """``t`` rounded once to fp32 (ties to even), as a Python float; raises the threshold error otherwise."""
    if isinstance(t, bool) or not isinstance(t, (int, float)) or not math.isfinite(t):
        raise ValueError(ERRORS["threshold"])
    try:
        return struct.unpack("<f", struct.pack("<f", t))[0]
    except OverflowError:  # beyond the fp32 range
        raise ValueError(ERRORS["threshold"]) from None


def options(payload: Dict[str, Any]) -> Options:
    """The validated option keys; raises the op's ``ValueError`` s before any device work."""
    threshold = to_fp32(payload.get("threshold"))
    metric = payload.get("metric", "cosine")
    if metric not in ("cosine", "dot"):
        raise ValueError(ERRORS["metric"])
    pooling = payload.get("pooling", "mean")
    if pooling not in ("mean", "cls"):
        raise ValueError(ERRORS["pooling"])
    max_pairs = payload.get("max_pairs", 0)
    if not _int(max_pairs, 0, MAX_PAIRS):
        raise ValueError(ERRORS["max_pairs"])
    form = payload.get("output", "rows")
    if form not in ("rows", "npy", "summary"):
        raise ValueError(ERRORS["output"])
    uri = payload.get("output_uri")
    if form == "npy":
        if not isinstance(uri, str) or not uri or "://" in uri and not uri.startswith("file://"):
            raise ValueError(ERRORS["output_uri"])
        uri = uri[len("file://"):] if uri.startswith("file://") else uri
    return Options(threshold, metric, pooling, max_pairs, form, uri if form == "npy" else None)


def check_payload(payload: Dict[str, Any]) -> Options:
    """Everything that can be refused without a device or a file: the options, then the vector source."""
    opt = options(payload)
    if sum(key in payload for key in ("vectors_uri", "texts", "vectors")) != 1:
        raise ValueError(ERRORS["source"])
    if "vectors_uri" in payload:
        from agent_tpu_amd.runtime.search import local_path

        local_path(payload["vectors_uri"])  # a remote or non-string uri: ERRORS["corpus_file"]
    elif "texts" in payload:
        if not isinstance(payload["texts"], list) or not all(t is None or isinstance(t, str) for t in payload["texts"]):
            raise ValueError(ERRORS["texts"])
        if not payload["texts"]:
            raise ValueError(ERRORS["rows_empty"])
    else:
        if not _matrix(payload["vectors"]):
            raise ValueError(ERRORS["vectors"])
        if not _dim_ok(len(payload["vectors"][0])):
            raise ValueError(ERRORS["dim"])
    return opt


def _dim_ok(dim: int) -> bool:
    return dim % 64 == 0 and 64 <= dim <= 1024  # ops.sim_join_ok


def output_path(uri: str) -> str:
    """The file of ``output: "npy"``, next to ``output_uri``: ``<stem>.group.npy``."""
    stem = uri[:-4] if uri.endswith(".npy") else uri
    return stem + ".group.npy"


def load_rows(h, device, payload: Dict[str, Any], opt: Options, rank: int, ws: int):
    """-> (x fp32 on ``device``, total, index_cached or None). ``vectors_uri`` and ``vectors``: all rows on every
    rank; ``texts``: this rank's ``split_range`` slice (the caller all-gathers). Normalised for cosine."""
    import torch

    from agent_tpu_amd.parallel.dp import split_range
    from agent_tpu_amd.runtime import search as rs

    cosine = opt.metric == "cosine"
    if "vectors_uri" in payload:
        corpus = rs.load_corpus(payload["vectors_uri"], 0, -1, cosine, device)
        return corpus.vectors, corpus.total, corpus.cached
    if "texts" in payload:
        texts = ["" if t is None else str(t) for t in payload["texts"]]
        s_r, n_r = split_range(0, len(texts), ws, rank)
        if n_r == 0:
            return torch.zeros((0, h.cfg.hidden), dtype=torch.float32, device=device), len(texts), None
        x = h.engine.embed_texts(texts[s_r:s_r + n_r], opt.pooling, cosine).emb.to(device=device, dtype=torch.float32)
        return x.contiguous(), len(texts), None
    rows = payload["vectors"]
    x = torch.tensor(rows, dtype=torch.float32).reshape(len(rows), len(rows[0])).to(device)
    x = rs.normalize_rows(x) if cosine else x
    return x.contiguous(), len(rows), None


def dedup_one(payload: Dict[str, Any], rank: int, ws: int) -> Optional[Dict[str, Any]]:
    """One job (every rank calls it)."""
    from agent_tpu_amd.parallel.dp import all_gather_rows
    from agent_tpu_amd.parallel.dp_ops import exchange_errors, maybe_inject_fault
    from agent_tpu_amd.runtime import dedup as rd

    from ._gpu_runtime import device_for_rank, get_gpu_handle, get_model_path

    opt = check_payload(payload)  # the same payload on every rank: all raise together
    if "texts" in payload:
        h = get_gpu_handle(get_model_path(payload.get("model_path")))
        device = h.engine.device
    else:
        h, device = None, device_for_rank()
    exc, x, total, cached = None, None, 0, None
    try:
        x, total, cached = load_rows(h, device, payload, opt, rank, ws)
        if not _dim_ok(int(x.shape[1])):
            raise ValueError(ERRORS["dim"])
        if opt.output == "rows" and total > max_json_values():
            raise ValueError(ERRORS["too_large"])
        maybe_inject_fault("dedup")
    except Exception as e:
        exc = e
    counts = exchange_errors(exc, int(x.shape[0]) if x is not None else 0)
    if "texts" in payload:
        (x,) = all_gather_rows(x, counts=counts)
        x = x.contiguous()
    dup = rd.near_duplicates(x, opt.threshold, rank, ws, total)
    if rank != 0:
        return None
    return result(dup, payload, opt, total, int(x.shape[1]), cached, ws)


def best_pairs(pairs, scores, n: int):
    """The best ``n`` of the (I, J)-sorted pairs in the total order score descending, ``i`` ascending, ``j``
    ascending: one stable sort (``+ 0.0``: ``-0.0`` ties with ``+0.0``)."""
    import torch

    order = torch.sort(scores + 0.0, descending=True, stable=True).indices[:n]
    return [{"i": int(i), "j": int(j), "score": float(s)}
            for (i, j), s in zip(pairs[order].tolist(), scores[order].tolist())]


def result(dup, payload: Dict[str, Any], opt: Options, total: int, dim: int, cached: Optional[bool], ws: int
           ) -> Dict[str, Any]:
    """The job's result (rank 0) from the labels and the sorted pairs."""
    import numpy as np
    import torch

    labels = dup.labels.cpu()
    sizes = torch.bincount(labels.to(torch.int64), minlength=total)
    duplicates = int((labels != torch.arange(total, dtype=torch.int32)).sum())
    elapsed_ms, rate = _jobs.timing(payload, total)
    out: Dict[str, Any] = {"ok": True, "op": payload.get("_op", OP_NAME), "row_count": total, "dim": dim,
                           "metric": opt.metric, "threshold": opt.threshold, "pair_count": int(dup.pairs.shape[0]),
                           "group_count": int((sizes >= 2).sum()), "duplicate_count": duplicates,
                           "kept_count": total - duplicates, "largest_group": int(sizes.max()),
                           "elapsed_ms": elapsed_ms, "rows_per_sec": rate, "dp_world_size": ws}
    if cached is not None:
        out["index_cached"] = bool(cached)
    if opt.output == "rows":
        group = labels.tolist()
        out.update(group=group, keep=[i for i, g in enumerate(group) if g == i])
    elif opt.output == "npy":
        path = output_path(opt.output_uri)
        _save(path, np.ascontiguousarray(labels.numpy(), dtype="<i4"))
        out["group_uri"] = path
    if opt.max_pairs > 0:
        out["pairs"] = best_pairs(dup.pairs.cpu(), dup.scores.cpu(), opt.max_pairs)
    return out


def run(payload: Dict[str, Any], ctx: Dict[str, Any] = None) -> Dict[str, Any]:
    return _jobs.run_single(payload, OP_NAME, OP_NAME, check_payload)


@register_op("map_dedup")
def map_dedup(payload: Dict[str, Any], ctx: Dict[str, Any] = None) -> Dict[str, Any]:
    return run(payload, ctx)
