"""``map_cluster`` — k-means over ``map_embed`` vectors on MI355X.

"What groups are in here?": Lloyd's k-means, spherical (``metric: "cosine"``) or Euclidean (``"l2"``), over the
rows of a ``map_embed`` ``.npy`` kept resident on the device, over texts embedded on the fly, or over vectors
given as numbers (see map_cluster.CONTRACT.md). The loop is ``agent_tpu_amd/runtime/cluster.py``: an exact fp32
similarity GEMM with an arg-max epilogue, integer (order-free) centroid sums and a single-rounding finalize,
so labels, sizes, centroids, objective and iterations have the same bits for every launch shape and every DP
world size.

A clustering job is a whole-device job: it takes the single-job path (no lease batching, no stream
executor). Under ``torchrun`` every rank holds its ``split_range`` slice of the rows and the per-iteration
sums meet in one integer all-reduce. Errors are ``ValueError`` s with the fixed messages of :data:`ERRORS`;
there is no fallback stub.
"""
from __future__ import annotations

import math
import os
from typing import Any, Dict, NamedTuple, Optional

from . import _jobs, register_op

OP_NAME = "map_cluster"
MAX_K = 4096
MAX_ITER = 300
MAX_REPRESENTATIVES = 32

#: every input error of the op (each listed in map_cluster.CONTRACT.md)
ERRORS: Dict[str, str] = {
    "source": 'payload needs exactly one of "vectors_uri", "texts" or "vectors"',
    "texts": "payload.texts must be a list of strings",
    "vectors": "payload.vectors must be a list of equal-length, non-empty lists of finite numbers",
    "k": "payload.k is required: an integer from 1 to 4096",
    "k_rows": "payload.k exceeds the number of rows",
    "metric": "payload.metric must be 'cosine' or 'l2'",
    "pooling": "payload.pooling must be 'mean' or 'cls'",
    "max_iter": "payload.max_iter must be an integer from 1 to 300",
    "tol": "payload.tol must be a number in [0, 1)",
    "seed": "payload.seed must be an integer from 0 to 2^63 - 1",
    "init_centroids": "payload.init_centroids must be k equal-length lists of finite numbers of the vectors' dim",
    "representatives": "payload.representatives must be an integer from 0 to 32",
    "output": "payload.output must be 'rows', 'npy' or 'summary'",
    "output_uri": "payload.output_uri (a local path) is required for output 'npy'",
    "too_large": "row_count + k * dim exceeds MAP_EMBED_MAX_JSON_VALUES: use output 'npy' or 'summary'",
    "rows_empty": "no rows to cluster",
    "corpus_file": "corpus_uri must be a local 2-D float32 or float16 .npy file",
    "corpus_empty": "corpus has no rows",
    "corpus_nonfinite": "corpus holds non-finite values",
    "corpus_too_large": "corpus slice exceeds SEARCH_INDEX_MAX_GB of float32",
}


class Options(NamedTuple):
    k: int
    metric: str
    pooling: str
    max_iter: int
    tol: float
    seed: int
    representatives: int
    output: str
    output_uri: Optional[str]


def _int(x: Any, lo: int, hi: int) -> bool:
    return isinstance(x, int) and not isinstance(x, bool) and lo <= x <= hi


def _number(x: Any) -> bool:
    return isinstance(x, (int, float)) and not isinstance(x, bool) and math.isfinite(x)


def _matrix(v: Any) -> bool:
    ok = isinstance(v, list) and len(v) > 0 and all(isinstance(r, list) and r for r in v)
    return ok and len({len(r) for r in v}) == 1 and all(_number(a) for r in v for a in r)


def max_json_values() -> int:
    return int(os.getenv("MAP_EMBED_MAX_JSON_VALUES", "4194304"))


def options(payload: Dict[str, Any]) -> Options:
    """The validated option keys; raises the op's ``ValueError`` s before any device work."""
    k = payload.get("k")
    if not _int(k, 1, MAX_K):
        raise ValueError(ERRORS["k"])
    metric = payload.get("metric", "cosine")
    if metric not in ("cosine", "l2"):
        raise ValueError(ERRORS["metric"])
    pooling = payload.get("pooling", "mean")
    if pooling not in ("mean", "cls"):
        raise ValueError(ERRORS["pooling"])
    max_iter = payload.get("max_iter", 25)
    if not _int(max_iter, 1, MAX_ITER):
        raise ValueError(ERRORS["max_iter"])
    tol = payload.get("tol", 0)
    if not _number(tol) or not 0 <= tol < 1:
        raise ValueError(ERRORS["tol"])
    seed = payload.get("seed", 0)
    if not _int(seed, 0, 2 ** 63 - 1):
        raise ValueError(ERRORS["seed"])
    reps = payload.get("representatives", 0)
    if not _int(reps, 0, MAX_REPRESENTATIVES):
        raise ValueError(ERRORS["representatives"])
    form = payload.get("output", "rows")
    if form not in ("rows", "npy", "summary"):
        raise ValueError(ERRORS["output"])
    uri = payload.get("output_uri")
    if form == "npy":
        if not isinstance(uri, str) or not uri or "://" in uri and not uri.startswith("file://"):
            raise ValueError(ERRORS["output_uri"])
        uri = uri[len("file://"):] if uri.startswith("file://") else uri
    return Options(k, metric, pooling, max_iter, float(tol), seed, reps, form, uri if form == "npy" else None)


def check_payload(payload: Dict[str, Any]) -> Options:
    """Everything that can be refused without a device or a file: the options, then the vector source."""
    opt = options(payload)
    if sum(key in payload for key in ("vectors_uri", "texts", "vectors")) != 1:
        raise ValueError(ERRORS["source"])
    dim = None
    if "vectors_uri" in payload:
        from agent_tpu_amd.runtime.search import local_path

        local_path(payload["vectors_uri"])  # a remote or non-string uri: ERRORS["corpus_file"]
    elif "texts" in payload:
        if not isinstance(payload["texts"], list) or not all(t is None or isinstance(t, str) for t in payload["texts"]):
            raise ValueError(ERRORS["texts"])
        rows = len(payload["texts"])
    else:
        if not _matrix(payload["vectors"]):
            raise ValueError(ERRORS["vectors"])
        rows, dim = len(payload["vectors"]), len(payload["vectors"][0])
    if "vectors_uri" not in payload:
        if rows == 0:
            raise ValueError(ERRORS["rows_empty"])
        if opt.k > rows:
            raise ValueError(ERRORS["k_rows"])
    init = payload.get("init_centroids")
    if init is not None:
        if not _matrix(init) or len(init) != opt.k or (dim is not None and len(init[0]) != dim):
            raise ValueError(ERRORS["init_centroids"])
    return opt


def output_paths(uri: str):
    """The two files of ``output: "npy"``, next to ``output_uri``: ``<stem>.labels.npy``, ``<stem>.centroids.npy``."""
    stem = uri[:-4] if uri.endswith(".npy") else uri
    return stem + ".labels.npy", stem + ".centroids.npy"


def _save(path: str, arr) -> None:
    import numpy as np

    tmp = f"{path}.{os.getpid()}.part"
    with open(tmp, "wb") as f:
        np.save(f, arr)
    os.replace(tmp, path)  # rename into place, as map_embed


def load_rows(h, device, payload: Dict[str, Any], opt: Options, rank: int, ws: int):
    """This rank's ``split_range`` slice of the rows on ``device`` (normalised for cosine) ->
    (x ``[n, dim]`` fp32, start, total, index_cached or None)."""
    import torch

    from agent_tpu_amd.parallel.dp import split_range
    from agent_tpu_amd.runtime import search as rs

    cosine = opt.metric == "cosine"
    if "vectors_uri" in payload:
        total, _ = rs.corpus_shape(payload["vectors_uri"])
        s_r, n_r = split_range(0, total, ws, rank)
        corpus = rs.load_corpus(payload["vectors_uri"], s_r, n_r, cosine, device)
        return corpus.vectors, s_r, total, corpus.cached
    if "texts" in payload:
        texts = ["" if t is None else str(t) for t in payload["texts"]]
        s_r, n_r = split_range(0, len(texts), ws, rank)
        if n_r == 0:
            return torch.zeros((0, h.cfg.hidden), dtype=torch.float32, device=device), s_r, len(texts), None
        x = h.engine.embed_texts(texts[s_r:s_r + n_r], opt.pooling, cosine).emb.to(device=device, dtype=torch.float32)
        return x.contiguous(), s_r, len(texts), None
    rows = payload["vectors"]
    s_r, n_r = split_range(0, len(rows), ws, rank)
    x = torch.tensor(rows[s_r:s_r + n_r], dtype=torch.float32).reshape(n_r, len(rows[0])).to(device)
    x = rs.normalize_rows(x) if cosine and n_r else x
    return x.contiguous(), s_r, len(rows), None


def representatives(km, x, opt: Options, labels_all, best_all, start: int, total: int, rank: int, ws: int):
    """Every cluster's ``n`` best member ids and scores in the total order (score desc, id asc). ``cosine``: the
    centroids are the queries of a ``sim_topk`` over the rows (at most 32 candidates per centroid), filtered by
    label; ``l2``: the members ranked on the host by ``best``. -> a list of ``{"ids", "scores"}`` on rank 0."""
    import torch

    from agent_tpu_amd.parallel.dp import all_gather_rows
    from agent_tpu_amd.runtime import search as rs

    n, K = opt.representatives, opt.k
    if opt.metric == "cosine":
        top = MAX_REPRESENTATIVES
        s, i = rs.search(km.centroids, x, top, id_base=start)
        if s.shape[1] < top:
            pad = top - s.shape[1]
            s = torch.cat([s, torch.full((K, pad), float("-inf"), dtype=s.dtype, device=s.device)], 1)
            i = torch.cat([i, torch.full((K, pad), 2 ** 62, dtype=i.dtype, device=i.device)], 1)
        s, i = all_gather_rows(s.contiguous(), i.contiguous(), counts=[K] * ws)
        if rank != 0:
            return None
        s, i = s.cpu(), i.cpu()
        if ws > 1:
            s = s.view(ws, K, top).permute(1, 0, 2).reshape(K, ws * top)
            i = i.view(ws, K, top).permute(1, 0, 2).reshape(K, ws * top)
            s, i = rs.merge_topk(s, i, top)
        out, lab_l = [], labels_all.tolist()
        for k in range(K):
            keep = [(int(r), float(v)) for r, v in zip(i[k].tolist(), s[k].tolist()) if r < total and lab_l[r] == k]
            out.append({"ids": [r for r, _ in keep[:n]], "scores": [v for _, v in keep[:n]]})
        return out
    if rank != 0:
        return None
    by_id = torch.arange(total)
    order = torch.sort(best_all + 0.0, descending=True, stable=True).indices  # ids ascending among equal scores
    lab = labels_all[order]
    out = []
    for k in range(K):
        pick = order[lab == k][:n]
        out.append({"ids": by_id[pick].tolist(), "scores": best_all[pick].tolist()})
    return out


def cluster_one(payload: Dict[str, Any], rank: int, ws: int) -> Optional[Dict[str, Any]]:
    """One job (every rank calls it)."""
    import torch

    from agent_tpu_amd import ops as kops
    from agent_tpu_amd.parallel.dp import all_gather_rows
    from agent_tpu_amd.parallel.dp_ops import exchange_errors, maybe_inject_fault
    from agent_tpu_amd.runtime import cluster as rc

    from ._gpu_runtime import device_for_rank, get_gpu_handle, get_model_path

    opt = check_payload(payload)  # the same payload on every rank: all raise together
    if "texts" in payload:
        h = get_gpu_handle(get_model_path(payload.get("model_path")))
        device = h.engine.device
    else:
        h, device = None, device_for_rank()
    exc, x, start, total, cached, init = None, None, 0, 0, None, None
    try:
        x, start, total, cached = load_rows(h, device, payload, opt, rank, ws)
        dim = int(x.shape[1])
        if total == 0:
            raise ValueError(ERRORS["rows_empty"])
        if opt.k > total:
            raise ValueError(ERRORS["k_rows"])
        if payload.get("init_centroids") is not None:
            if len(payload["init_centroids"][0]) != dim:
                raise ValueError(ERRORS["init_centroids"])
            init = torch.tensor(payload["init_centroids"], dtype=torch.float32)
        if opt.output == "rows" and total + opt.k * dim > max_json_values():
            raise ValueError(ERRORS["too_large"])
        if device.type == "cuda" and not kops.kmeans_ok(dim, opt.k):  # kmeans_assign's own error, before the loop
            raise ValueError(f"agent_tpu_amd: kmeans_assign: unsupported shape D={dim} K={opt.k}")
        maybe_inject_fault("cluster")
    except Exception as e:
        exc = e
    counts = exchange_errors(exc, int(x.shape[0]) if x is not None else 0)
    km = rc.kmeans(x, opt.k, opt.metric, opt.seed, opt.max_iter, opt.tol, init, rank, ws, start, total)
    labels, best = all_gather_rows(km.labels, km.best, counts=counts)
    labels, best = labels.cpu(), best.cpu()
    reps = representatives(km, x, opt, labels, best, start, total, rank, ws) if opt.representatives else None
    if rank != 0:
        return None
    return result(km, labels, payload, opt, total, dim, cached, reps, ws)


def result(km, labels, payload: Dict[str, Any], opt: Options, total: int, dim: int, cached: Optional[bool], reps,
           ws: int) -> Dict[str, Any]:
    """The job's result (rank 0) from the loop's outcome and the gathered labels."""
    import numpy as np

    sizes = km.sizes.cpu().tolist()
    cent = km.centroids.cpu()
    elapsed_ms, rate = _jobs.timing(payload, total)
    out: Dict[str, Any] = {"ok": True, "op": payload.get("_op", OP_NAME), "row_count": total, "dim": dim, "k": opt.k,
                           "metric": opt.metric, "iterations": km.iterations, "converged": km.converged,
                           "changed_last": km.changed_last, "objective": km.objective, "sizes": sizes,
                           "empty_clusters": sum(1 for s in sizes if s == 0), "elapsed_ms": elapsed_ms,
                           "rows_per_sec": rate, "dp_world_size": ws}
    if cached is not None:
        out["index_cached"] = bool(cached)
    if opt.output == "rows":
        out.update(labels=labels.tolist(), centroids=cent.tolist())
    elif opt.output == "npy":
        lp, cp = output_paths(opt.output_uri)
        _save(lp, np.ascontiguousarray(labels.numpy(), dtype="<i4"))
        _save(cp, np.ascontiguousarray(cent.numpy(), dtype="<f4"))
        out.update(labels_uri=lp, centroids_uri=cp)
    if reps is not None:
        out["representatives"] = reps
    return out


def run(payload: Dict[str, Any], ctx: Dict[str, Any] = None) -> Dict[str, Any]:
    return _jobs.run_single(payload, OP_NAME, OP_NAME, check_payload)


@register_op("map_cluster")
def map_cluster(payload: Dict[str, Any], ctx: Dict[str, Any] = None) -> Dict[str, Any]:
    return run(payload, ctx)
