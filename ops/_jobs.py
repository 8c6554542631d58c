"""The parts every batched GPU op shares (``map_rerank``, ``map_answer``, ``map_tag``, ``map_fill`` ...):
the lease handler, the single-job entry, per-payload validation, the collective middle of a DP job and
the small payload checks. Plain functions; each op module keeps what is its own."""
from __future__ import annotations

import time
from typing import Any, Callable, Dict, List, Optional, Sequence, Tuple


def lease_batch(payloads: List[Dict[str, Any]], op_name: str, task_name: str, group_key: Callable[[Dict[str, Any]], Any],
                single: Callable[[Dict[str, Any]], Any]) -> List[Any]:
    """The batch handler of an op: the jobs of one lease that share ``group_key(p)`` go to the device
    together, as one dispatch of ``task_name``; a payload whose ``group_key`` raises (malformed, or
    not batchable) takes the single-job path ``single(p)`` and fails alone. One ``("ok", result)`` /
    ``("err", exc)`` entry per payload; a dispatch that raises fills its group with that error."""
    from agent_tpu_amd.parallel.dp_ops import dispatch

    t0 = time.time()
    out: List[Any] = [None] * len(payloads)
    groups: Dict[Any, List[int]] = {}
    for i, p in enumerate(payloads):
        p = p or {}
        try:
            groups.setdefault(group_key(p), []).append(i)
        except Exception:
            try:
                out[i] = ("ok", single(p))
            except Exception as exc:
                out[i] = ("err", exc)
    for idxs in groups.values():
        descs = [dict(payloads[i], _op=op_name, _t0=t0) for i in idxs]
        try:
            res = dispatch(task_name, {"payloads": descs})
        except Exception as exc:
            res = [("err", exc)] * len(idxs)
        for i, entry in zip(idxs, res):
            out[i] = entry
    return out


def run_single(payload: Optional[Dict[str, Any]], op_name: str, task_name: str,
               validate: Callable[[Dict[str, Any]], Any]) -> Any:
    """One job: ``validate(payload)`` raises the op's errors before any device work, then the task runs
    on every rank."""
    payload = payload or {}
    t0 = time.time()
    from agent_tpu_amd.parallel.dp_ops import dispatch

    validate(payload)
    return dispatch(task_name, dict(payload, _op=op_name, _t0=t0))


def validated(payloads: List[Dict[str, Any]], check: Callable[[Dict[str, Any]], tuple]) -> Tuple[List[Any], List[tuple]]:
    """``(out, jobs)``: ``jobs`` holds ``(i,) + check(p)`` for every payload that passes, ``out[i]`` is
    ``("err", exc)`` for one that does not (the same payloads on every rank: the same outcome)."""
    out: List[Any] = [None] * len(payloads)
    jobs = []
    for i, p in enumerate(payloads):
        try:
            jobs.append((i,) + tuple(check(p)))
        except Exception as exc:
            out[i] = ("err", exc)
    return out, jobs


def shard_and_gather(stage: str, n_items: int, rank: int, ws: int, compute: Callable[[int, int], tuple]) -> tuple:
    """The collective middle of a DP job: this rank's contiguous share ``(s_r, n_r)`` of ``n_items``
    goes through ``compute``, which returns a tuple of row tensors; the per-rank errors and row counts
    are exchanged (every rank reaches the exchange, also one whose ``compute`` raised, and all fail
    together) and the rows all-gathered."""
    from agent_tpu_amd.parallel.dp import all_gather_rows, split_range
    from agent_tpu_amd.parallel.dp_ops import exchange_errors, maybe_inject_fault

    exc, rows = None, None
    try:
        s_r, n_r = split_range(0, n_items, ws, rank)
        maybe_inject_fault(stage)
        rows = compute(s_r, n_r)
    except Exception as e:
        exc = e
    counts = exchange_errors(exc, int(rows[0].shape[0]) if rows is not None else 0)
    return all_gather_rows(*rows, counts=counts)


def pairs_of(payload: Dict[str, Any], one: str, many: str, errors: Dict[str, str]) -> Tuple[List[str], List[List[str]]]:
    """``(queries, passages per query)`` of a pair payload, either ``{one: str, "passages": [str]}`` or
    ``{many: [str], "passages": [[str]]}``; ``errors`` has the keys ``missing``, ``both``, ``one``,
    ``many``, ``passages`` and ``passage_lists``."""
    if "passages" not in payload or (one not in payload and many not in payload):
        raise ValueError(errors["missing"])
    if one in payload and many in payload:
        raise ValueError(errors["both"])
    passages = payload["passages"]
    if one in payload:
        if not isinstance(payload[one], str):
            raise ValueError(errors[one])
        if not isinstance(passages, list) or not all(isinstance(p, str) for p in passages):
            raise ValueError(errors["passages"])
        return [payload[one]], [list(passages)]
    queries = payload[many]
    if not isinstance(queries, list) or not all(isinstance(q, str) for q in queries):
        raise ValueError(errors[many])
    if (not isinstance(passages, list) or len(passages) != len(queries)
            or not all(isinstance(ps, list) and all(isinstance(p, str) for p in ps) for ps in passages)):
        raise ValueError(errors["passage_lists"])
    return list(queries), [list(ps) for ps in passages]


def texts_of(payload: Dict[str, Any], errors: Dict[str, str]) -> List[str]:
    """The texts of either form, ``{"text": str}`` or ``{"texts": [str]}``."""
    if "text" not in payload and "texts" not in payload:
        raise ValueError(errors["missing"])
    if "text" in payload and "texts" in payload:
        raise ValueError(errors["both"])
    if "text" in payload:
        if not isinstance(payload["text"], str):
            raise ValueError(errors["text"])
        return [payload["text"]]
    texts = payload["texts"]
    if not isinstance(texts, list) or not all(isinstance(t, str) for t in texts):
        raise ValueError(errors["texts"])
    return list(texts)


def offsets(groups: Sequence[Sequence[Any]]) -> List[int]:
    """``[0, len(g0), len(g0) + len(g1), ...]``: where every group's rows start in the flat list."""
    goff = [0]
    for g in groups:
        goff.append(goff[-1] + len(g))
    return goff


def number_or_none(payload: Dict[str, Any], key: str, error: str) -> Optional[float]:
    """An optional number (no bool, no NaN) as a float."""
    v = payload.get(key)
    if v is None:
        return None
    if isinstance(v, bool) or not isinstance(v, (int, float)) or v != v:
        raise ValueError(error)
    return float(v)


def timing(payload: Dict[str, Any], n: int) -> Tuple[float, Optional[float]]:
    """``(elapsed_ms, items per second)`` of a job of ``n`` items since its ``_t0``."""
    dt = time.time() - float(payload.get("_t0", time.time()))
    return dt * 1000.0, (n / dt) if dt > 0 else None
