"""Rank body of the filtered map_search DP test (launched by torch.distributed.run, gloo, CPU engines
via CLASSIFY_DEVICE=cpu): rank 0 runs the op, the others serve in ``worker_loop``. Rank 0 prints one
``RESULT {json}`` line with the DP results next to single-process references on the same data."""
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, REPO)

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402

from agent_tpu_amd import ops  # noqa: E402
from agent_tpu_amd.parallel import dp, dp_ops  # noqa: E402

N, D = 101, 64  # slice starts 51 (world 2) and 34, 68 (world 3): no multiple of 32
TIMING = ("elapsed_ms", "queries_per_sec", "index_cached")


def scenario():
    rank, ws = dp.world()
    if rank != 0:
        dp_ops.worker_loop()
        return None
    from ops.map_search import FILTER_ERRORS, map_search, map_search_batch

    tmp = os.environ["DP_TEST_DIR"]
    gen = torch.Generator().manual_seed(9)
    c = torch.randint(-2, 3, (N, D), generator=gen).float()
    for r in (33, 34, 50, 51, 67, 68, 100):  # one vector on both sides of every slice boundary: ties across ranks
        c[r] = c[2]
    q = torch.randint(-2, 3, (5, D), generator=gen).float()
    q[0] = c[2]
    labels = np.arange(N, dtype=np.int64) // 10  # 0 .. 10 in ascending blocks
    cpath, lpath = os.path.join(tmp, "corpus.npy"), os.path.join(tmp, "labels.npy")
    np.save(cpath, c.numpy())
    np.save(lpath, labels)
    job = {"query_vectors": q.tolist(), "corpus_uri": cpath, "metric": "dot", "top_k": 8, "corpus_labels_uri": lpath}

    def single(rows, k=8):
        """The single-process answer: the twin over the gathered allowed rows, ids mapped back."""
        R = torch.tensor(sorted(rows), dtype=torch.int64)
        if R.numel() == 0:
            return {"ids": [[] for _ in range(q.shape[0])], "scores": [[] for _ in range(q.shape[0])], "filter_rows": 0}
        s, i = ops.sim_topk_ref(q, c[R].contiguous(), k)
        return {"ids": R[i].tolist(), "scores": s.tolist(), "filter_rows": int(R.numel())}

    cases = {
        # rows of every slice, the boundary copies included
        "ids_all_ranks": ({"ids": [2, 33, 34, 50, 51, 67, 68, 100, 5, 40, 41, 90, 90]},
                          {2, 33, 34, 50, 51, 67, 68, 100, 5, 40, 41, 90}),
        # only rows below 34: the later ranks' slices have no allowed row
        "ids_first_slice": ({"ids": [2, 33, 7, 8, 9]}, {2, 33, 7, 8, 9}),
        # fewer than top_k over all ranks
        "ids_few": ({"ids": [100, 2, 51]}, {100, 2, 51}),
        "exclude": ({"exclude_ids": list(range(3, 99))}, {0, 1, 2, 99, 100}),
        # labels 7 .. 10 are rows 70 .. 100: rank 0 has no allowed row (world 2 and 3)
        "range_last_slice": ({"label_range": [7, 10]}, set(range(70, N))),
        "range_middle": ({"label_range": [3, 5]}, set(range(30, 60))),
        "labels": ({"labels": [0, 10, 5]}, set(range(0, 10)) | set(range(50, 60)) | {100}),
        "nothing": ({"label_range": [50, 60]}, set()),
    }
    out = {"world": ws, "cases": {}}
    for name, (flt, rows) in cases.items():
        got = map_search(dict(job, filter=flt))
        out["cases"][name] = {"dp": {k: got[k] for k in ("ids", "scores", "filter_rows")}, "ref": single(rows),
                              "world": got.get("dp_world_size"), "rows": got["corpus_rows"],
                              "keys": sorted(k for k in got if k not in TIMING)}
    plain = map_search(dict(job))
    out["plain_keys"] = sorted(k for k in plain if k not in TIMING)
    s, i = ops.sim_topk_ref(q, c, 8)
    out["plain"] = {"dp": {"ids": plain["ids"], "scores": plain["scores"]}, "ref": {"ids": i.tolist(), "scores": s.tolist()}}
    # the same input error on every rank keeps its type and message
    errs = {}
    for name, extra in (("ids", {"filter": {"ids": [N]}}),
                        ("file", {"filter": {"labels": [1]}, "corpus_labels_uri": cpath})):
        try:
            map_search(dict(job, **extra))
            errs[name] = None
        except Exception as exc:
            errs[name] = [type(exc).__name__, str(exc)]
    out["errors"] = {"got": errs, "want": {"ids": ["ValueError", FILTER_ERRORS["filter_ids"].format(key="ids")],
                                           "file": ["ValueError", FILTER_ERRORS["labels_file"]]}}
    # through the lease batch handler (query_vectors jobs ride along on the single-job path)
    res = map_search_batch([dict(job, filter={"ids": [2, 51, 100]}), dict(job, filter={"label_range": [7, 10]}, top_k=3)])
    out["batch"] = {"kinds": [r[0] for r in res],
                    "ids": [r[1]["ids"] for r in res], "rows": [r[1]["filter_rows"] for r in res]}
    dp_ops.shutdown_workers()
    return out


def main():
    dist.init_process_group("gloo")
    try:
        res = scenario()
    finally:
        if dist.is_initialized():
            dist.destroy_process_group()
    if int(os.environ.get("RANK", "0")) == 0:
        print("RESULT " + json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
