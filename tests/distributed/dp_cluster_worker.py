"""Rank body of the map_cluster DP test (launched by torch.distributed.run, gloo, CPU engines via
CLASSIFY_DEVICE=cpu): rank 0 runs the op, the others serve in ``worker_loop``. Rank 0 prints one
``RESULT {json}`` line; the test compares it with a single-process run of the same jobs."""
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, REPO)

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402

from agent_tpu_amd.parallel import dp, dp_ops  # noqa: E402

KEYS = ("labels", "centroids", "sizes", "objective", "iterations", "converged", "representatives")


def data():
    """101 rows (not divisible by 2 or 3) of 64 columns: three loose groups of random rows and duplicates."""
    gen = torch.Generator().manual_seed(12)
    centres = 3.0 * torch.randn(3, 64, generator=gen)
    x = centres[torch.randint(0, 3, (101,), generator=gen)] + torch.randn(101, 64, generator=gen)
    x[50] = x[49]  # equal rows on both sides of the world-2 boundary
    x[51] = x[49]
    return x.contiguous()


def jobs(tmp):
    path = os.path.join(tmp, "vec.npy")
    if not os.path.exists(path):
        np.save(path, data().numpy())
    return {"cosine": {"vectors_uri": path, "k": 5, "seed": 4, "representatives": 4},
            "l2": {"vectors_uri": path, "k": 5, "metric": "l2", "seed": 4, "representatives": 4},
            "vectors": {"vectors": data()[:40].tolist(), "k": 7, "metric": "l2", "seed": 1, "max_iter": 3},
            "k_rows": {"vectors": data()[:5].tolist(), "k": 5, "output": "rows"}}


def run_jobs(tmp):
    from ops.map_cluster import map_cluster

    out = {}
    for name, payload in jobs(tmp).items():
        r = map_cluster(dict(payload))
        out[name] = {k: r.get(k) for k in KEYS}
        out[name]["world"] = r["dp_world_size"]
    return out


def scenario():
    rank, ws = dp.world()
    if rank != 0:
        dp_ops.worker_loop()
        return None
    from ops.map_cluster import ERRORS, map_cluster

    tmp = os.environ["DP_TEST_DIR"]
    if os.environ.get("DP_CLUSTER_FAULT"):
        try:
            map_cluster(dict(jobs(tmp)["cosine"]))
            out = {"fault": None}
        except Exception as exc:
            out = {"fault": [type(exc).__name__, str(exc)]}
        dp_ops.shutdown_workers()
        return out
    out = run_jobs(tmp)
    try:  # the same input error on every rank keeps its type and message
        map_cluster({"vectors_uri": os.path.join(tmp, "vec.npy"), "k": 102})
        out["bad"] = None
    except Exception as exc:
        out["bad"] = [type(exc).__name__, str(exc), ERRORS["k_rows"]]
    dp_ops.shutdown_workers()
    return out


def main():
    if os.environ.get("DP_CLUSTER_SINGLE"):  # the single-process reference: no process group
        print("RESULT " + json.dumps(run_jobs(os.environ["DP_TEST_DIR"])), flush=True)
        return
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
