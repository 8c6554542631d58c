"""Rank body of the map_dedup DP test (launched by torch.distributed.run, gloo, CPU engines via
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
from agent_tpu_amd.runtime import dedup as rd  # noqa: E402

TIMING = ("elapsed_ms", "rows_per_sec", "index_cached", "dp_world_size")
rd.BLOCK_ROWS = 16  # 101 rows: seven blocks, so every rank of a world of 2 or 3 joins some (every rank imports this file)


def data():
    """101 rows (not divisible by 2 or 3) of 64 columns: random rows, planted copies on both sides of the block
    and rank boundaries, near-copies and a chain."""
    gen = torch.Generator().manual_seed(12)
    x = torch.randn(101, 64, generator=gen)
    x[50] = x[49]
    x[51] = x[49]
    x[100] = x[0]
    x[15] = x[16] + 0.05 * torch.randn(64, generator=gen)
    for i in range(30, 36):  # a chain of near-copies: one group by single linkage
        x[i + 1] = x[i] + 0.1 * torch.randn(64, generator=gen)
    return x.contiguous()


def jobs(tmp):
    path = os.path.join(tmp, "vec.npy")
    if not os.path.exists(path):
        np.save(path, data().numpy())
    return {"cosine": {"vectors_uri": path, "threshold": 0.95, "max_pairs": 40},
            "dot": {"vectors_uri": path, "threshold": 20.0, "metric": "dot", "max_pairs": 65536},
            "vectors": {"vectors": data()[:40].tolist(), "threshold": 0.5, "output": "summary", "max_pairs": 5},
            "none": {"vectors": data()[:20].tolist(), "threshold": 1.5}}


def run_jobs(tmp):
    from ops.map_dedup import map_dedup

    out = {}
    for name, payload in jobs(tmp).items():
        r = map_dedup(dict(payload))
        out[name] = {k: v for k, v in r.items() if k not in TIMING}
        out[name]["world"] = r["dp_world_size"]
    return out


def scenario():
    rank, ws = dp.world()
    if rank != 0:
        dp_ops.worker_loop()
        return None
    from ops.map_dedup import ERRORS, map_dedup

    tmp = os.environ["DP_TEST_DIR"]
    if os.environ.get("DP_DEDUP_FAULT"):
        try:
            map_dedup(dict(jobs(tmp)["cosine"]))
            out = {"fault": None}
        except Exception as exc:
            out = {"fault": [type(exc).__name__, str(exc)]}
        dp_ops.shutdown_workers()
        return out
    out = run_jobs(tmp)
    bad = os.path.join(tmp, "odd.npy")
    np.save(bad, np.ones((5, 96), dtype=np.float32))
    try:  # the same input error on every rank (found after the load) keeps its type and message
        map_dedup({"vectors_uri": bad, "threshold": 0.5})
        out["bad"] = None
    except Exception as exc:
        out["bad"] = [type(exc).__name__, str(exc), ERRORS["dim"]]
    again = map_dedup(dict(jobs(tmp)["none"]))  # the group survives a failed job
    out["after_bad"] = again["pair_count"]
    dp_ops.shutdown_workers()
    return out


def main():
    if os.environ.get("DP_DEDUP_SINGLE"):  # the single-process reference: no process group
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
