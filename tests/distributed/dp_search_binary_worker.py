"""Rank body of the binary map_search DP test (torch.distributed.run, gloo, CPU engines): rank 0 runs the op, the
others serve in ``worker_loop``, and rank 0 prints one ``RESULT {json}`` line. ``DP_BINARY_SINGLE=1``: the same jobs
without a process group. The corpus is test_search_binary_cpu.py's seeded mixture at 4096 x 64."""
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests", "contract"))

import numpy as np  # noqa: E402
import torch.distributed as dist  # noqa: E402

from agent_tpu_amd.parallel import dp, dp_ops  # noqa: E402
from test_search_binary_cpu import BIN, mixture  # noqa: E402


def run_jobs(tmp):
    from ops.map_search import map_search

    q, x = mixture(4096, 64, 64)
    path = os.path.join(tmp, "mix.npy")
    if not os.path.exists(path):
        np.save(path, x.numpy())
    job = {"query_vectors": q.tolist(), "corpus_uri": path, "top_k": 5}
    jobs = {"exact": job, "zero": dict(job, top_k=32, compression=BIN),
            "mean": dict(job, compression=dict(BIN, threshold="mean")),
            "refined": dict(job, compression=BIN, refine={"candidates": 256, "vectors": "float32"})}
    out = {}
    for name, payload in jobs.items():
        r = map_search(dict(payload))
        out[name] = {k: r.get(k) for k in ("ids", "scores", "compression", "refine", "corpus_rows", "top_k")}
        out[name]["world"] = r.get("dp_world_size", 1)
    return out


def main():
    if os.environ.get("DP_BINARY_SINGLE"):
        print("RESULT " + json.dumps(run_jobs(os.environ["DP_TEST_DIR"])), flush=True)
        return
    dist.init_process_group("gloo")
    try:
        res = None
        if dp.world()[0] != 0:
            dp_ops.worker_loop()
        else:
            res = run_jobs(os.environ["DP_TEST_DIR"])
            dp_ops.shutdown_workers()
    finally:
        if dist.is_initialized():
            dist.destroy_process_group()
    if res is not None:
        print("RESULT " + json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
