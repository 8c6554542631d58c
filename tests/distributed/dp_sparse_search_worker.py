"""Rank body of the map_sparse_search DP test (torch.distributed.run, gloo, CPU engines): rank 0 runs the op, the
others serve in ``worker_loop``, and rank 0 prints one ``RESULT {json}`` line. ``DP_SPARSE_SINGLE=1``: the same jobs
without a process group. The corpus is test_sparse_search_cpu.py's seeded matrix (9000 x 50: two blocks, the ranks'
slices of 4500 rows cut the first one)."""
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests", "contract"))

import torch.distributed as dist  # noqa: E402

from agent_tpu_amd.parallel import dp, dp_ops  # noqa: E402
from test_sparse_search_cpu import MODEL, _save, matrix  # noqa: E402


def run_jobs(tmp):
    from ops import get_batch_op, get_op

    path = os.path.join(tmp, "c.npz")
    if not os.path.exists(path):
        _save(path, matrix())
    terms = [{"token_ids": [2], "weights": [1.0]}, {"token_ids": [7, 3, 11, 40], "weights": [0.3, 1.7, 2.5, 0.9]},
             {"token_ids": [], "weights": []}]
    job = {"corpus_uri": path, "query_terms": terms, "top_k": 32}
    run = get_op("map_sparse_search")
    out = {"terms": run(dict(job)), "batch": [r for _, r in get_batch_op("map_sparse_search")([dict(job, top_k=5), dict(job)])]}
    texts = os.path.join(tmp, "texts.npz")
    if not os.path.exists(texts):
        get_op("map_sparse_embed")({"texts": [f"passage number {i} about topic {i % 5}" for i in range(20)],
                                    "model_path": MODEL, "output": "npz", "output_uri": texts})
    out["texts"] = run({"corpus_uri": texts, "queries": ["passage number 3 about topic 3", "topic"], "model_path": MODEL,
                        "top_k": 4})
    return out


def main():
    if os.environ.get("DP_SPARSE_SINGLE"):
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
