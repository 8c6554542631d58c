"""Rank body of the IVF-PQ map_search DP test (torch.distributed.run, gloo, CPU engines): rank 0 runs the op and prints
one ``RESULT {json}`` line, the others serve in ``worker_loop``; ``DP_IVFPQ_SINGLE=1`` runs without a process group.
The rows have sixteen +-1 entries, whose normalisation (a division by 4) is exact."""
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, REPO)

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402

from agent_tpu_amd.parallel import dp, dp_ops  # noqa: E402


def run_jobs(tmp):
    from ops.map_search import map_search

    gen = torch.Generator().manual_seed(13)
    c = torch.zeros(300, 64)  # slice starts 150 (world 2) and 100, 200 (world 3)
    for r in range(300):
        c[r, torch.randperm(64, generator=gen)[:16]] = torch.randint(0, 2, (16,), generator=gen).float() * 2 - 1
    c[[99, 100, 149, 150, 199, 200]] = c[2].clone()  # one vector on both sides of every slice boundary: ties across ranks
    path = os.path.join(tmp, "signs.npy")
    if not os.path.exists(path):
        np.save(path, c.numpy())
    ix = {"type": "ivfpq", "subvectors": 16, "clusters": 5, "nprobe": 2, "train_rows": 256, "train_iterations": 4}
    job = {"query_vectors": torch.cat([c[2:3], c[40:44]]).tolist(), "corpus_uri": path, "top_k": 8, "index": ix}
    jobs = {"two": job, "all": dict(job, top_k=32, index=dict(ix, nprobe=5)), "again": dict(job, top_k=3)}
    out = {}
    for name, payload in jobs.items():
        r = map_search(dict(payload))
        out[name] = {k: r.get(k) for k in ("ids", "scores", "index", "corpus_rows", "top_k", "index_cached")}
        out[name]["world"] = r.get("dp_world_size", 1)
    return out


def main():
    if os.environ.get("DP_IVFPQ_SINGLE"):
        print("RESULT " + json.dumps(run_jobs(os.environ["DP_TEST_DIR"])), flush=True)
        return
    dist.init_process_group("gloo")
    try:
        rank, ws = dp.world()
        res = None
        if rank != 0:
            dp_ops.worker_loop()
        else:
            res = run_jobs(os.environ["DP_TEST_DIR"])
            dp_ops.shutdown_workers()
    finally:
        if dist.is_initialized():
            dist.destroy_process_group()
    if rank == 0:
        print("RESULT " + json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
