"""Rank body of the map_search ``depth`` DP test (torch.distributed.run, gloo, CPU): rank 0 runs the op with
``query_vectors``, the other rank serves in ``worker_loop``. Rank 0 prints one ``RESULT {json}`` line with the DP
results next to ``sim_topk_ref`` on the whole corpus."""
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


def scenario():
    rank, ws = dp.world()
    if rank != 0:
        dp_ops.worker_loop()
        return None
    from ops.map_search import map_search

    out = {"world": ws}
    gen = torch.Generator().manual_seed(11)
    base = torch.randint(-2, 3, (120, 64), generator=gen).float()
    q = torch.randint(-2, 3, (3, 64), generator=gen).float()
    # rows: 150 -> slices of 75 (shorter than the depth), 300 -> slices of 150 (longer); duplicated rows tie
    # across the rank boundary
    for rows in (150, 300):
        c = base[torch.randint(0, 120, (rows,), generator=gen)].contiguous()
        path = os.path.join(os.environ["DP_TEST_DIR"], f"corpus{rows}.npy")
        np.save(path, c.numpy())
        got = map_search({"query_vectors": q.tolist(), "corpus_uri": path, "depth": 100, "metric": "dot"})
        s, i = ops.sim_topk_ref(q, c, 100)
        out[str(rows)] = {"dp": {"ids": got["ids"], "scores": got["scores"]}, "depth": got["depth"],
                          "world": got.get("dp_world_size"), "ref": {"ids": i.tolist(), "scores": s.tolist()}}
    dp_ops.shutdown_workers()
    return out


if __name__ == "__main__":
    dist.init_process_group("gloo")
    try:
        res = scenario()
    finally:
        if dist.is_initialized():
            dist.destroy_process_group()
    if res is not None:
        print("RESULT " + json.dumps(res), flush=True)
