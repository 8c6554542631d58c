"""Rank body of the ``diversify`` map_search DP test (launched by torch.distributed.run, gloo, CPU engines via
CLASSIFY_DEVICE=cpu): rank 0 runs the op, the others serve in ``worker_loop``. Rank 0 prints one ``RESULT {json}``
line with the DP results next to single-process ones (the twins over the whole resident corpus) on the same data."""
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
    from agent_tpu_amd.runtime import search as rs
    from ops.map_search import map_search

    out = {"world": ws}
    # 37 rows of different norms, every row of 0 .. 11 three times: rank 0 holds rows 0 .. 18, rank 1 rows 19 .. 36
    gen = torch.Generator().manual_seed(7)
    rows = (torch.randn(12, 64, generator=gen)[torch.arange(37) % 12] * torch.linspace(0.5, 3.0, 37).unsqueeze(1))
    queries = torch.cat([rows[18:19], rows[5:6], torch.randn(3, 64, generator=gen)])
    path = os.path.join(os.environ["DP_TEST_DIR"], "corpus.npy")
    np.save(path, rows.numpy())
    dv = {"lambda": 0.25, "candidates": 16}
    for dtype, metric in (("float32", "cosine"), ("float16", "cosine"), ("float16", "dot")):
        got = map_search({"query_vectors": queries.tolist(), "corpus_uri": path, "top_k": 6, "metric": metric,
                          "corpus_dtype": dtype, "diversify": dv})
        q = rs.normalize_rows(queries) if metric == "cosine" else queries
        if dtype == "float32":
            vec, scale = rs.normalize_rows(rows), None
        else:
            vec = rows.half()
            scale = vec.double().norm(dim=1).clamp_min(rs.EPS).reciprocal().float() if metric == "cosine" else None
        s, i = ops.sim_topk_ref(q, vec, 16, row_scale=scale)
        pi, ps, pm = ops.mmr_select_ref(s, i.to(torch.int32), vec, 6, 0.25, row_scale=scale)
        out[f"{dtype}_{metric}"] = {"dp": {k: got[k] for k in ("ids", "scores", "mmr_scores")},
                                    "ref": {"ids": pi.tolist(), "scores": ps.tolist(), "mmr_scores": pm.tolist()},
                                    "plain": i[:, :6].tolist(), "world": got.get("dp_world_size"),
                                    "diversify": got["diversify"]}
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
