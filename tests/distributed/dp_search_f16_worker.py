"""Rank body of the float16 map_search DP test (launched by torch.distributed.run, gloo, CPU engines
via CLASSIFY_DEVICE=cpu): rank 0 runs the op with ``corpus_dtype: "float16"``, the others serve in
``worker_loop``. Rank 0 prints one ``RESULT {json}`` line with the DP results next to
single-process ones (the twin over the whole fp16 corpus and its row scale) on the same data."""
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
    from agent_tpu_amd.runtime.search import EPS, normalize_rows
    from ops.map_search import map_search

    out = {"world": ws}
    tmp = os.environ["DP_TEST_DIR"]
    # 37 rows of different norms: rank 0 holds rows 0 .. 18, rank 1 rows 19 .. 36; rows 17 .. 20 are one
    # vector (ties across the boundary), rows 5 and 30 another
    gen = torch.Generator().manual_seed(7)
    rows = torch.randn(37, 64, generator=gen) * torch.linspace(0.5, 3.0, 37).unsqueeze(1)
    rows[17:21] = rows[17]
    rows[30] = rows[5]
    queries = torch.cat([rows[18:19], rows[5:6], torch.randn(3, 64, generator=gen)])
    for name, arr in (("f16", rows.half().numpy()), ("f32", rows.numpy())):
        path = os.path.join(tmp, f"corpus_{name}.npy")
        np.save(path, arr)
        c16 = rows.half()  # the resident rows of both files
        for metric in ("cosine", "dot"):
            got = map_search({"query_vectors": queries.tolist(), "corpus_uri": path, "top_k": 8, "metric": metric,
                              "corpus_dtype": "float16"})
            if metric == "cosine":
                scale = c16.double().norm(dim=1).clamp_min(EPS).reciprocal().float()
                s, i = ops.sim_topk_ref(normalize_rows(queries), c16, 8, row_scale=scale)
            else:
                s, i = ops.sim_topk_ref(queries, c16, 8)
            out[f"{name}_{metric}"] = {"dp": {"ids": got["ids"], "scores": got["scores"]},
                                       "ref": {"ids": i.tolist(), "scores": s.tolist()},
                                       "world": got.get("dp_world_size"), "rows": got["corpus_rows"],
                                       "cached": got["index_cached"], "corpus_dtype": got.get("corpus_dtype")}
    again = map_search({"query_vectors": queries.tolist(), "corpus_uri": path, "top_k": 8, "metric": "dot",
                        "corpus_dtype": "float16"})
    out["again_cached"] = again["index_cached"]
    plain = map_search({"query_vectors": queries.tolist(), "corpus_uri": path, "top_k": 8, "metric": "dot"})
    out["plain_keys"] = sorted(plain)
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
