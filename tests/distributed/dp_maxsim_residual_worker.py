"""Rank body of the residual-index DP test (torch.distributed.run, gloo, CPU engines): rank 0 builds a
residual-compressed index through the op and queries it, the others serve in ``worker_loop``. Rank 0 prints one
``RESULT {json}`` line; the world-1 run of the same file is the reference."""
import json
import os
import shutil
import sys
import tempfile

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, REPO)

import torch.distributed as dist  # noqa: E402

from agent_tpu_amd.parallel import dp, dp_ops  # noqa: E402

MODEL = "bert-tiny?late=64&batch=4&seq=32&seed=6"


def scenario(tmp):
    rank, ws = dp.world()
    if rank != 0:
        dp_ops.worker_loop()
        return None
    from agent_tpu_amd.runtime import maxsim_residual as mr
    from ops.map_maxsim import map_maxsim

    queries = ["alpha beta gamma", "lorem ipsum", "dolor sit amet consectetur"]
    pool = [f"passage {i} " + "lorem ipsum dolor " * (i % 3) for i in range(5)] + ["ipsum", "amet sit"]  # 7 passages
    uri = os.path.join(tmp, "rc.npy")
    b = map_maxsim({"passages": pool, "model_path": MODEL,
                    "index_out": {"uri": uri, "compression": {"type": "residual", "bits": 2, "centroids": 4}}})
    files = [uri, b["offsets_uri"]] + [mr.companion(uri, k) for k in ("cids", "centroids", "weights")]
    out = {"world": ws, "build": {k: b[k] for k in ("passage_count", "token_count", "bits", "centroids", "bytes", "dtype")},
           "files": [open(f, "rb").read().hex() for f in files]}
    whole = map_maxsim({"queries": queries, "index_uri": uri, "model_path": MODEL, "top_k": 3})
    cand = map_maxsim({"queries": queries, "index_uri": uri, "candidates": [[6, 0, 3, 2], [], [1, 5, 4]],
                       "model_path": MODEL, "top_k": 3, "return_scores": True})
    out["whole"] = [whole["ranked"], whole["index_dtype"], whole["pair_count"], whole.get("dp_world_size", 1)]
    out["cand"] = [cand["ranked"], cand["scores"], cand["pair_count"]]
    dp_ops.shutdown_workers()
    return out


def main():
    dist.init_process_group("gloo")
    tmp = tempfile.mkdtemp(prefix="dp_maxsim_residual_") if int(os.environ.get("RANK", "0")) == 0 else None
    try:
        res = scenario(tmp)
    finally:
        if dist.is_initialized():
            dist.destroy_process_group()
        if tmp is not None:
            shutil.rmtree(tmp, ignore_errors=True)
    if int(os.environ.get("RANK", "0")) == 0:
        print("RESULT " + json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
