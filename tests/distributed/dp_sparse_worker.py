"""Rank body of the map_sparse_embed DP test: rank 0 runs the op and prints one ``RESULT {json}`` line, the others serve."""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402

from agent_tpu_amd.parallel import dp, dp_ops  # noqa: E402

MODEL = "bert-tiny?mlm=1&batch=4&seq=40&seed=6"


def scenario():
    if dp.world()[0] != 0:
        dp_ops.worker_loop()
        return None
    from agent_tpu_amd.models.bert import config_for, init_random
    from agent_tpu_amd.runtime.classify import ClassifyEngine
    from ops.map_sparse_embed import map_sparse_embed

    cfg = config_for("bert-tiny", mlm_head=True)
    eng = ClassifyEngine(cfg, init_random(cfg, seed=6), torch.device("cpu"), batch_rows=4, seq_len=40)
    texts = [f"text {i} naïve café " + "lorem dolor " * (i % 4) for i in range(11)]  # 11 rows split 6 + 5
    got = map_sparse_embed({"texts": texts, "model_path": MODEL, "max_terms": 12})
    terms, nnz = eng.sparse_texts(texts, 12)
    one = map_sparse_embed({"text": texts[3], "model_path": MODEL, "max_terms": 12})  # the other rank's slice is empty
    dp_ops.shutdown_workers()
    return {"got": got, "one": one, "ref": {"terms": terms, "nnz": nnz}}


if __name__ == "__main__":
    dist.init_process_group("gloo")
    try:
        res = scenario()
    finally:
        if dist.is_initialized():
            dist.destroy_process_group()
    if int(os.environ.get("RANK", "0")) == 0:
        print("RESULT " + json.dumps(res), flush=True)
