"""Rank body of the map_embed DP test (launched by torch.distributed.run, gloo, CPU engines via
CLASSIFY_DEVICE=cpu): rank 0 runs the op, the others serve in ``worker_loop``. Rank 0 prints one
``RESULT {json}`` line with the DP results next to single-process ones on the same rows."""
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, REPO)

import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402

from agent_tpu_amd.parallel import dp, dp_ops  # noqa: E402

MODEL = "bert-tiny?batch=4&seq=32&seed=6"


def scenario():
    rank, ws = dp.world()
    if rank != 0:
        dp_ops.worker_loop()
        return None
    from agent_tpu_amd.io.csv import open_csv
    from agent_tpu_amd.models.bert import config_for, init_random
    from agent_tpu_amd.runtime.classify import ClassifyEngine
    from ops.map_embed import ERRORS, map_embed, map_embed_batch

    cfg = config_for("bert-tiny")
    eng = ClassifyEngine(cfg, init_random(cfg, seed=6), torch.device("cpu"), batch_rows=4, seq_len=32)
    out = {"world": ws}
    texts = [f"row {i} " + "lorem ipsum dolor sit amet " * (i % 4) for i in range(7)]  # odd: 4 + 3
    got = map_embed({"texts": texts, "model_path": MODEL, "pooling": "mean"})
    out["texts"] = {"dp": got["embeddings"], "ref": eng.embed_texts(texts).emb.tolist(),
                    "world": got["dp_world_size"], "rows": got["row_count"]}
    path = os.environ["DP_TEST_CSV"]
    tab = open_csv(path)
    col = tab.native.column_index("text")
    rows = [tab.native.row(i)[col] for i in range(2, 13)]  # 11 rows: 6 + 5
    got = map_embed({"source_uri": path, "start_row": 2, "shard_size": 11, "model_path": MODEL, "pooling": "cls",
                     "normalize": False})
    out["csv"] = {"dp": got["embeddings"], "ref": eng.embed_texts(rows, "cls", False).emb.tolist(),
                  "world": got["dp_world_size"], "rows": got["row_count"], "end_row": got["end_row"]}
    # one row: rank 1's shard is empty
    got = map_embed({"texts": texts[:1], "model_path": MODEL})
    out["one"] = {"dp": got["embeddings"], "ref": eng.embed_texts(texts[:1]).emb.tolist()}
    # the same input error on every rank keeps its type and message
    try:
        map_embed({"source_uri": path, "text_column": "nope", "model_path": MODEL})
        out["bad"] = None
    except Exception as exc:
        out["bad"] = [type(exc).__name__, str(exc), ERRORS["column"]]
    res = map_embed_batch([{"texts": texts[:3], "model_path": MODEL}, {"texts": 5, "model_path": MODEL},
                           {"texts": texts[3:], "model_path": MODEL}])
    out["batch"] = {"kinds": [r[0] for r in res], "dp": res[0][1]["embeddings"] + res[2][1]["embeddings"]}
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
