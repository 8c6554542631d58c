"""Rank body of the map_search DP test (launched by torch.distributed.run, gloo, CPU engines via
CLASSIFY_DEVICE=cpu): rank 0 runs the op, the others serve in ``worker_loop``. Rank 0 prints one
``RESULT {json}`` line with the DP results next to single-process ones on the same data."""
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

MODEL = "bert-tiny?batch=4&seq=32&seed=6"


def scenario():
    rank, ws = dp.world()
    if rank != 0:
        dp_ops.worker_loop()
        return None
    from agent_tpu_amd.models.bert import config_for, init_random
    from agent_tpu_amd.runtime.classify import ClassifyEngine
    from agent_tpu_amd.runtime.search import normalize_rows
    from ops.map_search import ERRORS, map_search, map_search_batch

    cfg = config_for("bert-tiny")
    eng = ClassifyEngine(cfg, init_random(cfg, seed=6), torch.device("cpu"), batch_rows=4, seq_len=32)
    out = {"world": ws}
    tmp = os.environ["DP_TEST_DIR"]
    # 37 rows: rank 0 holds rows 0 .. 18, rank 1 rows 19 .. 36; rows 17 .. 20 are one text (ties
    # across the boundary), rows 5 and 30 another
    texts = [f"row {i} " + "lorem ipsum dolor sit amet " * (i % 4) for i in range(37)]
    for i in (17, 18, 19, 20):
        texts[i] = "the same sentence on both sides of the boundary"
    texts[30] = texts[5]
    corpus = eng.embed_texts(texts, "mean", False).emb
    path = os.path.join(tmp, "corpus.npy")
    np.save(path, corpus.numpy())
    queries = [texts[18], texts[5], texts[0], "something else entirely", texts[36]]

    def single(qs, rows, k, metric):
        q = eng.embed_texts(qs, "mean", metric == "cosine").emb
        c = normalize_rows(rows) if metric == "cosine" else rows
        s, i = ops.sim_topk_ref(q, c, k)
        return {"ids": i.tolist(), "scores": s.tolist()}

    for metric in ("cosine", "dot"):
        got = map_search({"queries": queries, "corpus_uri": path, "model_path": MODEL, "top_k": 8, "metric": metric})
        out[metric] = {"dp": {"ids": got["ids"], "scores": got["scores"]}, "ref": single(queries, corpus, 8, metric),
                       "world": got.get("dp_world_size"), "rows": got["corpus_rows"], "cached": got["index_cached"]}
    # a top_k larger than one rank's slice: 9 rows are 5 + 4
    small = os.path.join(tmp, "small.npy")
    np.save(small, corpus[:9].numpy())
    got = map_search({"queries": queries, "corpus_uri": small, "model_path": MODEL, "top_k": 8})
    out["small"] = {"dp": {"ids": got["ids"], "scores": got["scores"]}, "ref": single(queries, corpus[:9], 8, "cosine")}
    # fewer rows than ranks: rank 1's slice is empty
    one = os.path.join(tmp, "one.npy")
    np.save(one, corpus[:1].numpy())
    got = map_search({"queries": queries[:2], "corpus_uri": one, "model_path": MODEL, "top_k": 8})
    out["one"] = {"dp": {"ids": got["ids"], "scores": got["scores"]}, "ref": single(queries[:2], corpus[:1], 8, "cosine")}
    # corpus_texts and query_vectors forms
    got = map_search({"queries": queries, "corpus_texts": texts, "model_path": MODEL, "top_k": 8})
    out["texts"] = {"ids": got["ids"]}
    got = map_search({"query_vectors": corpus[:3].tolist(), "corpus_uri": path, "top_k": 2, "metric": "dot"})
    s, i = ops.sim_topk_ref(corpus[:3], corpus, 2)
    out["vectors"] = {"dp": {"ids": got["ids"], "scores": got["scores"]}, "ref": {"ids": i.tolist(), "scores": s.tolist()}}
    # the same input error on every rank keeps its type and message
    bad = os.path.join(tmp, "bad.npy")
    np.save(bad, np.zeros((4, 64), dtype=np.float32))
    try:
        map_search({"queries": queries, "corpus_uri": bad, "model_path": MODEL})
        out["bad"] = None
    except Exception as exc:
        out["bad"] = [type(exc).__name__, str(exc), ERRORS["dim"]]
    res = map_search_batch([{"queries": queries[:2], "corpus_uri": path, "model_path": MODEL, "top_k": 3},
                            {"queries": 5, "corpus_uri": path, "model_path": MODEL},
                            {"queries": queries[2:], "corpus_uri": path, "model_path": MODEL, "top_k": 8}])
    out["batch"] = {"kinds": [r[0] for r in res], "ids": res[0][1]["ids"] + res[2][1]["ids"],
                    "scores": res[0][1]["scores"] + res[2][1]["scores"], "world": res[0][1].get("dp_world_size")}
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
