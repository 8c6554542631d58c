"""Rank body of the map_rerank DP test (launched by torch.distributed.run, gloo, CPU engines via
CLASSIFY_DEVICE=cpu): rank 0 runs the op, the others serve in ``worker_loop``. Rank 0 prints one
``RESULT {json}`` line with the DP results next to single-process ones on the same pairs."""
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, REPO)

import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402

from agent_tpu_amd.parallel import dp, dp_ops  # noqa: E402

MODEL = "bert-tiny?labels=1&batch=4&seq=32&seed=6"


def fault():
    """``MI355X_FAULT=rank:1:rerank:1``: rank 1 raises in its first rerank job only."""
    from ops.map_rerank import map_rerank

    out = {}
    try:
        map_rerank({"query": "q", "passages": ["p", "r", "s"], "model_path": MODEL})
        out["err"] = None
    except Exception as exc:
        out["err"] = [type(exc).__name__, str(exc)]
    got = map_rerank({"query": "q", "passages": ["p", "r", "s"], "model_path": MODEL})  # the group still serves
    out["after"] = [got["pair_count"], got["dp_world_size"], len(got["ranked"][0])]
    dp_ops.shutdown_workers()
    return out


def scenario():
    rank, ws = dp.world()
    if rank != 0:
        dp_ops.worker_loop()
        return None
    if sys.argv[1:] == ["fault"]:
        return fault()
    from agent_tpu_amd.models.bert import config_for, init_random
    from agent_tpu_amd.runtime.classify import ClassifyEngine
    from ops.map_rerank import ERRORS, map_rerank, map_rerank_batch

    cfg = config_for("bert-tiny", num_labels=1)
    eng = ClassifyEngine(cfg, init_random(cfg, seed=6), torch.device("cpu"), batch_rows=4, seq_len=32)
    out = {"world": ws}
    queries = ["alpha beta gamma", "lorem ipsum", "unused", "dolor sit amet consectetur"]
    groups = [[f"passage {i} " + "lorem ipsum dolor " * (i % 3) for i in range(5)], ["ipsum", "amet sit"], [],
              [f"text {i}" for i in range(4)]]  # 11 pairs: 6 + 5, the split falls inside the last group
    flat = [p for g in groups for p in g]
    goff = [0, 5, 7, 7, 11]

    def ref(k):
        r = eng.rerank_pairs(queries, flat, goff, top_k=k)
        return {"idx": r.idx.tolist(), "scores": r.scores.tolist()}

    got = map_rerank({"queries": queries, "passages": groups, "model_path": MODEL, "top_k": 3, "return_scores": True})
    out["many"] = {"ranked": got["ranked"], "scores": got["scores"], "world": got["dp_world_size"],
                   "pairs": got["pair_count"], "ref": ref(3)}
    # one pair: rank 1's slice is empty
    got = map_rerank({"query": queries[0], "passages": flat[:1], "model_path": MODEL, "return_scores": True})
    one = eng.rerank_pairs(queries[:1], flat[:1], [0, 1])
    out["one"] = {"ranked": got["ranked"], "scores": got["scores"], "ref": one.scores.tolist()}
    # the same input error on every rank keeps its type and message
    try:
        map_rerank({"query": "q", "passages": ["p"], "model_path": MODEL, "label": 3})
        out["bad"] = None
    except Exception as exc:
        out["bad"] = [type(exc).__name__, str(exc), ERRORS["label"]]
    res = map_rerank_batch([{"queries": queries[:2], "passages": groups[:2], "model_path": MODEL, "top_k": 3,
                             "return_scores": True},
                            {"query": 5, "passages": [], "model_path": MODEL},
                            {"queries": queries[2:], "passages": groups[2:], "model_path": MODEL, "top_k": 2,
                             "return_scores": True}])
    out["batch"] = {"kinds": [r[0] for r in res], "scores": res[0][1]["scores"] + res[2][1]["scores"],
                    "idx": [[e["index"] for e in x] for x in res[0][1]["ranked"] + res[2][1]["ranked"]]}
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
