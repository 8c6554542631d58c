"""Rank body of the map_tag DP test (launched by torch.distributed.run, gloo, CPU engines via
CLASSIFY_DEVICE=cpu): rank 0 runs the op, the others serve in ``worker_loop``. Rank 0 prints one
``RESULT {json}`` line with the DP results next to single-process ones on the same texts."""
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, REPO)

import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402

from agent_tpu_amd.parallel import dp, dp_ops  # noqa: E402

MODEL = "bert-tiny?tags=5&batch=4&seq=40&seed=6"


def fault():
    """``MI355X_FAULT=rank:1:tag:1``: rank 1 raises in its first tag job only."""
    from ops.map_tag import map_tag

    out = {}
    try:
        map_tag({"texts": ["p one", "r two", "s three"], "model_path": MODEL})
        out["err"] = None
    except Exception as exc:
        out["err"] = [type(exc).__name__, str(exc)]
    got = map_tag({"texts": ["p one", "r two", "s three"], "model_path": MODEL})  # still serves
    out["after"] = [got["row_count"], got["dp_world_size"], len(got["entities"])]
    dp_ops.shutdown_workers()
    return out


def _keys(entities, name="entity_group"):
    return [[[e[name], e["start"], e["end"], e["word"]] for e in row] for row in entities]


def _scores(entities):
    return [e["score"] for row in entities for e in row]


def scenario():
    rank, ws = dp.world()
    if rank != 0:
        dp_ops.worker_loop()
        return None
    if sys.argv[1:] == ["fault"]:
        return fault()
    from agent_tpu_amd.models.bert import config_for, init_random
    from agent_tpu_amd.runtime.classify import ClassifyEngine
    from ops.map_tag import ERRORS, map_tag, map_tag_batch

    cfg = config_for("bert-tiny", tag_labels=5)
    eng = ClassifyEngine(cfg, init_random(cfg, seed=6), torch.device("cpu"), batch_rows=4, seq_len=40)
    out = {"world": ws}
    texts = [f"text {i} naïve café " + "lorem ipsum dolor " * (i % 4) for i in range(10)] + [""]  # 11 rows

    got = map_tag({"texts": texts, "model_path": MODEL, "max_entities": 4})
    ref = eng.tag_texts(texts, "simple", 4)
    out["many"] = {"keys": _keys(got["entities"]), "scores": _scores(got["entities"]), "counts": got["entity_counts"],
                   "truncated": got["truncated"], "world": got["dp_world_size"], "rows": got["row_count"],
                   "ref": {"keys": _keys(ref.entities), "scores": _scores(ref.entities), "counts": ref.counts,
                           "truncated": ref.truncated}}
    # one row: the other ranks' slices are empty
    got = map_tag({"text": texts[3], "model_path": MODEL, "aggregation": "none"})
    one = eng.tag_texts(texts[3:4], "none", 64)
    out["one"] = {"keys": _keys(got["entities"], "entity"), "ref_keys": _keys(one.entities, "entity"),
                  "counts": got["entity_counts"], "ref_counts": one.counts}
    # the same input error on every rank keeps its type and message
    try:
        map_tag({"text": "q", "model_path": MODEL, "aggregation": "first"})
        out["bad"] = None
    except Exception as exc:
        out["bad"] = [type(exc).__name__, str(exc), ERRORS["vocab"]]
    res = map_tag_batch([{"texts": texts[:5], "model_path": MODEL, "max_entities": 4},
                         {"text": 5, "model_path": MODEL},
                         {"texts": texts[5:], "model_path": MODEL, "max_entities": 4}])
    out["batch"] = {"kinds": [r[0] for r in res], "keys": _keys(res[0][1]["entities"] + res[2][1]["entities"])}
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
