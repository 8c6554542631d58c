"""Rank body of the map_fill DP test (launched by torch.distributed.run, gloo, CPU engines via
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

MODEL = "bert-tiny?mlm=1&batch=4&seq=40&seed=6"


def fault():
    """``MI355X_FAULT=rank:1:fill:1``: rank 1 raises in its first fill job only."""
    from ops.map_fill import map_fill

    out = {}
    texts = ["p [MASK]", "r [MASK] two", "[MASK] three"]
    try:
        map_fill({"texts": texts, "model_path": MODEL})
        out["err"] = None
    except Exception as exc:
        out["err"] = [type(exc).__name__, str(exc)]
    got = map_fill({"texts": texts, "model_path": MODEL})  # still serves
    out["after"] = [got["row_count"], got["dp_world_size"], len(got["fills"])]
    dp_ops.shutdown_workers()
    return out


def _keys(fills):
    return [[[m["start"], m["end"], [c["token_id"] for c in m["candidates"]]] for m in row] for row in fills]


def _scores(fills):
    return [c["score"] for row in fills for m in row for c in m["candidates"]]


def scenario():
    rank, ws = dp.world()
    if rank != 0:
        dp_ops.worker_loop()
        return None
    if sys.argv[1:] == ["fault"]:
        return fault()
    from agent_tpu_amd.models.bert import config_for, init_random
    from agent_tpu_amd.runtime.classify import ClassifyEngine
    from ops.map_fill import ERRORS, map_fill, map_fill_batch

    cfg = config_for("bert-tiny", mlm_head=True)
    eng = ClassifyEngine(cfg, init_random(cfg, seed=6), torch.device("cpu"), batch_rows=4, seq_len=40)
    out = {"world": ws}
    texts = [f"text {i} naïve [MASK] café " + "lorem [MASK] dolor " * (i % 4) for i in range(10)]
    texts.append("word " * 60 + "[MASK]")  # 11 rows; the last row's mask falls beyond the row

    got = map_fill({"texts": texts, "model_path": MODEL, "top_k": 4})
    ref = eng.fill_texts(texts, 4)
    out["many"] = {"keys": _keys(got["fills"]), "scores": _scores(got["fills"]), "truncated": got["truncated"],
                   "world": got["dp_world_size"], "rows": got["row_count"],
                   "ref": {"keys": _keys(ref.fills), "scores": _scores(ref.fills),
                           "truncated": [list(t) for t in ref.truncated]}}
    # one row: the other ranks' slices are empty
    got = map_fill({"text": texts[3], "model_path": MODEL, "targets": [1500, 3, 2000]})
    one = eng.fill_texts(texts[3:4], 5, tids=[1500, 3, 2000])
    out["one"] = {"keys": _keys(got["fills"]), "ref_keys": _keys(one.fills)}
    # the same input error on every rank keeps its type and message
    try:
        map_fill({"text": "q [MASK]", "model_path": MODEL, "targets": ["word"]})
        out["bad"] = None
    except Exception as exc:
        out["bad"] = [type(exc).__name__, str(exc), ERRORS["target_vocab"]]
    res = map_fill_batch([{"texts": texts[:5], "model_path": MODEL, "top_k": 4},
                          {"text": 5, "model_path": MODEL},
                          {"texts": texts[5:], "model_path": MODEL, "top_k": 4}])
    out["batch"] = {"kinds": [r[0] for r in res], "keys": _keys(res[0][1]["fills"] + res[2][1]["fills"]),
                    "truncated": [res[0][1]["truncated"], res[2][1]["truncated"]]}
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
