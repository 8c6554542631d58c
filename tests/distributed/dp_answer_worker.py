"""Rank body of the map_answer DP test (launched by torch.distributed.run, gloo, CPU engines via
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

MODEL = "bert-tiny?qa=1&batch=4&seq=40&seed=6"


def fault():
    """``MI355X_FAULT=rank:1:answer:1``: rank 1 raises in its first answer job only."""
    from ops.map_answer import map_answer

    out = {}
    try:
        map_answer({"question": "q", "passages": ["p one", "r two", "s three"], "model_path": MODEL})
        out["err"] = None
    except Exception as exc:
        out["err"] = [type(exc).__name__, str(exc)]
    got = map_answer({"question": "q", "passages": ["p one", "r two", "s three"], "model_path": MODEL})  # still serves
    out["after"] = [got["pair_count"], got["dp_world_size"], len(got["answers"][0])]
    dp_ops.shutdown_workers()
    return out


def _keys(answers):
    return [[[e["passage"], e["start"], e["end"], e["text"]] for e in row] for row in answers]


def scenario():
    rank, ws = dp.world()
    if rank != 0:
        dp_ops.worker_loop()
        return None
    if sys.argv[1:] == ["fault"]:
        return fault()
    from agent_tpu_amd.models.bert import config_for, init_random
    from agent_tpu_amd.runtime.classify import ClassifyEngine
    from ops.map_answer import ERRORS, map_answer, map_answer_batch

    cfg = config_for("bert-tiny", qa_head=True)
    eng = ClassifyEngine(cfg, init_random(cfg, seed=6), torch.device("cpu"), batch_rows=4, seq_len=40)
    out = {"world": ws}
    questions = ["alpha beta gamma", "lorem ipsum", "unused", "dolor sit amet consectetur"]
    groups = [[f"passage {i} " + "lorem ipsum dolor " * (i % 3) for i in range(5)], ["ipsum", "amet sit"], [],
              [f"text {i} naïve café" for i in range(4)]]  # 11 pairs: every split falls inside a group
    flat = [p for g in groups for p in g]
    goff = [0, 5, 7, 7, 11]

    def ref(k):
        r = eng.answer_pairs(questions, flat, goff, top_k=k)
        return {"keys": _keys(r.answers), "scores": [[e["score"] for e in row] for row in r.answers],
                "null": r.null.tolist()}

    got = map_answer({"questions": questions, "passages": groups, "model_path": MODEL, "top_k": 3,
                      "return_null_scores": True})
    out["many"] = {"keys": _keys(got["answers"]), "scores": [[e["score"] for e in row] for row in got["answers"]],
                   "probs": [[e["probability"] for e in row] for row in got["answers"]],
                   "null": got["null_scores"], "world": got["dp_world_size"], "pairs": got["pair_count"], "ref": ref(3)}
    # one pair: the other ranks' slices are empty
    got = map_answer({"question": questions[0], "passages": flat[:1], "model_path": MODEL, "return_null_scores": True})
    one = eng.answer_pairs(questions[:1], flat[:1], [0, 1])
    out["one"] = {"keys": _keys(got["answers"]), "null": got["null_scores"], "ref_keys": _keys(one.answers),
                  "ref_null": one.null.tolist()}
    # the same input error on every rank keeps its type and message
    try:
        map_answer({"question": "q", "passages": ["p"], "model_path": MODEL, "max_answer_tokens": 99})
        out["bad"] = None
    except Exception as exc:
        out["bad"] = [type(exc).__name__, str(exc), ERRORS["max_answer_tokens"]]
    res = map_answer_batch([{"questions": questions[:2], "passages": groups[:2], "model_path": MODEL, "top_k": 3},
                            {"question": 5, "passages": [], "model_path": MODEL},
                            {"questions": questions[2:], "passages": groups[2:], "model_path": MODEL, "top_k": 2}])
    out["batch"] = {"kinds": [r[0] for r in res], "keys": _keys(res[0][1]["answers"] + res[2][1]["answers"])}
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
