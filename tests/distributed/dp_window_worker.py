"""Rank body of the map_answer ``doc_stride`` DP test (launched by torch.distributed.run, gloo, CPU engines
via CLASSIFY_DEVICE=cpu): rank 0 runs the op, the others serve in ``worker_loop``. Rank 0 prints one
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
STRIDE = 8


def _keys(answers):
    return [[[e["passage"], e["start"], e["end"], e["text"]] for e in row] for row in answers]


def scenario():
    rank, ws = dp.world()
    if rank != 0:
        dp_ops.worker_loop()
        return None
    from agent_tpu_amd.models.bert import config_for, init_random
    from agent_tpu_amd.runtime.classify import ClassifyEngine
    from agent_tpu_amd.utils.synthetic import make_text_rows
    from ops.map_answer import WINDOW_ERRORS, map_answer, map_answer_batch

    cfg = config_for("bert-tiny", qa_head=True)
    eng = ClassifyEngine(cfg, init_random(cfg, seed=6), torch.device("cpu"), batch_rows=4, seq_len=40)
    out = {"world": ws}
    questions = ["alpha beta gamma", "lorem ipsum", "unused", "dolor sit amet consectetur"]
    long = make_text_rows(4, words_per_row=70, seed=21)  # several windows each
    groups = [[long[0], "passage one", long[1], "", "lorem ipsum dolor"], ["ipsum", long[2]], [],
              [f"text {i} naïve café" for i in range(3)] + [long[3]]]  # 11 pairs: every split falls inside a group
    flat = [p for g in groups for p in g]
    goff = [0, 5, 7, 7, 11]

    ref = eng.answer_pairs(questions, flat, goff, top_k=3, doc_stride=STRIDE)
    got = map_answer({"questions": questions, "passages": groups, "model_path": MODEL, "top_k": 3,
                      "return_null_scores": True, "doc_stride": STRIDE})
    out["many"] = {"keys": _keys(got["answers"]), "scores": [[e["score"] for e in row] for row in got["answers"]],
                   "null": got["null_scores"], "world": got["dp_world_size"], "pairs": got["pair_count"],
                   "windows": got["window_count"], "doc_stride": got["doc_stride"],
                   "ends": [[e["end"] for e in row] for row in got["answers"]],
                   "ref": {"keys": _keys(ref.answers), "scores": [[e["score"] for e in row] for row in ref.answers],
                           "null": ref.null.tolist(), "windows": ref.window_count,
                           "per_pair": eng.window_counts.tolist()}}
    plain = eng.answer_pairs(questions, flat, goff, top_k=3)
    out["plain_ends"] = [[e["end"] for e in row] for row in plain.answers]
    # one pair: the other ranks' slices are empty
    got = map_answer({"question": questions[0], "passages": flat[:1], "model_path": MODEL, "doc_stride": STRIDE})
    one = eng.answer_pairs(questions[:1], flat[:1], [0, 1], doc_stride=STRIDE)
    out["one"] = {"keys": _keys(got["answers"]), "windows": got["window_count"], "ref_keys": _keys(one.answers),
                  "ref_windows": one.window_count}
    # the same input error on every rank keeps its type and message
    try:
        map_answer({"question": "q", "passages": ["p"], "model_path": MODEL, "doc_stride": 38})
        out["bad"] = None
    except Exception as exc:
        out["bad"] = [type(exc).__name__, str(exc), WINDOW_ERRORS["doc_stride"]]
    res = map_answer_batch([{"questions": questions[:2], "passages": groups[:2], "model_path": MODEL, "top_k": 3,
                             "doc_stride": STRIDE},
                            {"question": "q", "passages": ["p"], "model_path": MODEL, "doc_stride": 0},
                            {"questions": questions[2:], "passages": groups[2:], "model_path": MODEL, "top_k": 2,
                             "doc_stride": STRIDE}])
    out["batch"] = {"kinds": [r[0] for r in res], "keys": _keys(res[0][1]["answers"] + res[2][1]["answers"]),
                    "windows": [res[0][1]["window_count"], res[2][1]["window_count"]]}
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
