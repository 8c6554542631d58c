"""Rank body of the map_zero_shot DP test (launched by torch.distributed.run, gloo, CPU engines via
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

MODEL = "bert-tiny?nli=1&batch=4&seq=32&seed=6"
LABELS = ["technology", "weather", "cooking", "sports", "x"]


def fault():
    """``MI355X_FAULT=rank:1:zero_shot:1``: rank 1 raises in its first zero-shot job only."""
    from ops.map_zero_shot import map_zero_shot

    out = {}
    texts = ["p one", "r two two", "three"]
    try:
        map_zero_shot({"texts": texts, "candidate_labels": LABELS, "model_path": MODEL})
        out["err"] = None
    except Exception as exc:
        out["err"] = [type(exc).__name__, str(exc)]
    got = map_zero_shot({"texts": texts, "candidate_labels": LABELS, "model_path": MODEL})  # still serves
    out["after"] = [got["row_count"], got["dp_world_size"], len(got["results"]), got["pair_count"]]
    dp_ops.shutdown_workers()
    return out


def _ref(eng, texts, labels, multi, template="This example is {}."):
    """The single-process engine on the same job: ``[labels, scores]`` per text."""
    hyps = [template.replace("{}", name) for name in labels]
    res = eng.zero_shot(texts, hyps, [(0, len(hyps))] * len(texts), multi, ent=2, con=0)
    out = []
    for t in range(len(texts)):
        order, score = res.ranked(t)
        out.append([[labels[i] for i in order], score])
    return out


def _flat(results):
    return [[x["labels"], x["scores"]] for x in results]


def scenario():
    rank, ws = dp.world()
    if rank != 0:
        dp_ops.worker_loop()
        return None
    if sys.argv[1:] == ["fault"]:
        return fault()
    from agent_tpu_amd.models.bert import config_for, init_random
    from agent_tpu_amd.runtime.classify import ClassifyEngine
    from ops.map_zero_shot import ERRORS, map_zero_shot, map_zero_shot_batch

    cfg = config_for("bert-tiny", num_labels=3)
    eng = ClassifyEngine(cfg, init_random(cfg, seed=6), torch.device("cpu"), batch_rows=4, seq_len=32)
    out = {"world": ws}
    texts = [f"text {i} naïve café " + "lorem ipsum dolor " * (i % 4) for i in range(7)]  # 35 pairs: an uneven split

    got = map_zero_shot({"texts": texts, "candidate_labels": LABELS, "model_path": MODEL})
    out["many"] = {"got": _flat(got["results"]), "ref": _ref(eng, texts, LABELS, False), "world": got["dp_world_size"],
                   "rows": got["row_count"], "pairs": got["pair_count"]}
    # one text, two labels: some ranks' slices are empty, and the labels may sit on different ranks
    got = map_zero_shot({"text": texts[3], "candidate_labels": LABELS[:2], "model_path": MODEL, "multi_label": True})
    out["one"] = {"got": _flat(got["results"]), "ref": _ref(eng, texts[3:4], LABELS[:2], True)}
    # the same input error on every rank keeps its type and message
    try:
        map_zero_shot({"text": "q", "candidate_labels": LABELS, "model_path": MODEL, "entailment_id": 9})
        out["bad"] = None
    except Exception as exc:
        out["bad"] = [type(exc).__name__, str(exc), ERRORS["label_ids"]]
    res = map_zero_shot_batch([{"texts": texts[:4], "candidate_labels": LABELS, "model_path": MODEL},
                               {"text": 5, "candidate_labels": LABELS, "model_path": MODEL},
                               {"texts": texts[4:], "candidate_labels": LABELS[1:4], "model_path": MODEL,
                                "hypothesis_template": "it is about {}"}])
    out["batch"] = {"kinds": [r[0] for r in res], "got": [_flat(res[0][1]["results"]), _flat(res[2][1]["results"])],
                    "ref": [_ref(eng, texts[:4], LABELS, False),
                            _ref(eng, texts[4:], LABELS[1:4], False, "it is about {}")]}
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
