"""Rank body of the map_maxsim DP test (launched by torch.distributed.run, gloo, CPU engines via
CLASSIFY_DEVICE=cpu): rank 0 runs the op, the others serve in ``worker_loop``. Rank 0 prints one
``RESULT {json}`` line with the DP results next to single-process ones (a world-1 engine) on the same texts."""
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, REPO)

import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402

from agent_tpu_amd.parallel import dp, dp_ops  # noqa: E402

MODEL = "bert-tiny?late=64&batch=4&seq=32&seed=6"


def scenario():
    rank, ws = dp.world()
    if rank != 0:
        dp_ops.worker_loop()
        return None
    from agent_tpu_amd.models.bert import config_for, init_random
    from agent_tpu_amd.runtime.classify import ClassifyEngine
    from ops.map_maxsim import map_maxsim, map_maxsim_batch

    cfg = config_for("bert-tiny", late_dim=64)
    eng = ClassifyEngine(cfg, init_random(cfg, seed=6), torch.device("cpu"), batch_rows=4, seq_len=32)  # world 1
    out = {"world": ws}
    queries = ["alpha beta gamma", "lorem ipsum", "unused", "dolor sit amet consectetur"]
    groups = [[f"passage {i} " + "lorem ipsum dolor " * (i % 3) for i in range(5)], ["ipsum", "amet sit"], [],
              [f"text {i}" for i in range(4)]]  # 11 pairs: every split falls inside a group
    flat = [p for g in groups for p in g]
    goff = [0, 5, 7, 7, 11]
    pool = flat[:7]

    def ref(q, p, g, k):
        r = eng.maxsim_rank(q, p, g, top_k=k)
        return {"idx": r.idx.tolist(), "score": r.score.tolist(), "scores": r.scores.tolist()}

    def pick(got):
        return {"ranked": got["ranked"], "scores": got["scores"], "world": got["dp_world_size"],
                "pairs": got["pair_count"], "form": got["form"]}

    got = map_maxsim({"queries": queries, "passages": groups, "model_path": MODEL, "top_k": 3, "return_scores": True})
    out["many"] = dict(pick(got), ref=ref(queries, flat, goff, 3))
    got = map_maxsim({"queries": queries[:3], "shared_passages": pool, "model_path": MODEL, "top_k": 3,
                      "return_scores": True})
    out["shared"] = dict(pick(got), ref=ref(queries[:3], pool, None, 3))
    # one passage: every rank but the first has none
    got = map_maxsim({"query": queries[0], "passages": flat[:1], "model_path": MODEL, "return_scores": True})
    out["one"] = dict(pick(got), ref=ref(queries[:1], flat[:1], [0, 1], 10))
    got = map_maxsim({"queries": queries[:2], "shared_passages": pool[:1], "model_path": MODEL, "return_scores": True})
    out["shared_one"] = dict(pick(got), ref=ref(queries[:2], pool[:1], None, 10))
    try:
        map_maxsim({"query": "q", "passages": ["p"], "model_path": MODEL, "top_k": 40})
        out["bad"] = None
    except Exception as exc:
        out["bad"] = [type(exc).__name__, str(exc)]
    res = map_maxsim_batch([{"queries": queries[:2], "passages": groups[:2], "model_path": MODEL, "top_k": 3,
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
