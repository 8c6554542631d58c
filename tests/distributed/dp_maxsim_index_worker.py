"""Rank body of the map_maxsim index DP test (launched by torch.distributed.run, gloo, CPU engines via
CLASSIFY_DEVICE=cpu): rank 0 runs the op, the others serve in ``worker_loop``. Rank 0 prints one
``RESULT {json}`` line with the DP results next to single-process ones (a world-1 engine and the runtime's
own writer and loader) on the same texts."""
import json
import os
import shutil
import sys
import tempfile

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, REPO)

import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402

from agent_tpu_amd.parallel import dp, dp_ops  # noqa: E402

MODEL = "bert-tiny?late=64&batch=4&seq=32&seed=6"


def _bytes(path):
    with open(path, "rb") as f:
        return f.read()


def scenario(tmp):
    rank, ws = dp.world()
    if rank != 0:
        dp_ops.worker_loop()
        return None
    from agent_tpu_amd.models.bert import config_for, init_random
    from agent_tpu_amd.runtime import maxsim_index as mi
    from agent_tpu_amd.runtime.classify import ClassifyEngine
    from ops.map_maxsim import map_maxsim, map_maxsim_batch

    cfg = config_for("bert-tiny", late_dim=64)
    eng = ClassifyEngine(cfg, init_random(cfg, seed=6), torch.device("cpu"), batch_rows=4, seq_len=32)  # world 1
    out = {"world": ws}
    queries = ["alpha beta gamma", "lorem ipsum", "dolor sit amet consectetur"]
    pool = [f"passage {i} " + "lorem ipsum dolor " * (i % 3) for i in range(5)] + ["ipsum", "amet sit"]  # 7 passages

    def build(passages, dtype, name):
        uri, ref = os.path.join(tmp, f"{name}.npy"), os.path.join(tmp, f"{name}_ref.npy")
        got = map_maxsim({"passages": passages, "index_out": {"uri": uri, "dtype": dtype}, "model_path": MODEL})
        tok, lens = eng.maxsim_build(passages)
        mi.write_index(ref, tok, lens, dtype)
        same = _bytes(uri) == _bytes(ref) and _bytes(mi.offsets_path(uri)) == _bytes(mi.offsets_path(ref))
        return uri, ref, {"same_files": same, "world": got["dp_world_size"], "passages": got["passage_count"],
                          "tokens": got["token_count"], "form": got["form"]}

    def ref_rank(q, ref, cand, k):
        index = mi.load_index(ref)
        r = eng.maxsim_index_rank(q, index, cand, top_k=k)
        idx = r.idx.tolist() if cand is None else [[cand[qi][i] if i >= 0 else -1 for i in row]
                                                   for qi, row in enumerate(r.idx.tolist())]
        return {"idx": idx, "score": r.score.tolist(), "scores": r.scores.tolist()}

    def pick(got):
        return {"ranked": got["ranked"], "scores": got.get("scores"), "world": got["dp_world_size"],
                "pairs": got["pair_count"], "form": got["form"], "passages": got["passage_count"],
                "dtype": got["index_dtype"]}

    uri16, ref16, out["build16"] = build(pool, "float16", "p16")
    uri32, ref32, out["build32"] = build(pool, "float32", "p32")
    for name, uri, ref in (("f16", uri16, ref16), ("f32", uri32, ref32)):
        got = map_maxsim({"queries": queries, "index_uri": uri, "model_path": MODEL, "top_k": 3})
        out["whole_" + name] = dict(pick(got), ref=ref_rank(queries, ref, None, 3))
        cand = [[6, 0, 3, 2], [], [1, 5, 4]]
        got = map_maxsim({"queries": queries, "index_uri": uri, "candidates": cand, "model_path": MODEL, "top_k": 3,
                          "return_scores": True})
        out["cand_" + name] = dict(pick(got), ref=ref_rank(queries, ref, cand, 3))
    # the fp32 index equals the shared form on the same strings
    r = eng.maxsim_rank(queries, pool, None, top_k=3)
    out["shared_ref"] = {"idx": r.idx.tolist(), "score": r.score.tolist()}
    # fewer passages than ranks: every rank but the first holds an empty slice
    uri1, ref1, out["build1"] = build(pool[:1], "float16", "one")
    got = map_maxsim({"queries": queries[:2], "index_uri": uri1, "model_path": MODEL})
    out["whole_one"] = dict(pick(got), ref=ref_rank(queries[:2], ref1, None, 10))
    got = map_maxsim({"queries": queries[:2], "index_uri": uri1, "candidates": [[0], [0]], "model_path": MODEL,
                      "return_scores": True})
    out["cand_one"] = dict(pick(got), ref=ref_rank(queries[:2], ref1, [[0], [0]], 10))
    try:
        map_maxsim({"queries": queries, "index_uri": uri16, "candidates": [[7], [], []], "model_path": MODEL})
        out["bad"] = None
    except Exception as exc:
        out["bad"] = [type(exc).__name__, str(exc)]
    res = map_maxsim_batch([{"queries": queries[:2], "index_uri": uri16, "model_path": MODEL, "top_k": 3},
                            {"query": 5, "index_uri": uri16, "model_path": MODEL},
                            {"queries": queries[2:], "index_uri": uri16, "model_path": MODEL, "top_k": 2}])
    out["batch"] = {"kinds": [r[0] for r in res], "ranked": res[0][1]["ranked"] + res[2][1]["ranked"]}
    dp_ops.shutdown_workers()
    return out


def main():
    dist.init_process_group("gloo")
    tmp = tempfile.mkdtemp(prefix="dp_maxsim_index_") if int(os.environ.get("RANK", "0")) == 0 else None
    try:
        res = scenario(tmp)
    finally:
        if dist.is_initialized():
            dist.destroy_process_group()
        if tmp is not None:
            shutil.rmtree(tmp, ignore_errors=True)
    if int(os.environ.get("RANK", "0")) == 0:
        print("RESULT " + json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
