"""The real ``app.py`` with ``TASKS=map_search`` against the mock controller (CPU engine): ``map_search`` jobs
with an ``index`` in one lease next to a job without one and a bad one."""
from .mock_controller import MockController
from .test_agent_loop import start_agent, stop_agent

MODEL = "bert-tiny?batch=8&seq=32&seed=1"
CORPUS = ["alpha beta", "gamma", "delta eps zeta", "a fourth row", "gamma", "the sixth", "alpha beta gamma"]


def test_agent_posts_ivf_map_search_results(tmp_path):
    import os

    import numpy as np
    import torch

    from agent_tpu_amd.models.bert import config_for, init_random
    from agent_tpu_amd.runtime.classify import ClassifyEngine

    cfg = config_for("bert-tiny")
    eng = ClassifyEngine(cfg, init_random(cfg, seed=1), torch.device("cpu"), batch_rows=8, seq_len=32)
    path = os.path.join(str(tmp_path), "corpus.npy")
    np.save(path, eng.embed_texts(CORPUS).emb.numpy())

    def job(jid, queries, top_k, index=None):
        payload = {"corpus_uri": path, "model_path": MODEL, "queries": queries, "top_k": top_k}
        if index is not None:
            payload["index"] = index
        return {"id": jid, "op": "map_search", "payload": payload}

    # every job has two queries: a one-row matmul of the CPU twin would take another BLAS route
    lease = [job("plain", ["gamma", "alpha beta"], 4),
             job("full", ["gamma", "alpha beta"], 4, {"type": "ivf", "clusters": 3, "nprobe": 3}),
             job("one", ["gamma", "the sixth"], 7, {"type": "ivf", "clusters": 3, "nprobe": 1, "train_iterations": 5}),
             job("bad", ["x", "y"], 2, {"type": "ivf", "clusters": 8})]
    ctl = MockController().start()
    try:
        ctl.lease(*lease, lease_id="L0")
        p = start_agent(ctl, tasks="map_search", MAX_TASKS=len(lease), CLASSIFY_DEVICE="cpu", OMP_NUM_THREADS="2")
        try:
            assert ctl.wait(lambda c: {j["id"] for j in lease} <= {r["job_id"] for r in c.results}, 240), ctl.results
        finally:
            rc, out = stop_agent(p, timeout=60)
        assert rc == 0, out[-3000:]
        res = {r["job_id"]: r for r in ctl.results}
    finally:
        ctl.stop()
    for jid in ("plain", "full", "one"):
        assert res[jid]["status"] == "succeeded" and res[jid]["lease_id"] == "L0" and res[jid]["error"] is None, res[jid]
    plain, full, one = (res[j]["result"] for j in ("plain", "full", "one"))
    assert "index" not in plain and plain["ids"][0][:2] == [1, 4] and plain["ids"][1][0] == 0
    assert full["ids"] == plain["ids"] and full["scores"] == plain["scores"]  # every cluster probed: the exact search
    assert full["index"]["type"] == "ivf" and full["index"]["clusters"] == 3 and full["index"]["nprobe"] == 3
    assert 1 <= full["index"]["train_iterations"] <= 10 and set(full) == set(plain) | {"index"}
    assert one["index"]["nprobe"] == 1 and one["index_cached"] is False and one["corpus_rows"] == 7
    assert one["ids"][0][:2] == [1, 4] and one["scores"][0][0] == one["scores"][0][1]  # both copies of "gamma": one cluster
    assert one["ids"][1][0] == 5 and all(1 <= len(x) <= 7 for x in one["ids"])
    assert res["bad"]["status"] == "failed" and res["bad"]["error"]["type"] == "ValueError"
    assert res["bad"]["error"]["message"].startswith("payload.index must be {'type': 'ivf'}")
