"""The real ``app.py`` with ``TASKS=map_search`` against the mock controller (CPU engine): a lease
with two ``map_search`` jobs and a bad one posts one result per job, through the lease batch handler."""
from .mock_controller import MockController
from .test_agent_loop import start_agent, stop_agent

MODEL = "bert-tiny?batch=8&seq=32&seed=1"
CORPUS = ["alpha beta", "gamma", "delta eps zeta", "a fourth row", "gamma"]


def test_agent_posts_map_search_results(tmp_path):
    import os

    import numpy as np

    from agent_tpu_amd.models.bert import config_for, init_random
    from agent_tpu_amd.runtime.classify import ClassifyEngine
    import torch

    cfg = config_for("bert-tiny")
    eng = ClassifyEngine(cfg, init_random(cfg, seed=1), torch.device("cpu"), batch_rows=8, seq_len=32)
    path = os.path.join(str(tmp_path), "corpus.npy")
    np.save(path, eng.embed_texts(CORPUS).emb.numpy())
    jobs = [
        {"id": "s1", "op": "map_search", "payload": {"queries": ["gamma", "alpha beta"], "corpus_uri": path,
                                                     "model_path": MODEL, "top_k": 2}},
        {"id": "s2", "op": "map_search", "payload": {"queries": ["delta eps zeta"], "corpus_uri": path,
                                                     "model_path": MODEL, "top_k": 32}, "job_epoch": 5},
        {"id": "bad", "op": "map_search", "payload": {"queries": ["x"], "corpus_uri": path, "model_path": MODEL,
                                                      "metric": "l2"}},
    ]
    ctl = MockController().start()
    try:
        ctl.lease(*jobs, lease_id="LS")
        p = start_agent(ctl, tasks="map_search", MAX_TASKS=len(jobs), CLASSIFY_DEVICE="cpu", OMP_NUM_THREADS="2")
        try:
            assert ctl.wait(lambda c: {"s1", "s2", "bad"} <= {r["job_id"] for r in c.results}, 240), ctl.results
        finally:
            rc, out = stop_agent(p, timeout=60)
        assert rc == 0, out[-3000:]
        res = {r["job_id"]: r for r in ctl.results}
        assert ctl.lease_requests[0]["worker_profile"]["workers"]["batch_ops"] == ["map_search"]
    finally:
        ctl.stop()
    s1 = res["s1"]
    assert s1["status"] == "succeeded" and s1["lease_id"] == "LS" and s1["error"] is None
    r = s1["result"]
    assert r["ok"] and r["op"] == "map_search" and r["query_count"] == 2 and r["corpus_rows"] == 5 and r["dim"] == 256
    assert r["ids"] == [[1, 4], [0, r["ids"][1][1]]] and r["scores"][0][0] == r["scores"][0][1]  # the duplicated row ties
    assert abs(r["scores"][1][0] - 1.0) <= 1e-5 and r["top_k"] == 2 and r["metric"] == "cosine"
    r2 = res["s2"]
    assert r2["status"] == "succeeded" and r2["job_epoch"] == 5
    assert r2["result"]["ids"][0][0] == 2 and len(r2["result"]["ids"][0]) == 5 and r2["result"]["top_k"] == 32
    assert res["bad"]["status"] == "failed" and res["bad"]["error"]["type"] == "ValueError"
    assert res["bad"]["error"]["message"] == "payload.metric must be 'cosine' or 'dot'"
