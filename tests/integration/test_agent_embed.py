"""The real ``app.py`` with ``TASKS=map_embed`` against the mock controller (CPU engine): a leased
``map_embed`` job posts its result, lease batching included, and a bad job fails alone."""
import numpy as np

from .mock_controller import MockController
from .test_agent_loop import start_agent, stop_agent

MODEL = "bert-tiny?batch=8&seq=32&seed=1"


def test_agent_posts_map_embed_results():
    jobs = [
        {"id": "e1", "op": "map_embed", "payload": {"texts": ["alpha beta", "gamma", ""], "model_path": MODEL}},
        {"id": "e2", "op": "map_embed", "payload": {"texts": ["delta eps zeta"] * 2, "model_path": MODEL,
                                                    "output": "summary"}, "job_epoch": 5},
        {"id": "bad", "op": "map_embed", "payload": {"texts": ["x"], "model_path": MODEL, "pooling": "max"}},
    ]
    ctl = MockController().start()
    try:
        ctl.lease(*jobs, lease_id="LE")
        p = start_agent(ctl, tasks="map_embed", MAX_TASKS=len(jobs), CLASSIFY_DEVICE="cpu", OMP_NUM_THREADS="2")
        try:
            assert ctl.wait(lambda c: {"e1", "e2", "bad"} <= {r["job_id"] for r in c.results}, 240), ctl.results
        finally:
            rc, out = stop_agent(p, timeout=60)
        assert rc == 0, out[-3000:]
        res = {r["job_id"]: r for r in ctl.results}
        assert ctl.lease_requests[0]["worker_profile"]["workers"]["batch_ops"] == ["map_embed"]
    finally:
        ctl.stop()
    e1 = res["e1"]
    assert e1["status"] == "succeeded" and e1["lease_id"] == "LE" and e1["error"] is None
    r = e1["result"]
    assert r["ok"] and r["op"] == "map_embed" and r["row_count"] == 3 and r["dim"] == 256 and r["pooling"] == "mean"
    emb = np.asarray(r["embeddings"])
    assert emb.shape == (3, 256) and np.allclose(np.linalg.norm(emb, axis=1), 1.0, atol=1e-5)
    assert res["e2"]["status"] == "succeeded" and res["e2"]["job_epoch"] == 5
    assert len(res["e2"]["result"]["centroid"]) == 256 and abs(res["e2"]["result"]["norm_mean"] - 1.0) < 1e-5
    assert res["bad"]["status"] == "failed" and res["bad"]["error"]["type"] == "ValueError"
    assert res["bad"]["error"]["message"] == "payload.pooling must be 'mean' or 'cls'"
