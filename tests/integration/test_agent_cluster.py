"""The real ``app.py`` with ``TASKS=map_cluster`` against the mock controller (CPU engine): a lease with a
``vectors`` job, a ``vectors_uri`` job with ``output: "npy"`` and a bad one posts one result per job; the bad
one fails alone."""
import os

import numpy as np

from .mock_controller import MockController
from .test_agent_loop import start_agent, stop_agent

KEYS = {"ok", "op", "row_count", "dim", "k", "metric", "iterations", "converged", "changed_last", "objective", "sizes",
        "empty_clusters", "elapsed_ms", "rows_per_sec", "dp_world_size"}


def test_agent_posts_map_cluster_results(tmp_path):
    rng = np.random.default_rng(0)
    x = np.zeros((60, 64), dtype=np.float32)
    planted = np.arange(60) % 3
    for k in range(3):
        x[planted == k, 20 * k:20 * k + 20] = 30.0
    x += rng.integers(-1, 2, x.shape).astype(np.float32)
    path = os.path.join(str(tmp_path), "vec.npy")
    np.save(path, x)
    out = os.path.join(str(tmp_path), "res.npy")
    init = x[:3].tolist()  # rows 0, 1, 2: one of every group
    jobs = [
        {"id": "c1", "op": "map_cluster", "payload": {"vectors": x.tolist(), "k": 3, "metric": "l2", "init_centroids": init,
                                                      "representatives": 2}},
        {"id": "c2", "op": "map_cluster", "payload": {"vectors_uri": path, "k": 3, "init_centroids": init, "output": "npy",
                                                      "output_uri": out}, "job_epoch": 7},
        {"id": "bad", "op": "map_cluster", "payload": {"vectors_uri": path, "k": 3, "metric": "dot"}},
    ]
    ctl = MockController().start()
    try:
        ctl.lease(*jobs, lease_id="LC")
        p = start_agent(ctl, tasks="map_cluster", MAX_TASKS=len(jobs), CLASSIFY_DEVICE="cpu", OMP_NUM_THREADS="2")
        try:
            assert ctl.wait(lambda c: {"c1", "c2", "bad"} <= {r["job_id"] for r in c.results}, 240), ctl.results
        finally:
            rc, log = stop_agent(p, timeout=60)
        assert rc == 0, log[-3000:]
        res = {r["job_id"]: r for r in ctl.results}
    finally:
        ctl.stop()
    c1 = res["c1"]
    assert c1["status"] == "succeeded" and c1["lease_id"] == "LC" and c1["error"] is None
    r = c1["result"]
    assert KEYS <= set(r) and r["op"] == "map_cluster" and r["row_count"] == 60 and r["dim"] == 64 and r["k"] == 3
    assert r["labels"] == planted.tolist() and r["sizes"] == [20, 20, 20] and r["converged"] and r["metric"] == "l2"
    assert len(r["centroids"]) == 3 and len(r["centroids"][0]) == 64 and r["empty_clusters"] == 0
    assert all(len(rep["ids"]) == 2 and all(planted[i] == k for i in rep["ids"]) for k, rep in enumerate(r["representatives"]))
    c2 = res["c2"]
    assert c2["status"] == "succeeded" and c2["job_epoch"] == 7
    r2 = c2["result"]
    assert KEYS <= set(r2) and "labels" not in r2 and r2["index_cached"] is False and r2["metric"] == "cosine"
    assert np.load(r2["labels_uri"]).tolist() == planted.tolist() and np.load(r2["centroids_uri"]).shape == (3, 64)
    assert res["bad"]["status"] == "failed" and res["bad"]["error"]["type"] == "ValueError"
    assert res["bad"]["error"]["message"] == "payload.metric must be 'cosine' or 'l2'"
