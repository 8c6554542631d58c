"""The real ``app.py`` with ``TASKS=map_dedup`` against the mock controller (CPU engine): a lease with a
``vectors`` job, a ``vectors_uri`` job with ``output: "npy"`` and a bad one posts one result per job; the bad
one fails alone."""
import os

import numpy as np

from .mock_controller import MockController
from .test_agent_loop import start_agent, stop_agent

KEYS = {"ok", "op", "row_count", "dim", "metric", "threshold", "pair_count", "group_count", "duplicate_count",
        "kept_count", "largest_group", "elapsed_ms", "rows_per_sec", "dp_world_size"}


def test_agent_posts_map_dedup_results(tmp_path):
    rng = np.random.default_rng(0)
    x = rng.integers(-2, 3, (60, 64)).astype(np.float32)
    group = list(range(60))
    for a in (0, 10, 20):  # three groups of three identical rows
        x[a + 1] = x[a + 5] = x[a]
        group[a + 1] = group[a + 5] = a
    path = os.path.join(str(tmp_path), "vec.npy")
    np.save(path, x)
    out = os.path.join(str(tmp_path), "res.npy")
    jobs = [
        {"id": "d1", "op": "map_dedup", "payload": {"vectors": x.tolist(), "threshold": 0.999, "max_pairs": 4}},
        {"id": "d2", "op": "map_dedup", "payload": {"vectors_uri": path, "threshold": 0.999, "output": "npy",
                                                    "output_uri": out}, "job_epoch": 7},
        {"id": "bad", "op": "map_dedup", "payload": {"vectors_uri": path, "threshold": 0.999, "metric": "l2"}},
    ]
    ctl = MockController().start()
    try:
        ctl.lease(*jobs, lease_id="LD")
        p = start_agent(ctl, tasks="map_dedup", MAX_TASKS=len(jobs), CLASSIFY_DEVICE="cpu", OMP_NUM_THREADS="2")
        try:
            assert ctl.wait(lambda c: {"d1", "d2", "bad"} <= {r["job_id"] for r in c.results}, 240), ctl.results
        finally:
            rc, log = stop_agent(p, timeout=60)
        assert rc == 0, log[-3000:]
        res = {r["job_id"]: r for r in ctl.results}
    finally:
        ctl.stop()
    d1 = res["d1"]
    assert d1["status"] == "succeeded" and d1["lease_id"] == "LD" and d1["error"] is None
    r = d1["result"]
    assert KEYS <= set(r) and r["op"] == "map_dedup" and r["row_count"] == 60 and r["dim"] == 64 and r["metric"] == "cosine"
    assert r["group"] == group and r["keep"] == [i for i in range(60) if group[i] == i]
    assert r["pair_count"] == 9 and r["group_count"] == 3 and r["duplicate_count"] == 6 and r["kept_count"] == 54
    assert r["largest_group"] == 3 and len(r["pairs"]) == 4 and all(p["i"] < p["j"] for p in r["pairs"])
    assert r["threshold"] == float(np.float32(0.999))
    d2 = res["d2"]
    assert d2["status"] == "succeeded" and d2["job_epoch"] == 7
    r2 = d2["result"]
    assert KEYS <= set(r2) and "group" not in r2 and r2["index_cached"] is False
    assert np.load(r2["group_uri"]).tolist() == group
    assert res["bad"]["status"] == "failed" and res["bad"]["error"]["type"] == "ValueError"
    assert res["bad"]["error"]["message"] == "payload.metric must be 'cosine' or 'dot'"
