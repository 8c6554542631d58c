"""The real ``app.py`` with ``TASKS=map_tag`` against the mock controller (CPU engine): a leased ``map_tag``
job of either payload form posts its result, a lease of jobs is batched, and a bad job fails alone."""
from .mock_controller import MockController
from .test_agent_loop import start_agent, stop_agent

MODEL = "bert-tiny?tags=5&batch=8&seq=40&seed=1"
TEXTS = ["matrix cores multiply tiles", "a recipe for bread", "", "gpus multiply matrices, naïve café in Zürich"]


def _run(jobs, lease_id):
    ctl = MockController().start()
    try:
        ctl.lease(*jobs, lease_id=lease_id)
        p = start_agent(ctl, tasks="map_tag", MAX_TASKS=len(jobs), CLASSIFY_DEVICE="cpu", OMP_NUM_THREADS="2")
        try:
            want = {j["id"] for j in jobs}
            assert ctl.wait(lambda c: want <= {r["job_id"] for r in c.results}, 240), ctl.results
        finally:
            rc, out = stop_agent(p, timeout=60)
        assert rc == 0, out[-3000:]
        return {r["job_id"]: r for r in ctl.results}, ctl.lease_requests[0]
    finally:
        ctl.stop()


def _check_entities(result, texts, max_entities, keys):
    assert len(result["entities"]) == len(texts) == len(result["entity_counts"]) == result["row_count"]
    assert result["truncated"] == [i for i, c in enumerate(result["entity_counts"]) if c > max_entities]
    for text, row, count in zip(texts, result["entities"], result["entity_counts"]):
        assert len(row) == min(count, max_entities) and (count > 0 or not text)
        for e in row:
            assert set(e) == keys and text[e["start"]:e["end"]] == e["word"] and e["word"] and 0 < e["score"] <= 1


GROUPED = {"entity_group", "score", "word", "start", "end"}
TOKENS = {"entity", "score", "index", "word", "start", "end"}


def test_agent_posts_map_tag_results_of_both_forms():
    jobs = [{"id": "t1", "op": "map_tag", "payload": {"texts": TEXTS, "model_path": MODEL, "max_entities": 3}},
            {"id": "t2", "op": "map_tag", "payload": {"text": TEXTS[3], "model_path": MODEL, "aggregation": "none"}}]
    res, lease = _run(jobs, "LT1")
    assert lease["worker_profile"]["workers"]["batch_ops"] == ["map_tag"]
    t1, t2 = res["t1"], res["t2"]
    assert t1["status"] == "succeeded" and t1["lease_id"] == "LT1" and t1["error"] is None
    r = t1["result"]
    assert r["ok"] and r["op"] == "map_tag" and r["row_count"] == 4 and r["aggregation"] == "simple"
    _check_entities(r, TEXTS, 3, GROUPED)
    assert t2["status"] == "succeeded" and t2["result"]["row_count"] == 1 and t2["result"]["max_entities"] == 64
    _check_entities(t2["result"], TEXTS[3:], 64, TOKENS)


def test_agent_batches_a_lease_and_a_bad_job_fails_alone():
    jobs = [
        {"id": "a", "op": "map_tag", "payload": {"texts": TEXTS[:2], "model_path": MODEL}},
        {"id": "bad", "op": "map_tag", "payload": {"text": "x", "model_path": MODEL, "max_entities": 999}},
        {"id": "b", "op": "map_tag", "payload": {"texts": [], "model_path": MODEL}, "job_epoch": 4},
        {"id": "c", "op": "map_tag", "payload": {"texts": TEXTS, "model_path": MODEL}},
    ]
    res, _ = _run(jobs, "LT2")
    assert res["a"]["status"] == "succeeded" and res["c"]["status"] == "succeeded"
    _check_entities(res["a"]["result"], TEXTS[:2], 64, GROUPED)
    _check_entities(res["c"]["result"], TEXTS, 64, GROUPED)
    assert res["b"]["status"] == "succeeded" and res["b"]["job_epoch"] == 4
    assert res["b"]["result"]["entities"] == [] and res["b"]["result"]["row_count"] == 0
    # the same texts in one engine call: job a's rows are job c's first rows
    key = lambda e: (e["entity_group"], e["start"], e["end"], e["word"])  # noqa: E731
    for ra, rc in zip(res["a"]["result"]["entities"], res["c"]["result"]["entities"]):
        assert [key(e) for e in ra] == [key(e) for e in rc]
    assert res["bad"]["status"] == "failed" and res["bad"]["error"]["type"] == "ValueError"
    assert res["bad"]["error"]["message"] == "payload.max_entities must be an integer in [1, 512]"
