"""The real ``app.py`` with ``TASKS=map_answer`` against the mock controller (CPU engine): a leased
``map_answer`` job posts its result, a lease of mixed ``top_k`` jobs is batched, and a bad job fails alone."""
from .mock_controller import MockController
from .test_agent_loop import start_agent, stop_agent

MODEL = "bert-tiny?qa=1&batch=8&seq=40&seed=1"
PASSAGES = ["matrix cores multiply tiles", "a recipe for bread", "", "gpus multiply matrices with matrix cores"]


def _run(jobs, lease_id):
    ctl = MockController().start()
    try:
        ctl.lease(*jobs, lease_id=lease_id)
        p = start_agent(ctl, tasks="map_answer", MAX_TASKS=len(jobs), CLASSIFY_DEVICE="cpu", OMP_NUM_THREADS="2")
        try:
            want = {j["id"] for j in jobs}
            assert ctl.wait(lambda c: want <= {r["job_id"] for r in c.results}, 240), ctl.results
        finally:
            rc, out = stop_agent(p, timeout=60)
        assert rc == 0, out[-3000:]
        return {r["job_id"]: r for r in ctl.results}, ctl.lease_requests[0]
    finally:
        ctl.stop()


def _check_answers(result, groups, top_k):
    assert len(result["answers"]) == len(groups)
    for row, nulls, group in zip(result["answers"], result["null_scores"], groups):
        assert len(nulls) == len(group) and len(row) <= top_k and (len(row) > 0) == any(group)
        assert [e["score"] for e in row] == sorted((e["score"] for e in row), reverse=True)
        assert not row or abs(sum(e["probability"] for e in row) - 1.0) < 1e-9
        for e in row:
            assert group[e["passage"]][e["start"]:e["end"]] == e["text"] and e["text"]
            assert e["null_score"] == nulls[e["passage"]]


def test_agent_posts_one_map_answer_result():
    job = {"id": "a1", "op": "map_answer", "payload": {"question": "how do gpus multiply matrices", "passages": PASSAGES,
                                                       "model_path": MODEL, "top_k": 3, "return_null_scores": True}}
    res, lease = _run([job], "LA1")
    assert lease["worker_profile"]["workers"]["batch_ops"] == ["map_answer"]
    a1 = res["a1"]
    assert a1["status"] == "succeeded" and a1["lease_id"] == "LA1" and a1["error"] is None
    r = a1["result"]
    assert r["ok"] and r["op"] == "map_answer" and r["query_count"] == 1 and r["pair_count"] == 4 and r["top_k"] == 3
    assert len(r["answers"][0]) == 3
    _check_answers(r, [PASSAGES], 3)


def test_agent_batches_a_lease_of_mixed_top_k_and_a_bad_job_fails_alone():
    jobs = [
        {"id": "a", "op": "map_answer", "payload": {"questions": ["gpu matrix", "bread"],
                                                    "passages": [PASSAGES, PASSAGES[:2]], "model_path": MODEL,
                                                    "top_k": 2, "return_null_scores": True}},
        {"id": "bad", "op": "map_answer", "payload": {"question": "x", "passages": ["y"], "model_path": MODEL,
                                                      "top_k": 99}},
        {"id": "b", "op": "map_answer", "payload": {"question": "nothing to read", "passages": [], "model_path": MODEL},
         "job_epoch": 4},
        {"id": "c", "op": "map_answer", "payload": {"question": "gpu matrix", "passages": PASSAGES, "model_path": MODEL,
                                                    "top_k": 5, "return_null_scores": True}},
    ]
    res, _ = _run(jobs, "LA2")
    assert res["a"]["status"] == "succeeded" and res["c"]["status"] == "succeeded"
    _check_answers(res["a"]["result"], [PASSAGES, PASSAGES[:2]], 2)
    _check_answers(res["c"]["result"], [PASSAGES], 5)
    assert res["b"]["status"] == "succeeded" and res["b"]["job_epoch"] == 4
    assert res["b"]["result"]["answers"] == [[]] and res["b"]["result"]["pair_count"] == 0
    # same question and passages, one engine call at the largest top_k: job a's answers are the prefix of job c's
    key = lambda e: (e["passage"], e["start"], e["end"], e["text"])  # noqa: E731
    a0, c0 = res["a"]["result"]["answers"][0], res["c"]["result"]["answers"][0]
    assert len(a0) == 2 and len(c0) == 5 and [key(e) for e in a0] == [key(e) for e in c0[:2]]
    assert res["bad"]["status"] == "failed" and res["bad"]["error"]["type"] == "ValueError"
    assert res["bad"]["error"]["message"] == "payload.top_k must be an integer in [1, 32]"
