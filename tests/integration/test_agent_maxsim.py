"""The real ``app.py`` with ``TASKS=map_maxsim`` against the mock controller (CPU engine): one leased job of
each form posts its result, a lease of three pair jobs is batched, and a bad job fails alone."""
from .mock_controller import MockController
from .test_agent_loop import start_agent, stop_agent

MODEL = "bert-tiny?late=64&batch=8&seq=32&seed=1"
PASSAGES = ["matrix cores multiply tiles", "a recipe for bread", "", "gpus multiply matrices with matrix cores"]


def _run(jobs, lease_id):
    ctl = MockController().start()
    try:
        ctl.lease(*jobs, lease_id=lease_id)
        p = start_agent(ctl, tasks="map_maxsim", MAX_TASKS=len(jobs), CLASSIFY_DEVICE="cpu", OMP_NUM_THREADS="2")
        try:
            want = {j["id"] for j in jobs}
            assert ctl.wait(lambda c: want <= {r["job_id"] for r in c.results}, 240), ctl.results
        finally:
            rc, out = stop_agent(p, timeout=60)
        assert rc == 0, out[-3000:]
        return {r["job_id"]: r for r in ctl.results}, ctl.lease_requests[0]
    finally:
        ctl.stop()


def _check_ranked(result, groups, top_k):
    assert len(result["ranked"]) == len(groups)
    for ranked, scores, group in zip(result["ranked"], result["scores"], groups):
        assert len(scores) == len(group) and len(ranked) == min(top_k, len(group))
        order = sorted(range(len(scores)), key=lambda i: (-scores[i], i))[:top_k]
        assert [e["index"] for e in ranked] == order and [e["score"] for e in ranked] == [scores[i] for i in order]


def test_agent_posts_one_result_of_each_form():
    jobs = [{"id": "p1", "op": "map_maxsim", "payload": {"query": "how do gpus multiply matrices", "passages": PASSAGES,
                                                         "model_path": MODEL, "top_k": 3, "return_scores": True}},
            {"id": "s1", "op": "map_maxsim", "payload": {"queries": ["how do gpus multiply matrices", "bread"],
                                                         "shared_passages": PASSAGES, "model_path": MODEL, "top_k": 3,
                                                         "return_scores": True}}]
    res, lease = _run(jobs, "LM1")
    assert lease["worker_profile"]["workers"]["batch_ops"] == ["map_maxsim"]
    p1, s1 = res["p1"], res["s1"]
    assert p1["status"] == "succeeded" and p1["lease_id"] == "LM1" and p1["error"] is None and s1["status"] == "succeeded"
    r = p1["result"]
    assert r["ok"] and r["op"] == "map_maxsim" and r["query_count"] == 1 and r["pair_count"] == 4 and r["top_k"] == 3
    assert r["form"] == "pairs" and r["dim"] == 64
    _check_ranked(r, [PASSAGES], 3)
    s = s1["result"]
    assert s["form"] == "shared" and s["query_count"] == 2 and s["pair_count"] == 8
    _check_ranked(s, [PASSAGES, PASSAGES], 3)
    assert s["scores"][0] == r["scores"][0]  # the same query and passages: the same bits in either form


def test_agent_batches_a_lease_of_three_pair_jobs_and_a_bad_job_fails_alone():
    jobs = [
        {"id": "a", "op": "map_maxsim", "payload": {"queries": ["gpu matrix", "bread"], "passages": [PASSAGES, PASSAGES[:2]],
                                                    "model_path": MODEL, "top_k": 2, "return_scores": True}},
        {"id": "bad", "op": "map_maxsim", "payload": {"query": "x", "passages": ["y"], "model_path": MODEL, "top_k": 99}},
        {"id": "b", "op": "map_maxsim", "payload": {"query": "nothing to rank", "passages": [], "model_path": MODEL},
         "job_epoch": 4},
        {"id": "c", "op": "map_maxsim", "payload": {"query": "gpu matrix", "passages": PASSAGES, "model_path": MODEL,
                                                    "top_k": 4, "return_scores": True, "normalize_by_query_length": True}},
    ]
    res, _ = _run(jobs, "LM2")
    assert res["a"]["status"] == "succeeded" and res["c"]["status"] == "succeeded"
    _check_ranked(res["a"]["result"], [PASSAGES, PASSAGES[:2]], 2)
    assert res["b"]["status"] == "succeeded" and res["b"]["job_epoch"] == 4
    assert res["b"]["result"]["ranked"] == [[]] and res["b"]["result"]["pair_count"] == 0
    c = res["c"]["result"]
    _check_ranked(c, [PASSAGES], 4)
    assert all(-1.00001 <= e["score"] <= 1.00001 for e in c["ranked"][0])  # a mean of cosines
    # same query and passages, one engine call: job c ranks job a's first group the same way
    assert [e["index"] for e in c["ranked"][0]][:2] == [e["index"] for e in res["a"]["result"]["ranked"][0]]
    assert res["bad"]["status"] == "failed" and res["bad"]["error"]["type"] == "ValueError"
    assert res["bad"]["error"]["message"] == "payload.top_k must be an integer in [1, 32]"
