"""The real ``app.py`` with ``TASKS=map_rerank`` against the mock controller (CPU engine): a leased
``map_rerank`` job posts its result, lease batching included, and a bad job fails alone."""
from .mock_controller import MockController
from .test_agent_loop import start_agent, stop_agent

MODEL = "bert-tiny?labels=1&batch=8&seq=32&seed=1"
PASSAGES = ["matrix cores multiply tiles", "a recipe for bread", "", "gpus multiply matrices with matrix cores"]


def _run(jobs, lease_id):
    ctl = MockController().start()
    try:
        ctl.lease(*jobs, lease_id=lease_id)
        p = start_agent(ctl, tasks="map_rerank", MAX_TASKS=len(jobs), CLASSIFY_DEVICE="cpu", OMP_NUM_THREADS="2")
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


def test_agent_posts_one_map_rerank_result():
    job = {"id": "r1", "op": "map_rerank", "payload": {"query": "how do gpus multiply matrices", "passages": PASSAGES,
                                                       "model_path": MODEL, "top_k": 3, "return_scores": True}}
    res, lease = _run([job], "LR1")
    assert lease["worker_profile"]["workers"]["batch_ops"] == ["map_rerank"]
    r1 = res["r1"]
    assert r1["status"] == "succeeded" and r1["lease_id"] == "LR1" and r1["error"] is None
    r = r1["result"]
    assert r["ok"] and r["op"] == "map_rerank" and r["query_count"] == 1 and r["pair_count"] == 4 and r["top_k"] == 3
    _check_ranked(r, [PASSAGES], 3)


def test_agent_batches_a_lease_and_a_bad_job_fails_alone():
    jobs = [
        {"id": "a", "op": "map_rerank", "payload": {"queries": ["gpu matrix", "bread"], "passages": [PASSAGES, PASSAGES[:2]],
                                                    "model_path": MODEL, "top_k": 2, "return_scores": True}},
        {"id": "bad", "op": "map_rerank", "payload": {"query": "x", "passages": ["y"], "model_path": MODEL, "top_k": 99}},
        {"id": "b", "op": "map_rerank", "payload": {"query": "nothing to rank", "passages": [], "model_path": MODEL},
         "job_epoch": 4},
        {"id": "c", "op": "map_rerank", "payload": {"query": "gpu matrix", "passages": PASSAGES, "model_path": MODEL,
                                                    "top_k": 4, "return_scores": True, "activation": "sigmoid"}},
    ]
    res, _ = _run(jobs, "LR2")
    assert res["a"]["status"] == "succeeded" and res["c"]["status"] == "succeeded"
    _check_ranked(res["a"]["result"], [PASSAGES, PASSAGES[:2]], 2)
    assert res["b"]["status"] == "succeeded" and res["b"]["job_epoch"] == 4
    assert res["b"]["result"]["ranked"] == [[]] and res["b"]["result"]["pair_count"] == 0
    c = res["c"]["result"]
    assert c["activation"] == "sigmoid" and all(0.0 < e["score"] < 1.0 for e in c["ranked"][0])
    # same query and passages, one engine call: job c ranks job a's first group the same way
    assert [e["index"] for e in c["ranked"][0]][:2] == [e["index"] for e in res["a"]["result"]["ranked"][0]]
    assert res["bad"]["status"] == "failed" and res["bad"]["error"]["type"] == "ValueError"
    assert res["bad"]["error"]["message"] == "payload.top_k must be an integer in [1, 32]"
