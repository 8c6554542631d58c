"""The real ``app.py`` with ``TASKS=map_fill`` against the mock controller (CPU engine): a leased ``map_fill``
job of either payload form posts its result, a lease of jobs is batched and equals the jobs run one by one,
and a bad job fails alone."""
from .mock_controller import MockController
from .test_agent_loop import start_agent, stop_agent

MODEL = "bert-tiny?mlm=1&batch=8&seq=40&seed=1"
TEXTS = ["matrix cores [MASK] tiles", "a [MASK] for [MASK]", "[MASK]", "gpus multiply [MASK], naïve café in Zürich"]


def _run(jobs, lease_id):
    ctl = MockController().start()
    try:
        ctl.lease(*jobs, lease_id=lease_id)
        p = start_agent(ctl, tasks="map_fill", MAX_TASKS=len(jobs), CLASSIFY_DEVICE="cpu", OMP_NUM_THREADS="2")
        try:
            want = {j["id"] for j in jobs}
            assert ctl.wait(lambda c: want <= {r["job_id"] for r in c.results}, 240), ctl.results
        finally:
            rc, out = stop_agent(p, timeout=60)
        assert rc == 0, out[-3000:]
        return {r["job_id"]: r for r in ctl.results}, ctl.lease_requests[0]
    finally:
        ctl.stop()


def _check_fills(result, texts, k):
    assert len(result["fills"]) == len(texts) == result["row_count"] and result["truncated"] == []
    for text, row in zip(texts, result["fills"]):
        assert len(row) == text.count("[MASK]")
        for m in row:
            assert set(m) == {"start", "end", "candidates"} and text[m["start"]:m["end"]] == "[MASK]"
            assert len(m["candidates"]) == k
            sc = [c["score"] for c in m["candidates"]]
            assert sc == sorted(sc, reverse=True) and all(0 < s <= 1 for s in sc)
            for c in m["candidates"]:
                assert set(c) == {"token_id", "token", "score"} and c["token"] is None and 0 <= c["token_id"] < 4096


def _key(fills):
    return [[[m["start"], m["end"], [c["token_id"] for c in m["candidates"]]] for m in row] for row in fills]


def _scores(fills):
    return [c["score"] for row in fills for m in row for c in m["candidates"]]


def test_agent_posts_map_fill_results_of_both_forms():
    jobs = [{"id": "f1", "op": "map_fill", "payload": {"texts": TEXTS, "model_path": MODEL, "top_k": 3}},
            {"id": "f2", "op": "map_fill", "payload": {"text": TEXTS[1], "model_path": MODEL, "targets": [7, 1200, 7]}}]
    res, lease = _run(jobs, "LF1")
    assert lease["worker_profile"]["workers"]["batch_ops"] == ["map_fill"]
    f1, f2 = res["f1"], res["f2"]
    assert f1["status"] == "succeeded" and f1["lease_id"] == "LF1" and f1["error"] is None
    r = f1["result"]
    assert r["ok"] and r["op"] == "map_fill" and r["row_count"] == 4 and r["top_k"] == 3 and r["mask_token"] == "[MASK]"
    _check_fills(r, TEXTS, 3)
    assert f2["status"] == "succeeded" and f2["result"]["row_count"] == 1 and f2["result"]["top_k"] == 5
    _check_fills(f2["result"], TEXTS[1:2], 2)  # top_k capped by the two distinct targets
    for m in f2["result"]["fills"][0]:
        assert sorted(c["token_id"] for c in m["candidates"]) == [7, 1200]


def test_agent_batches_a_lease_and_a_bad_job_fails_alone():
    jobs = [
        {"id": "a", "op": "map_fill", "payload": {"texts": TEXTS[:2], "model_path": MODEL}},
        {"id": "bad", "op": "map_fill", "payload": {"text": "no mask here", "model_path": MODEL}},
        {"id": "b", "op": "map_fill", "payload": {"texts": [], "model_path": MODEL}, "job_epoch": 4},
        {"id": "c", "op": "map_fill", "payload": {"texts": TEXTS, "model_path": MODEL}},
    ]
    res, _ = _run(jobs, "LF2")
    assert res["a"]["status"] == "succeeded" and res["c"]["status"] == "succeeded"
    _check_fills(res["a"]["result"], TEXTS[:2], 5)
    _check_fills(res["c"]["result"], TEXTS, 5)
    assert res["b"]["status"] == "succeeded" and res["b"]["job_epoch"] == 4
    assert res["b"]["result"]["fills"] == [] and res["b"]["result"]["row_count"] == 0
    # the same texts in one engine call: job a's rows are job c's first rows
    assert _key(res["a"]["result"]["fills"]) == _key(res["c"]["result"]["fills"][:2])
    assert res["bad"]["status"] == "failed" and res["bad"]["error"]["type"] == "ValueError"
    assert res["bad"]["error"]["message"] == "payload text 0 has no mask token"
    # batched == job by job: each job alone posts the candidates the lease batch gave it
    for jid in ("a", "c"):
        job = next(j for j in jobs if j["id"] == jid)
        alone, _ = _run([job], "LF3" + jid)
        assert _key(alone[jid]["result"]["fills"]) == _key(res[jid]["result"]["fills"])
        for x, y in zip(_scores(alone[jid]["result"]["fills"]), _scores(res[jid]["result"]["fills"])):
            assert abs(x - y) <= 1e-6  # CPU engines: a row's fp32 sums depend on the rows it is batched with
