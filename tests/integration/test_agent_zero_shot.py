"""The real ``app.py`` with ``TASKS=map_zero_shot`` against the mock controller (CPU engine): a leased
``map_zero_shot`` job of either payload form posts its result, a lease of jobs is batched and equals the jobs
run one by one, and a bad job fails alone."""
from .mock_controller import MockController
from .test_agent_loop import start_agent, stop_agent

MODEL = "bert-tiny?nli=1&batch=8&seq=40&seed=1"
TEXTS = ["matrix cores multiply tiles", "rain, then sun", "", "gpus multiply matrices, naïve café in Zürich"]
LABELS = ["technology", "weather", "cooking"]


def _run(jobs, lease_id):
    ctl = MockController().start()
    try:
        ctl.lease(*jobs, lease_id=lease_id)
        p = start_agent(ctl, tasks="map_zero_shot", MAX_TASKS=len(jobs), CLASSIFY_DEVICE="cpu", OMP_NUM_THREADS="2")
        try:
            want = {j["id"] for j in jobs}
            assert ctl.wait(lambda c: want <= {r["job_id"] for r in c.results}, 240), ctl.results
        finally:
            rc, out = stop_agent(p, timeout=60)
        assert rc == 0, out[-3000:]
        return {r["job_id"]: r for r in ctl.results}, ctl.lease_requests[0]
    finally:
        ctl.stop()


def _check(result, texts, labels, multi=False):
    assert len(result["results"]) == len(texts) == result["row_count"]
    assert result["label_count"] == len(labels) and result["pair_count"] == len(texts) * len(labels)
    assert result["multi_label"] is multi and (result["entailment_id"], result["contradiction_id"]) == (2, 0)
    for x in result["results"]:
        assert set(x) == {"labels", "scores"} and sorted(x["labels"]) == sorted(labels)
        assert x["scores"] == sorted(x["scores"], reverse=True) and all(0 < s < 1 for s in x["scores"])
        if not multi:
            assert abs(sum(x["scores"]) - 1) < 1e-5


def test_agent_posts_map_zero_shot_results_of_both_forms():
    jobs = [{"id": "z1", "op": "map_zero_shot", "payload": {"texts": TEXTS, "candidate_labels": LABELS, "model_path": MODEL}},
            {"id": "z2", "op": "map_zero_shot", "payload": {"text": TEXTS[1], "candidate_labels": LABELS, "model_path": MODEL,
                                                            "multi_label": True, "top_k": 2,
                                                            "hypothesis_template": "it is about {}"}}]
    res, lease = _run(jobs, "LZ1")
    assert lease["worker_profile"]["workers"]["batch_ops"] == ["map_zero_shot"]
    z1, z2 = res["z1"], res["z2"]
    assert z1["status"] == "succeeded" and z1["lease_id"] == "LZ1" and z1["error"] is None
    r = z1["result"]
    assert r["ok"] and r["op"] == "map_zero_shot" and r["hypothesis_template"] == "This example is {}."
    _check(r, TEXTS, LABELS)
    r = z2["result"]
    assert z2["status"] == "succeeded" and r["row_count"] == 1 and r["label_count"] == 3 and r["multi_label"] is True
    assert r["hypothesis_template"] == "it is about {}" and len(r["results"][0]["labels"]) == 2  # top_k


def test_agent_batches_a_lease_and_a_bad_job_fails_alone():
    jobs = [
        {"id": "a", "op": "map_zero_shot", "payload": {"texts": TEXTS[:2], "candidate_labels": LABELS, "model_path": MODEL}},
        {"id": "bad", "op": "map_zero_shot", "payload": {"text": "no labels", "candidate_labels": [], "model_path": MODEL}},
        {"id": "b", "op": "map_zero_shot", "payload": {"texts": [], "candidate_labels": LABELS, "model_path": MODEL},
         "job_epoch": 4},
        {"id": "c", "op": "map_zero_shot", "payload": {"texts": TEXTS, "candidate_labels": LABELS[::-1] + ["x"],
                                                       "model_path": MODEL}},
    ]
    res, _ = _run(jobs, "LZ2")
    assert res["a"]["status"] == "succeeded" and res["c"]["status"] == "succeeded"
    _check(res["a"]["result"], TEXTS[:2], LABELS)
    _check(res["c"]["result"], TEXTS, LABELS[::-1] + ["x"])
    assert res["b"]["status"] == "succeeded" and res["b"]["job_epoch"] == 4
    assert res["b"]["result"]["results"] == [] and res["b"]["result"]["row_count"] == 0
    assert res["bad"]["status"] == "failed" and res["bad"]["error"]["type"] == "ValueError"
    assert res["bad"]["error"]["message"] == "payload.candidate_labels must be a list of 1 to 256 non-empty strings"
    # batched == job by job: each job alone posts the ranking the lease batch gave it
    for jid in ("a", "c"):
        job = next(j for j in jobs if j["id"] == jid)
        alone, _ = _run([job], "LZ3" + jid)
        for x, y in zip(alone[jid]["result"]["results"], res[jid]["result"]["results"]):
            mine, theirs = dict(zip(x["labels"], x["scores"])), dict(zip(y["labels"], y["scores"]))
            assert mine.keys() == theirs.keys()
            # CPU engines: a pair's fp32 sums depend on the rows it is batched with
            assert all(abs(mine[k] - theirs[k]) <= 1e-6 for k in mine)
