"""The real ``app.py`` with ``TASKS=map_answer`` against the mock controller (CPU engine): a leased
``map_answer`` job with ``doc_stride`` reads a long passage past its first window and posts ``window_count``;
in one lease, jobs with and without the key run apart and a bad ``doc_stride`` fails alone."""
from agent_tpu_amd.utils.synthetic import make_text_rows

from .mock_controller import MockController
from .test_agent_loop import start_agent, stop_agent

MODEL = "bert-tiny?qa=1&batch=8&seq=40&seed=1"
LONG = make_text_rows(2, words_per_row=70, seed=31)
PASSAGES = ["matrix cores multiply tiles", LONG[0], "", LONG[1]]


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
        return {r["job_id"]: r for r in ctl.results}
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


def test_agent_posts_windowed_results_and_a_bad_doc_stride_fails_alone():
    payload = {"question": "how do gpus multiply matrices", "passages": PASSAGES, "model_path": MODEL, "top_k": 8,
               "return_null_scores": True}
    jobs = [{"id": "w", "op": "map_answer", "payload": dict(payload, doc_stride=8)},
            {"id": "plain", "op": "map_answer", "payload": payload},
            {"id": "w2", "op": "map_answer", "payload": dict(payload, doc_stride=8, top_k=2)},
            {"id": "bad", "op": "map_answer", "payload": dict(payload, doc_stride=38)}]
    res = _run(jobs, "LW1")
    w, plain, w2 = (res[k]["result"] for k in ("w", "plain", "w2"))
    assert res["w"]["status"] == res["plain"]["status"] == res["w2"]["status"] == "succeeded"
    assert w["ok"] and w["doc_stride"] == 8 and w["window_count"] > w["pair_count"] == 4
    assert "doc_stride" not in plain and "window_count" not in plain
    _check_answers(w, [PASSAGES], 8)
    _check_answers(plain, [PASSAGES], 8)
    # the windowed reader returns an answer that ends past everything the unwindowed one can reach
    assert max(e["end"] for e in w["answers"][0]) > max(e["end"] for e in plain["answers"][0])
    # jobs w and w2 share a lease batch: the smaller top_k is the prefix, the window count the same
    key = lambda e: (e["passage"], e["start"], e["end"], e["text"])  # noqa: E731
    assert [key(e) for e in w2["answers"][0]] == [key(e) for e in w["answers"][0][:2]]
    assert w2["window_count"] == w["window_count"]
    assert res["bad"]["status"] == "failed" and res["bad"]["error"]["type"] == "ValueError"
    assert res["bad"]["error"]["message"] == "payload.doc_stride must be an integer in [1, seq_len - 3]"
