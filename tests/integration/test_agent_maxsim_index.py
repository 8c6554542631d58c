"""The real ``app.py`` with ``TASKS=map_maxsim`` against the mock controller (CPU engine): a build job writes an
index, a query job in the next lease ranks against it as the shared form does, and a bad payload fails alone."""
import numpy as np

from .mock_controller import MockController
from .test_agent_loop import start_agent, stop_agent

MODEL = "bert-tiny?late=64&batch=8&seq=32&seed=1"
PASSAGES = ["matrix cores multiply tiles", "a recipe for bread", "", "gpus multiply matrices with matrix cores"]
QUERIES = ["how do gpus multiply matrices", "bread"]


def test_agent_builds_an_index_then_queries_it(tmp_path):
    uri = str(tmp_path / "pool.npy")
    op = "map_maxsim"
    first = [{"id": "build", "op": op, "payload": {"passages": PASSAGES, "index_out": {"uri": uri, "dtype": "float32"},
                                                   "model_path": MODEL}}]
    second = [{"id": "whole", "op": op, "payload": {"queries": QUERIES, "index_uri": uri, "model_path": MODEL, "top_k": 3}},
              {"id": "bad", "op": op, "payload": {"queries": QUERIES, "index_uri": uri, "model_path": MODEL,
                                                  "candidates": [[0, 0], [1]]}},
              {"id": "cand", "op": op, "payload": {"queries": QUERIES, "index_uri": uri, "model_path": MODEL, "top_k": 3,
                                                   "candidates": [[3, 1, 0, 2], [1]], "return_scores": True}},
              {"id": "shared", "op": op, "payload": {"queries": QUERIES, "shared_passages": PASSAGES, "model_path": MODEL,
                                                     "top_k": 3, "return_scores": True}}]
    ctl = MockController().start()
    try:
        ctl.lease(*first, lease_id="LX1")
        ctl.lease(*second, lease_id="LX2")
        p = start_agent(ctl, tasks=op, MAX_TASKS=5, CLASSIFY_DEVICE="cpu", OMP_NUM_THREADS="2")
        try:
            want = {j["id"] for j in first + second}
            assert ctl.wait(lambda c: want <= {r["job_id"] for r in c.results}, 240), ctl.results
        finally:
            rc, out = stop_agent(p, timeout=60)
        assert rc == 0, out[-3000:]
        res = {r["job_id"]: r for r in ctl.results}
    finally:
        ctl.stop()
    b = res["build"]
    assert b["status"] == "succeeded" and b["lease_id"] == "LX1" and b["error"] is None
    r = b["result"]
    assert r["ok"] and r["form"] == "build" and r["passage_count"] == 4 and r["dim"] == 64 and r["dtype"] == "float32"
    off = np.load(r["offsets_uri"])
    assert np.load(uri).shape == (r["token_count"], 64) and off[0] == 0 and off[-1] == r["token_count"] and len(off) == 5
    shared, whole, cand = res["shared"]["result"], res["whole"]["result"], res["cand"]["result"]
    assert res["whole"]["status"] == "succeeded" and res["whole"]["lease_id"] == "LX2"
    assert whole["form"] == "index" and whole["passage_count"] == 4 and whole["pair_count"] == 8 and "scores" not in whole
    assert whole["ranked"] == shared["ranked"]  # a float32 index: the same bits as the on-the-fly path
    assert cand["scores"] == [[shared["scores"][0][i] for i in (3, 1, 0, 2)], [shared["scores"][1][1]]]
    assert cand["ranked"][1] == [{"index": 1, "score": shared["scores"][1][1]}]
    assert sorted(e["index"] for e in cand["ranked"][0]) == sorted(e["index"] for e in shared["ranked"][0])
    assert res["bad"]["status"] == "failed" and res["bad"]["error"]["type"] == "ValueError"
    assert res["bad"]["error"]["message"] == "payload.candidates must not repeat an id within a query"
