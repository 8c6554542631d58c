"""The real ``app.py`` with ``TASKS=map_search`` against the mock controller (CPU engine): filtered
``map_search`` jobs in one lease, with equal and with different filters, post what each job gives
on its own (a lease of one)."""
from .mock_controller import MockController
from .test_agent_loop import start_agent, stop_agent

MODEL = "bert-tiny?batch=8&seq=32&seed=1"
CORPUS = ["alpha beta", "gamma", "delta eps zeta", "a fourth row", "gamma", "the sixth", "alpha beta gamma"]
LABELS = [0, 1, 0, 2, 1, 2, 0]


def _run(jobs):
    """Every job list of ``jobs`` as a lease of its own, one agent -> {job id: posted result}."""
    ctl = MockController().start()
    try:
        for n, lease in enumerate(jobs):
            ctl.lease(*lease, lease_id=f"L{n}")
        total = sum(len(lease) for lease in jobs)
        want = {j["id"] for lease in jobs for j in lease}
        p = start_agent(ctl, tasks="map_search", MAX_TASKS=total, CLASSIFY_DEVICE="cpu", OMP_NUM_THREADS="2")
        try:
            assert ctl.wait(lambda c: want <= {r["job_id"] for r in c.results}, 240), ctl.results
        finally:
            rc, out = stop_agent(p, timeout=60)
        assert rc == 0, out[-3000:]
        return {r["job_id"]: r for r in ctl.results}
    finally:
        ctl.stop()


def test_agent_posts_filtered_map_search_results(tmp_path):
    import os

    import numpy as np
    import torch

    from agent_tpu_amd.models.bert import config_for, init_random
    from agent_tpu_amd.runtime.classify import ClassifyEngine

    cfg = config_for("bert-tiny")
    eng = ClassifyEngine(cfg, init_random(cfg, seed=1), torch.device("cpu"), batch_rows=8, seq_len=32)
    path, lpath = os.path.join(str(tmp_path), "corpus.npy"), os.path.join(str(tmp_path), "labels.npy")
    np.save(path, eng.embed_texts(CORPUS).emb.numpy())
    np.save(lpath, np.asarray(LABELS, dtype=np.int32))
    base = {"corpus_uri": path, "model_path": MODEL, "corpus_labels_uri": lpath}

    def job(jid, queries, top_k, flt=None):
        payload = dict(base, queries=queries, top_k=top_k)
        if flt is not None:
            payload["filter"] = flt
        return {"id": jid, "op": "map_search", "payload": payload}

    lease = [job("a", ["gamma", "alpha beta"], 2, {"ids": [0, 4, 6]}),
             # equal to a's filter: one group. Two queries, as a has: alone, a one-row matmul of the CPU
             # twin would take another BLAS route than the group's and round differently
             job("b", ["delta eps zeta", "the sixth"], 5, {"ids": [6, 4, 0, 0]}),
             job("c", ["gamma"], 3, {"exclude_ids": [1]}),
             job("d", ["gamma", "the sixth"], 4, {"labels": [1, 2]}),
             job("e", ["alpha beta"], 4, {"label_range": [5, 9]}),  # allows nothing
             job("f", ["gamma"], 2),
             job("bad", ["x"], 2, {"ids": [7]})]
    res = _run([lease])
    for jid in "abcdef":
        assert res[jid]["status"] == "succeeded" and res[jid]["lease_id"] == "L0" and res[jid]["error"] is None, res[jid]
    a, b, c, d, e, f = (res[j]["result"] for j in "abcdef")
    assert a["filter_rows"] == 3 and [x[0] for x in a["ids"]] == [4, 0] and a["corpus_rows"] == 7
    assert all(len(x) == 2 and set(x) <= {0, 4, 6} for x in a["ids"])
    assert abs(a["scores"][0][0] - 1.0) <= 1e-5 and abs(a["scores"][1][0] - 1.0) <= 1e-5
    assert b["filter_rows"] == 3 and sorted(b["ids"][0]) == [0, 4, 6] and b["top_k"] == 5
    assert c["filter_rows"] == 6 and c["ids"][0][0] == 4 and 1 not in c["ids"][0]  # the other copy of "gamma"
    assert d["filter_rows"] == 4 and d["ids"][0][:2] == [1, 4] and d["scores"][0][0] == d["scores"][0][1]
    assert sorted(d["ids"][0]) == [1, 3, 4, 5] and d["ids"][1][0] == 5
    assert e["filter_rows"] == 0 and e["ids"] == [[]] and e["scores"] == [[]]
    assert "filter_rows" not in f and f["ids"] == [[1, 4]]
    assert res["bad"]["status"] == "failed" and res["bad"]["error"]["type"] == "ValueError"
    assert res["bad"]["error"]["message"] == ("payload.filter.ids must be a list of at most 1048576 integers "
                                              "in [0, corpus rows)")
    # batched equals job by job: the same jobs, each a lease of its own
    alone = _run([[j] for j in lease if j["id"] != "bad"])
    for jid in "abcdef":
        one, got = alone[jid]["result"], res[jid]["result"]
        assert set(one) == set(got), jid
        for key in one:
            if key not in ("elapsed_ms", "queries_per_sec", "index_cached"):
                assert got[key] == one[key], (jid, key)
