"""The real ``app.py`` with ``TASKS=map_search`` against the mock controller (CPU engine): a ``map_search`` job
with ``compression`` in one lease next to a job without it and a bad one."""
from .mock_controller import MockController
from .test_agent_loop import start_agent, stop_agent


def test_agent_posts_compressed_map_search_results(tmp_path):
    import os

    import numpy as np
    import torch

    gen = torch.Generator().manual_seed(3)
    proto = torch.randn(16, 16, 4, generator=gen)
    pick = torch.randint(0, 16, (300, 16), generator=gen)
    c = (proto[torch.arange(16)[None, :], pick] + 0.02 * torch.randn(300, 16, 4, generator=gen)).reshape(300, 64)
    c[250] = c[7]  # a duplicated row: equal codes, equal scores, ascending id
    path = os.path.join(str(tmp_path), "corpus.npy")
    np.save(path, c.numpy())
    queries = c[[7, 100]].tolist()

    def job(jid, top_k, compression=None):
        payload = {"corpus_uri": path, "query_vectors": queries, "top_k": top_k}
        if compression is not None:
            payload["compression"] = compression
        return {"id": jid, "op": "map_search", "payload": payload}

    lease = [job("plain", 3), job("pq", 3, {"type": "pq", "subvectors": 16, "train_iterations": 3}),
             job("bad", 3, {"type": "pq", "subvectors": 6})]
    ctl = MockController().start()
    try:
        ctl.lease(*lease, lease_id="L0")
        p = start_agent(ctl, tasks="map_search", MAX_TASKS=len(lease), CLASSIFY_DEVICE="cpu", OMP_NUM_THREADS="2")
        try:
            assert ctl.wait(lambda c: {j["id"] for j in lease} <= {r["job_id"] for r in c.results}, 240), ctl.results
        finally:
            rc, out = stop_agent(p, timeout=60)
        assert rc == 0, out[-3000:]
        res = {r["job_id"]: r for r in ctl.results}
    finally:
        ctl.stop()
    for jid in ("plain", "pq"):
        assert res[jid]["status"] == "succeeded" and res[jid]["lease_id"] == "L0" and res[jid]["error"] is None, res[jid]
    plain, pq = res["plain"]["result"], res["pq"]["result"]
    assert "compression" not in plain and set(pq) == set(plain) | {"compression"}
    assert pq["compression"] == {"type": "pq", "subvectors": 16, "train_rows": 300, "train_iterations": 3,
                                 "bytes_per_row": 16}
    assert plain["ids"][0][:2] == [7, 250] and plain["ids"][1][0] == 100
    assert pq["ids"][0][:2] == [7, 250] and pq["scores"][0][0] == pq["scores"][0][1] and pq["ids"][1][0] == 100
    assert pq["index_cached"] is False and pq["corpus_rows"] == 300 and all(len(x) == 3 for x in pq["ids"])
    assert res["bad"]["status"] == "failed" and res["bad"]["error"]["type"] == "ValueError"
    assert res["bad"]["error"]["message"].startswith("payload.compression must be {'type': 'pq'")
