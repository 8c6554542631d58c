"""sim_topk_wide's CPU path and argument checks, and map_search ``depth`` on the CPU engine (the HIP kernel is
tested in tests/kernels/test_search_wide_gpu.py)."""
import os

import numpy as np
import pytest
import torch

import ops as registry
from agent_tpu_amd import ops
from agent_tpu_amd.runtime import search as rs


def _ints(rows, nq=4, D=64, seed=3):
    gen = torch.Generator().manual_seed(seed)
    c = torch.randint(-2, 3, (40, D), generator=gen).float()[torch.randint(0, 40, (rows,), generator=gen)]  # ties
    return torch.randint(-2, 3, (nq, D), generator=gen).float(), c.contiguous()


def test_sim_topk_wide_ok_names_the_supported_shapes():
    assert ops.sim_topk_wide_ok(64, 1) and ops.sim_topk_wide_ok(768, 33) and ops.sim_topk_wide_ok(1024, 1024)
    for D, k in [(768, 0), (768, 1025), (32, 100), (96, 100), (1088, 100)]:
        assert not ops.sim_topk_wide_ok(D, k), (D, k)
    assert ops.search.WIDE_MAX_K == 1024 and ops.sim_topk_ok(768, 33) is False  # sim_topk keeps its own range


def test_cpu_path_is_the_twin_and_arguments_are_checked():
    q, c = _ints(300)
    for k in (33, 100, 1024):
        s, i = ops.sim_topk_wide(q, c, k, id_base=7)
        ws, wi = ops.sim_topk_ref(q, c, k, 7)
        assert s.shape == (4, min(k, 300)) and torch.equal(s, ws) and torch.equal(i, wi)
    s, i = ops.sim_topk_wide(q.half().float(), c.half(), 100, row_scale=torch.full((300,), 0.5))
    assert torch.equal(s, ops.sim_topk_ref(q, c, 100)[0] * 0.5)
    s, i = ops.sim_topk_wide(q[:0], c, 100)
    assert s.shape == i.shape == (0, 100) and i.dtype == torch.int64
    bad = [(q, c, 1025), (q, c, 0), (q, c, True), (q.double(), c, 100), (q, c[:0], 100), (q, c, 100, 0, 0),
           (q, c, 100, 0, 257), (q, c, 100, 0, None, torch.ones(300)), (q, c.half(), 100, 0, None, torch.ones(299)),
           (q[:, :32].contiguous(), c[:, :32].contiguous(), 100), (q, torch.zeros(300, 128)[:, ::2], 100)]
    for args in bad:  # (q, c, k, id_base, splits, row_scale)
        with pytest.raises(ValueError):
            ops.sim_topk_wide(*args)


@pytest.fixture
def search(monkeypatch):
    monkeypatch.setenv("CLASSIFY_DEVICE", "cpu")
    monkeypatch.delenv("TASKS", raising=False)
    monkeypatch.delenv("SEARCH_INDEX_DTYPE", raising=False)
    rs.clear_cache()
    yield registry.get_op("map_search")
    rs.clear_cache()


DEPTH_CASES = [("depth", {"depth": 100, "top_k": 5}), ("depth", {"depth": 32}), ("depth", {"depth": 1025}),
               ("depth", {"depth": True}), ("depth", {"depth": "100"}),
               ("depth_combined", {"depth": 100, "filter": {"ids": [1]}}),
               ("depth_combined", {"depth": 100, "index": {"type": "ivf"}}),
               ("depth_combined", {"depth": 100, "index": {"type": "ivfpq", "subvectors": 16}}),
               ("depth_combined", {"depth": 100, "compression": {"type": "pq", "subvectors": 16}}),
               ("depth_combined", {"depth": 100, "compression": {"type": "binary"}}),
               ("depth_combined", {"depth": 100, "refine": {"candidates": 128}}),
               ("depth_combined", {"depth": 100, "diversify": {}})]


@pytest.mark.parametrize("key,extra", DEPTH_CASES)
def test_depth_errors_are_fixed_and_listed_in_the_contract(search, tmp_path, key, extra):
    from ops import map_search as ms

    contract = open(os.path.join(os.path.dirname(ms.__file__), "map_search.CONTRACT.md")).read()
    msg = ms.DEPTH_ERRORS[key]
    assert msg in contract
    path = str(tmp_path / "c.npy")
    np.save(path, np.ones((300, 64), dtype=np.float32))
    with pytest.raises(ValueError) as e:
        search(dict({"query_vectors": [[1.0] * 64], "corpus_uri": path}, **extra))
    assert str(e.value) == msg


@pytest.mark.parametrize("rows", [300, 60])
def test_depth_job_returns_what_stable_sorts_give(search, tmp_path, rows):
    q, c = _ints(rows)
    path = str(tmp_path / "ints.npy")
    np.save(path, c.numpy())
    res = search({"query_vectors": q.tolist(), "corpus_uri": path, "metric": "dot", "depth": 100, "min_score": -1e9})
    sc = q.double().numpy() @ c.double().numpy().T
    order = np.argsort(-sc, axis=1, kind="stable")[:, :100]  # score descending, id ascending
    assert res["ids"] == order.tolist() and res["scores"] == np.take_along_axis(sc, order, 1).tolist()
    assert res["depth"] == 100 and res["corpus_rows"] == rows and len(res["ids"][0]) == min(100, rows)
    plain = search({"query_vectors": q.tolist(), "corpus_uri": path, "metric": "dot", "top_k": 32})
    assert "depth" not in plain and set(res) - set(plain) == {"depth"}
    assert plain["ids"] == [row[:32] for row in res["ids"]]  # a prefix of the deep list
