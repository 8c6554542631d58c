"""map_search with ``refine`` on a CPU engine: exact re-scoring of the product-quantized search's shortlist.

The corpus is test_search_pq_cpu.py's product-structured one (sixteen blobs per sub-space), generated the same way;
NOISY has more noise inside a blob than the codebooks resolve, so the plain PQ search misses exact neighbours.
Exact-score tolerance (test_search_f16_cpu.py's): ``(D + 2) * 2^-24 * scale * sum_k |q_k c_k|`` in fp64.
"""
import os

import numpy as np
import pytest
import torch

import ops as registry
from agent_tpu_amd import ops
from agent_tpu_amd.runtime import pq
from agent_tpu_amd.runtime import refine as rfn
from agent_tpu_amd.runtime import search as rs
from ops import map_search as ms

MODEL = "bert-tiny?batch=8&seq=32&seed=4"
U = 2.0 ** -24
N, D = 600, 64
NOISY = 0.35


def _blobs(noise, N=N, D=D, M=16, seed=2):
    gen = torch.Generator().manual_seed(seed)
    dsub = D // M
    proto = torch.randn(M, 16, dsub, generator=gen)
    proto = proto / proto.norm(dim=2, keepdim=True)  # sixteen unit blobs per sub-space
    pick = torch.randint(0, 16, (N, M), generator=gen)
    x = proto[torch.arange(M)[None, :], pick] + noise * torch.randn(N, M, dsub, generator=gen)
    return x.reshape(N, D).contiguous()


@pytest.fixture
def search(monkeypatch):
    monkeypatch.setenv("CLASSIFY_DEVICE", "cpu")
    for name in ("TASKS", "SEARCH_INDEX_DTYPE", "SEARCH_INDEX_MAX_GB", "SEARCH_REFINE_MAX_GB"):
        monkeypatch.delenv(name, raising=False)
    monkeypatch.setenv("SEARCH_INDEX_LRU_SIZE", "8")
    rs.clear_cache()
    yield registry.get_op("map_search")
    rs.clear_cache()


@pytest.fixture(scope="module")
def data(tmp_path_factory):
    c = _blobs(NOISY)
    gen = torch.Generator().manual_seed(5)
    q = (c[::12] + 0.2 * torch.randn(50, D, generator=gen)).contiguous()  # 50 queries near corpus rows
    path = str(tmp_path_factory.mktemp("refine") / "blobs.npy")
    np.save(path, c.numpy())
    return q, c, path


PQ = {"type": "pq", "subvectors": 16, "train_iterations": 4}


@pytest.mark.parametrize("metric", ["cosine", "dot"])
@pytest.mark.parametrize("vectors", ["float16", "float32"])
def test_scores_are_exact_and_the_result_has_the_refine_key(search, data, metric, vectors):
    q, c, path = data
    job = {"query_vectors": q[:9].tolist(), "corpus_uri": path, "top_k": 6, "metric": metric, "compression": PQ}
    plain = search(dict(job))
    res = search(dict(job, refine={"candidates": 64, "vectors": vectors}))
    assert list(res) == list(plain)[:-2] + ["refine", "ids", "scores"] and res["compression"] == plain["compression"]
    assert res["refine"] == {"candidates": 64, "vectors": vectors, "store": "host", "rescored_rows": 64}
    stored = c.half().double() if vectors == "float16" else c.double()
    qd = (rs.normalize_rows(q[:9]) if metric == "cosine" else q[:9]).double()
    scale = 1.0 / stored.norm(dim=1) if metric == "cosine" else torch.ones(N, dtype=torch.float64)
    exact = (qd @ stored.T) * scale
    tol = (D + 2) * U * scale * (qd.abs() @ stored.abs().T)
    for a, (ids, scores) in enumerate(zip(res["ids"], res["scores"])):
        assert len(set(ids)) == 6
        assert ((torch.tensor(scores, dtype=torch.float64) - exact[a, ids]).abs() <= tol[a, ids]).all(), a
    again = search(dict(job, refine={"candidates": 64, "vectors": vectors, "store": "host"}))
    assert again["index_cached"] is True and again["ids"] == res["ids"] and again["scores"] == res["scores"]
    assert search(dict(job, refine={"candidates": 64, "vectors": vectors, "store": "device"}))["index_cached"] is False
    # a job without the key: today's keys and today's values (the twin of the plain compressed search)
    after = search(dict(job))
    assert after["ids"] == plain["ids"] and after["scores"] == plain["scores"] and list(after) == list(plain)
    assert "refine" not in plain and "store" not in str(sorted(plain))
    idx = pq.load_index(path, 0, -1, torch.device("cpu"), 16, N, 4, metric == "cosine")
    assert idx.cached and idx.store is None
    ws, wi = ops.sim_topk_pq_ref((rs.normalize_rows(q[:9]) if metric == "cosine" else q[:9]).contiguous(), idx.codebooks,
                                 idx.codes, 6)
    assert plain["ids"] == wi.tolist() and plain["scores"] == ws.tolist()


@pytest.mark.parametrize("corpus_dtype", ["float32", "float16"])
def test_the_largest_shortlist_gives_the_uncompressed_search(search, data, corpus_dtype):
    """``candidates = 32 * ceil(rows / 64)``: one segment per 64-row code block, the longest shortlist the rows
    allow (half of them). It holds every query's exact top 10 here, so ids and scores are the uncompressed search's
    over the same ``corpus_dtype``, exactly: the same stored values, the same scale, the same order."""
    q, c, path = data
    job = {"query_vectors": q.tolist(), "corpus_uri": path, "top_k": 10}
    want = search(dict(job, corpus_dtype=corpus_dtype))
    res = search(dict(job, compression=PQ, refine={"candidates": 32 * -(-N // 64), "vectors": corpus_dtype}))
    assert res["refine"]["rescored_rows"] == 32 * (N // 64) + min(32, N % 64)
    assert res["ids"] == want["ids"] and res["scores"] == want["scores"]


def test_recall_is_no_lower_with_refine(search, data):
    q, c, path = data
    job = {"query_vectors": q.tolist(), "corpus_uri": path, "top_k": 10}
    exact = search(dict(job))["ids"]
    recall = lambda r: sum(len(set(a) & set(b)) for a, b in zip(r["ids"], exact)) / (10.0 * len(exact))  # noqa: E731
    plain, refined = recall(search(dict(job, compression=PQ))), recall(search(dict(job, compression=PQ, refine={"candidates": 64})))
    print(f"recall@10: plain PQ {plain:.3f}, refined (64 candidates, float16) {refined:.3f}")
    # measured on this corpus (CPU engine): plain PQ 0.828, refined 0.998
    assert plain < 0.9 and refined >= plain and refined > 0.9


CASES = [
    ("refine", {"refine": None}), ("refine", {"refine": 64}), ("refine", {"refine": {}}),
    ("refine", {"refine": {"candidates": 64, "rows": 1}}), ("refine", {"refine": {"candidates": 0}}),
    ("refine", {"refine": {"candidates": 48}}), ("refine", {"refine": {"candidates": 8224}}),
    ("refine", {"refine": {"candidates": 64.0}}), ("refine", {"refine": {"candidates": True}}),
    ("refine", {"refine": {"candidates": 64, "vectors": 16}, "compression": None}),  # malformed comes first
    ("refine", {"refine": {"candidates": 64, "vectors": "bfloat16"}}), ("refine", {"refine": {"candidates": 64, "store": "disk"}}),
    ("refine_compression", {"refine": {"candidates": 64}, "compression": None}),
    ("refine_filter", {"refine": {"candidates": 64}, "filter": {"ids": [1]}}),
    ("refine_index", {"refine": {"candidates": 64}, "index": {"type": "ivf"}, "compression": None}),
    ("refine_index", {"refine": {"candidates": 64}, "index": {"type": "ivfpq", "subvectors": 16}, "compression": None}),
]


@pytest.mark.parametrize("key,extra", CASES)
def test_refine_errors(search, data, key, extra):
    q, c, path = data
    job = dict({"query_vectors": q[:2].tolist(), "corpus_uri": path, "compression": PQ}, **extra)
    if job["compression"] is None:
        del job["compression"]
    with pytest.raises(ValueError) as e:
        search(job)
    assert str(e.value) == ms.REFINE_ERRORS[key]


def test_the_store_limit_and_the_contract(search, data, monkeypatch):
    q, c, path = data
    contract = open(os.path.join(os.path.dirname(ms.__file__), "map_search.CONTRACT.md")).read()
    for msg in ms.REFINE_ERRORS.values():
        assert msg in contract, msg
    assert set(ms.REFINE_ERRORS) == {k for k, _ in CASES} | {"refine_too_large"}
    assert ms.REFINE_ERRORS["refine_too_large"] == rfn.ERRORS["refine_too_large"]
    monkeypatch.setenv("SEARCH_INDEX_MAX_GB", str((N * 16 + N * D * 2) / 2 ** 30))  # the codes fit, not the fp16 rows beside them
    job = {"query_vectors": q[:2].tolist(), "corpus_uri": path, "compression": PQ}
    assert search(dict(job))["ok"]
    with pytest.raises(ValueError) as e:
        search(dict(job, refine={"candidates": 64}))
    assert str(e.value) == ms.REFINE_ERRORS["refine_too_large"] and len(rs.cache_info()["entries"]) == 1


def test_batch_handler_groups_by_the_canonical_refine(search, tmp_path):
    from agent_tpu_amd.models.bert import config_for

    texts = ["the quick brown fox", "jumps over, the lazy dog!", "MI355X " * 30, "x", "seven rows in all",
             "an index of sentence vectors", "nearest neighbours by cosine"]
    H = config_for("bert-tiny").hidden
    path = str(tmp_path / "corpus.npy")
    np.save(path, torch.randn(300, H, generator=torch.Generator().manual_seed(8)).numpy())
    job = {"corpus_uri": path, "model_path": MODEL,
           "compression": {"type": "pq", "subvectors": H // 8, "train_rows": 256, "train_iterations": 2}}
    payloads = [
        dict(job, queries=texts[:3], top_k=2, refine={"candidates": 64}),
        dict(job, queries=texts[3:5], top_k=7, refine={"store": "host", "vectors": "float16", "candidates": 64}),  # the same
        dict(job, queries=texts[5:], top_k=3, refine={"candidates": 96}),
        dict(job, queries=texts[:2], top_k=3, refine={"candidates": 64, "vectors": "float32"}),
        dict(job, queries=texts[:2], top_k=3),
    ]
    calls, real = [], ms.search_queries_pq

    def counting(*a, **kw):
        calls.append(a[8] if len(a) > 8 else kw.get("refine"))
        return real(*a, **kw)

    ms.search_queries_pq = counting
    try:
        res = registry.get_batch_op("map_search")([dict(p) for p in payloads])
    finally:
        ms.search_queries_pq = real
    assert [r[0] for r in res] == ["ok"] * 5
    assert sorted(calls, key=str) == sorted([(64, "float16", "host"), (96, "float16", "host"), (64, "float32", "host"), None],
                                            key=str)  # jobs 0 and 1 share one search
    for n in range(5):
        one, got = search(dict(payloads[n])), res[n][1]
        assert set(one) == set(got), n
        for key in one:
            if key not in ("elapsed_ms", "queries_per_sec", "index_cached"):
                assert got[key] == one[key], (n, key)
    assert "refine" not in res[4][1] and res[2][1]["refine"]["candidates"] == 96
