"""map_search with ``diversify`` (MMR) on a CPU engine. The corpus holds every distinct row three times, so the plain
search returns copies of one row first; the picks are checked against a plain fp64 replay of the contract's formula."""
import numpy as np
import pytest
import torch

import ops as registry
from agent_tpu_amd.runtime import search as rs
from ops import map_search as ms

MODEL = "bert-tiny?batch=8&seq=32&seed=4"
TEXTS = ["the quick brown fox", "jumps over, the lazy dog!", "x", "seven rows in all", "nearest neighbours by cosine"]


@pytest.fixture
def search(monkeypatch):
    monkeypatch.setenv("CLASSIFY_DEVICE", "cpu")
    for name in ("TASKS", "SEARCH_INDEX_DTYPE", "SEARCH_INDEX_MAX_GB"):
        monkeypatch.delenv(name, raising=False)
    rs.clear_cache()
    yield registry.get_op("map_search")
    rs.clear_cache()


def _corpus(tmp_path, D, seed=0):
    gen = torch.Generator().manual_seed(seed)
    base = torch.randn(12, D, generator=gen)
    c = base[torch.arange(36) % 12].contiguous()  # rows j, j + 12 and j + 24 are equal
    path = str(tmp_path / f"dup{D}.npy")
    np.save(path, c.numpy())
    return c, path


def _replay(c, q, ids, lam, R):
    """The picks in fp64 from the job's own candidate order: (ids, mmr) of one query."""
    cn, qn = rs.normalize_rows(c).double(), rs.normalize_rows(q[None]).double()[0]
    rel, G = cn[ids] @ qn, cn[ids] @ cn[ids].T
    picked, out = [], []
    for _ in range(len(ids)):
        v = [lam * rel[j] - ((1 - lam) * max(G[j][p] for p in picked) if picked else 0.0) for j in range(R)]
        best = max((j for j in range(R) if j not in picked), key=lambda j: (v[j], -ids[j]))
        picked.append(best)
        out.append(float(v[best]))
    return [ids[j] for j in picked], out


def test_diversify_returns_distinct_content_in_pick_order_with_its_keys(search, tmp_path):
    c, path = _corpus(tmp_path, 64)
    q = c[:4] + 0.5 * torch.randn(4, 64, generator=torch.Generator().manual_seed(1))
    job = {"query_vectors": q.tolist(), "corpus_uri": path, "top_k": 3}
    plain = search(dict(job))
    res = search(dict(job, diversify={"lambda": 0.25, "candidates": 12}))
    assert list(res) == list(plain) + ["mmr_scores", "diversify"] and res["diversify"] == {"lambda": 0.25, "candidates": 12}
    cand = search(dict(job, top_k=12))
    for a in range(4):
        assert {i % 12 for i in plain["ids"][a]} == {a}  # three copies of one row
        assert len({i % 12 for i in res["ids"][a]}) == 3 and res["ids"][a][0] == plain["ids"][a][0]
        ids, mmr = _replay(c, q[a], cand["ids"][a], 0.25, 12)
        assert res["ids"][a] == ids[:3] and np.allclose(res["mmr_scores"][a], mmr[:3], atol=1e-5, rtol=0)
        assert res["scores"][a] == [cand["scores"][a][cand["ids"][a].index(i)] for i in res["ids"][a]]  # relevance
    # defaults: lambda 0.5 over the top 32; lambda 1 is the plain list; a job without the key keeps its keys
    dflt = search(dict(job, diversify={}))
    assert dflt["diversify"] == {"lambda": 0.5, "candidates": 32}
    assert dflt["ids"] == search(dict(job, diversify={"lambda": 0.5, "candidates": 32}))["ids"]
    one = search(dict(job, diversify={"lambda": 1}))
    assert one["ids"] == plain["ids"] and one["scores"] == plain["scores"] and one["mmr_scores"] == plain["scores"]
    after = search(dict(job))
    assert list(after) == list(plain) and after["ids"] == plain["ids"] and after["scores"] == plain["scores"]
    # min_score drops entries by relevance, from all three lists
    floor = sorted(res["scores"][0])[1]
    cut = search(dict(job, diversify={"lambda": 0.25, "candidates": 12}, min_score=floor))
    keep = [j for j, v in enumerate(res["scores"][0]) if v >= floor]
    assert cut["ids"][0] == [res["ids"][0][j] for j in keep] and len(cut["mmr_scores"][0]) == len(keep) == 2


@pytest.mark.parametrize("extra", [{"metric": "dot"}, {"corpus_dtype": "float16"}, {"filter": {"exclude_ids": [0, 13]}}])
def test_diversify_with_the_other_forms(search, tmp_path, extra):
    c, path = _corpus(tmp_path, 64)
    job = dict({"query_vectors": c[:2].tolist(), "corpus_uri": path, "top_k": 4}, **extra)
    res = search(dict(job, diversify={"lambda": 0.25, "candidates": 12}))
    cand = search(dict(job, top_k=12))
    for a in range(2):
        assert set(res["ids"][a]) <= set(cand["ids"][a]) and len({i % 12 for i in res["ids"][a]}) == 4
        assert res["ids"][a][0] == cand["ids"][a][0]
    texts = search({"queries": TEXTS[:2], "corpus_texts": TEXTS + TEXTS, "model_path": MODEL, "top_k": 2,
                    "diversify": {"lambda": 0.25, "candidates": 10}})
    assert [len({i % 5 for i in row}) for row in texts["ids"]] == [2, 2] and len(texts["mmr_scores"][0]) == 2


def test_every_diversify_error_and_the_existing_errors_first(search, tmp_path):
    _, path = _corpus(tmp_path, 64)
    job = {"query_vectors": [[1.0] * 64], "corpus_uri": path, "top_k": 1, "diversify": {"candidates": 2}}
    pq = {"type": "pq", "subvectors": 16}
    for bad in ([], "mmr", {"lambda": 1.5}, {"lambda": -0.1}, {"lambda": "0.5"}, {"lambda": True}, {"lambda": float("nan")},
                {"candidates": 33}, {"candidates": 4}, {"candidates": 8.0}, {"candidates": 8, "fetch_k": 20}):
        with pytest.raises(ValueError) as e:
            search(dict(job, top_k=5, diversify=bad))
        assert str(e.value) == ms.DIVERSIFY_ERRORS["diversify"], bad
    for extra, msg in [({"top_k": 1, "diversify": {"candidates": 1}}, ms.DIVERSIFY_ERRORS["diversify"]),  # below 2
                       ({"index": {"type": "ivf"}}, ms.DIVERSIFY_ERRORS["diversify_index"]),
                       ({"index": {"type": "ivfpq", "subvectors": 16}}, ms.DIVERSIFY_ERRORS["diversify_index"]),
                       ({"compression": pq}, ms.DIVERSIFY_ERRORS["diversify_compression"]),
                       ({"compression": {"type": "binary"}}, ms.DIVERSIFY_ERRORS["diversify_compression"]),
                       ({"compression": pq, "refine": {"candidates": 32}}, ms.DIVERSIFY_ERRORS["diversify_compression"]),
                       ({"top_k": 33}, ms.ERRORS["top_k"]), ({"top_k": 33, "diversify": 7}, ms.ERRORS["top_k"]),
                       ({"index": {"type": "ivf"}, "filter": {"ids": [1]}}, ms.IVF_ERRORS["index_filter"]),
                       ({"compression": {"type": "pq"}}, ms.PQ_ERRORS["compression"]),
                       ({"corpus_uri": "s3://bucket/x.npy"}, ms.ERRORS["corpus_file"]),
                       ({"refine": {"candidates": 32}}, ms.REFINE_ERRORS["refine_compression"])]:
        with pytest.raises(ValueError) as e:
            search(dict(job, **extra))
        assert str(e.value) == msg, extra


def test_a_lease_batch_with_two_top_ks_gives_every_job_its_single_job_result(search, tmp_path):
    _, path = _corpus(tmp_path, 256, seed=3)
    dv = {"lambda": 0.75, "candidates": 16}
    payloads = [{"queries": TEXTS[:2], "corpus_uri": path, "model_path": MODEL, "top_k": 2, "diversify": dv},
                {"queries": TEXTS[2:], "corpus_uri": path, "model_path": MODEL, "top_k": 9, "diversify": dict(dv)},
                {"queries": TEXTS[:1], "corpus_uri": path, "model_path": MODEL, "top_k": 3},
                {"queries": TEXTS[:1], "corpus_uri": path, "model_path": MODEL, "top_k": 3, "diversify": {"lambda": 0.5}}]
    res = registry.get_batch_op("map_search")([dict(p) for p in payloads])
    assert [r[0] for r in res] == ["ok"] * 4
    for n, p in enumerate(payloads):
        one, got = search(dict(p)), res[n][1]
        assert list(got) == list(one) and ("mmr_scores" in got) == ("diversify" in p)
        for key in one:
            if key not in ("elapsed_ms", "queries_per_sec", "index_cached"):
                assert got[key] == one[key], (n, key)
    assert len(res[1][1]["ids"][0]) == 9 and res[1][1]["ids"] != search(dict(payloads[1], diversify={"lambda": 1}))["ids"]
