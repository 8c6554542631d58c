"""map_search on a CPU engine: the sim_topk twin, the op's forms, the corpus cache, errors and
lease batching."""
import json
import os

import numpy as np
import pytest
import torch

import ops as registry
from agent_tpu_amd import ops
from agent_tpu_amd.runtime import search as rs

MODEL = "bert-tiny?batch=8&seq=32&seed=4"
TEXTS = ["the quick brown fox", "jumps over, the lazy dog!", "MI355X " * 30, "x", "seven rows in all",
         "an index of sentence vectors", "nearest neighbours by cosine", "a corpus row", "another corpus row",
         "the last one"]


# ------------------------------------------------------------------- twin
def _brute(q, c, k, id_base=0):
    """Brute force in fp64: python sort on (-score, id)."""
    s = (q.double().unsqueeze(1) * c.double().unsqueeze(0)).sum(-1)
    ids, scores = [], []
    for row in s.tolist():
        order = sorted(range(len(row)), key=lambda j: (-row[j], j))[:k]
        ids.append([id_base + j for j in order])
        scores.append([row[j] for j in order])
    return torch.tensor(scores, dtype=torch.float64), torch.tensor(ids, dtype=torch.int64)


def test_twin_against_brute_force_and_its_options():
    gen = torch.Generator().manual_seed(0)
    q, c = torch.randn(7, 64, generator=gen), torch.randn(50, 64, generator=gen)
    ws, wi = _brute(q, c, 10)
    s, i = ops.sim_topk_ref(q, c, 10, dtype=torch.float64)
    assert torch.equal(i, wi) and torch.allclose(s, ws, atol=1e-12, rtol=0)
    s32, i32 = ops.sim_topk(q, c, 10)  # the CPU path of the wrapper is the fp32 twin
    assert s32.dtype == torch.float32 and i32.dtype == torch.int64 and torch.equal(i32, wi)
    assert torch.allclose(s32.double(), ws, atol=1e-4, rtol=0)
    # kk = min(k, N)
    s, i = ops.sim_topk(q, c[:4].contiguous(), 10)
    assert s.shape == i.shape == (7, 4) and sorted(i[0].tolist()) == [0, 1, 2, 3]
    # id_base offsets the ids and nothing else
    sb, ib = ops.sim_topk(q, c, 10, id_base=12345)
    assert torch.equal(sb, s32) and torch.equal(ib, i32 + 12345)
    s0, i0 = ops.sim_topk(torch.zeros((0, 64)), c, 3)
    assert s0.shape == i0.shape == (0, 3)


def test_ties_come_back_in_ascending_id():
    gen = torch.Generator().manual_seed(1)
    base = torch.randint(-2, 3, (5, 64), generator=gen).float()
    c = base[torch.tensor([0, 1, 0, 2, 1, 0, 3, 4, 4, 0])].contiguous()
    q = torch.randint(-2, 3, (6, 64), generator=gen).float()
    s, i = ops.sim_topk(q, c, 10)
    ws, wi = _brute(q, c, 10)
    assert torch.equal(i, wi) and torch.equal(s.double(), ws)  # integer data: exact
    same = s[:, 1:] == s[:, :-1]
    assert same.any() and (i[:, 1:][same] > i[:, :-1][same]).all()
    # all scores equal (a zero query): every row ties, ascending id
    assert ops.sim_topk(torch.zeros(1, 64), c, 10)[1].tolist() == [list(range(10))]


def test_sim_topk_ok_names_the_supported_shapes():
    for D, k in ((64, 1), (768, 10), (1024, 32), (128, 17)):
        assert ops.sim_topk_ok(D, k)
    for D, k in ((96, 10), (1088, 10), (32, 10), (0, 1), (768, 0), (768, 33)):
        assert not ops.sim_topk_ok(D, k)
    q = torch.zeros(2, 64)
    for bad in (lambda: ops.sim_topk(torch.zeros(2, 96), torch.zeros(4, 96), 2),
                lambda: ops.sim_topk(q, torch.zeros(4, 64), 0),
                lambda: ops.sim_topk(q, torch.zeros(4, 64), 33),
                lambda: ops.sim_topk(q, torch.zeros(0, 64), 2),
                lambda: ops.sim_topk(q, torch.zeros(4, 128), 2),
                lambda: ops.sim_topk(q, torch.zeros(4, 128)[:, ::2], 2),
                lambda: ops.sim_topk(q.double(), torch.zeros(4, 64), 2)):
        with pytest.raises(ValueError):
            bad()


def test_merge_topk_is_the_same_total_order():
    s = torch.tensor([[3.0, 1.0, float("-inf"), 3.0, 2.0, float("-inf")]])
    i = torch.tensor([[7, 9, 2 ** 62, 4, 5, 2 ** 62]])
    ms, mi = rs.merge_topk(s, i, 5)
    assert mi.tolist() == [[4, 7, 5, 9, 2 ** 62]] and ms.tolist() == [[3.0, 3.0, 2.0, 1.0, float("-inf")]]
    # +0.0 and -0.0 tie: the lower id first, whichever came first
    assert rs.merge_topk(torch.tensor([[0.0, -0.0]]), torch.tensor([[1, 0]]), 2)[1].tolist() == [[0, 1]]
    assert rs.merge_topk(torch.tensor([[-0.0, 0.0]]), torch.tensor([[1, 0]]), 2)[1].tolist() == [[0, 1]]


# --------------------------------------------------------------------- op
@pytest.fixture
def search(monkeypatch):
    monkeypatch.setenv("CLASSIFY_DEVICE", "cpu")
    monkeypatch.delenv("TASKS", raising=False)
    rs.clear_cache()
    yield registry.get_op("map_search")
    rs.clear_cache()


def _corpus(tmp_path, dtype="float32", name="corpus.npy"):
    path = str(tmp_path / name)
    res = registry.get_op("map_embed")({"texts": TEXTS, "model_path": MODEL, "output": "npy", "output_uri": path,
                                        "dtype": dtype})
    assert res["ok"] and res["shape"] == [len(TEXTS), 256]
    return path


def test_corpus_written_by_map_embed_finds_its_own_rows(search, tmp_path):
    path = _corpus(tmp_path)
    res = search({"queries": TEXTS, "corpus_uri": path, "model_path": MODEL, "top_k": 3})
    for key in ("ok", "op", "query_count", "corpus_rows", "dim", "top_k", "metric", "elapsed_ms", "queries_per_sec",
                "model_path", "pooling", "index_cached", "ids", "scores"):
        assert key in res, key
    assert res["op"] == "map_search" and res["query_count"] == len(TEXTS) == res["corpus_rows"] and res["dim"] == 256
    assert res["metric"] == "cosine" and res["top_k"] == 3 and res["pooling"] == "mean" and "dp_world_size" not in res
    json.dumps(res)
    for a, (ids, scores) in enumerate(zip(res["ids"], res["scores"])):
        assert len(ids) == len(scores) == 3 and ids[0] == a and abs(scores[0] - 1.0) <= 1e-5
        assert scores == sorted(scores, reverse=True)
    # the float16 file is widened on load: same neighbours, scores within fp16 rounding of unit rows
    p16 = _corpus(tmp_path, "float16", "corpus16.npy")
    assert np.load(p16).dtype == np.float16
    r16 = search({"queries": TEXTS, "corpus_uri": "file://" + p16, "model_path": MODEL, "top_k": 1})
    assert [r[0] for r in r16["ids"]] == list(range(len(TEXTS)))
    assert all(abs(r[0] - 1.0) <= 1e-5 for r in r16["scores"])  # cosine renormalises the widened rows
    # top_k above the corpus size: min(top_k, rows) entries
    assert [len(r) for r in search({"queries": TEXTS[:2], "corpus_uri": path, "model_path": MODEL,
                                    "top_k": 32})["ids"]] == [10, 10]


def test_query_vectors_with_dot_metric_are_exact_on_integer_data(search, tmp_path):
    gen = torch.Generator().manual_seed(3)
    c = torch.randint(-2, 3, (21, 64), generator=gen).float()
    c[7] = c[3]
    q = torch.randint(-2, 3, (4, 64), generator=gen).float()
    path = str(tmp_path / "ints.npy")
    np.save(path, c.numpy())
    res = search({"query_vectors": q.tolist(), "corpus_uri": path, "metric": "dot", "top_k": 6})
    ws, wi = _brute(q, c, 6)
    assert res["ids"] == wi.tolist() and res["scores"] == ws.tolist()
    assert "model_path" not in res and "pooling" not in res and res["dim"] == 64 and res["metric"] == "dot"
    cos = search({"query_vectors": q.tolist(), "corpus_uri": path, "top_k": 2})
    want = torch.nn.functional.normalize(q.double(), dim=1) @ torch.nn.functional.normalize(c.double(), dim=1).T
    assert np.allclose(cos["scores"], torch.sort(want, dim=1, descending=True).values[:, :2].numpy(), atol=1e-6)


def test_corpus_texts_and_min_score(search):
    res = search({"queries": TEXTS[2:4], "corpus_texts": TEXTS, "model_path": MODEL, "top_k": 4})
    assert [r[0] for r in res["ids"]] == [2, 3] and "index_cached" not in res and res["corpus_rows"] == len(TEXTS)
    cut = (res["scores"][0][1] + res["scores"][0][2]) / 2
    low = search({"queries": TEXTS[2:4], "corpus_texts": TEXTS, "model_path": MODEL, "top_k": 4, "min_score": cut})
    assert low["ids"][0] == res["ids"][0][:2] and low["scores"][0] == res["scores"][0][:2]
    assert all(v >= cut for row in low["scores"] for v in row) and low["top_k"] == 4
    assert search({"queries": TEXTS[:1], "corpus_texts": TEXTS, "model_path": MODEL, "min_score": 2.0})["ids"] == [[]]


def test_index_cache_hits_and_misses_a_rewritten_file(search, tmp_path):
    path = _corpus(tmp_path)
    job = {"queries": TEXTS[:2], "corpus_uri": path, "model_path": MODEL, "top_k": 2}
    first, second = search(dict(job)), search(dict(job))
    assert first["index_cached"] is False and second["index_cached"] is True
    assert first["ids"] == second["ids"] and first["scores"] == second["scores"]
    arr = np.load(path)
    st = os.stat(path)
    np.save(path, arr[::-1].copy())
    os.utime(path, ns=(st.st_atime_ns, st.st_mtime_ns + 1_000_000))  # a rewrite within the clock's tick still counts
    third = search(dict(job))
    assert third["index_cached"] is False and [r[0] for r in third["ids"]] == [9, 8]
    assert search(dict(job, metric="dot"))["index_cached"] is False  # normalize is part of the key


def test_errors_are_fixed_and_listed_in_the_contract(search, tmp_path, monkeypatch):
    from ops import map_search as ms

    contract = open(os.path.join(os.path.dirname(ms.__file__), "map_search.CONTRACT.md")).read()
    for msg in ms.ERRORS.values():
        assert msg in contract, msg
    for key, msg in rs.ERRORS.items():
        assert ms.ERRORS[key] == msg
    good = _corpus(tmp_path)
    np.save(str(tmp_path / "f64.npy"), np.zeros((3, 256)))
    np.save(str(tmp_path / "d1.npy"), np.zeros(256, dtype=np.float32))
    np.save(str(tmp_path / "empty.npy"), np.zeros((0, 256), dtype=np.float32))
    np.save(str(tmp_path / "d64.npy"), np.ones((3, 64), dtype=np.float32))
    bad = np.ones((3, 256), dtype=np.float32)
    bad[1, 5] = np.inf
    np.save(str(tmp_path / "inf.npy"), bad)
    with open(tmp_path / "text.npy", "w") as f:
        f.write("not an npy file")
    t = lambda name: str(tmp_path / name)  # noqa: E731
    q = {"queries": ["a"], "model_path": MODEL}
    cases = [
        ("missing_queries", {"corpus_uri": good}),
        ("missing_corpus", dict(q)),
        ("queries", {"queries": "a string", "corpus_uri": good}),
        ("query_vectors", {"query_vectors": [[1.0, 2.0], [1.0]], "corpus_uri": good}),
        ("query_vectors", {"query_vectors": [[1.0, "x"]], "corpus_uri": good}),
        ("query_vectors", {"query_vectors": "nope", "corpus_uri": good}),
        ("query_vectors", {"query_vectors": [[]], "corpus_uri": good}),
        ("query_vectors", {"query_vectors": [[float("nan")] * 256], "corpus_uri": good}),
        ("corpus_texts", {"query_vectors": [[1.0] * 256], "corpus_texts": ["a"]}),
        ("corpus_texts", dict(q, corpus_texts="a string")),
        ("top_k", dict(q, corpus_uri=good, top_k=0)),
        ("top_k", dict(q, corpus_uri=good, top_k=33)),
        ("top_k", dict(q, corpus_uri=good, top_k="3")),
        ("metric", dict(q, corpus_uri=good, metric="l2")),
        ("pooling", dict(q, corpus_uri=good, pooling="max")),
        ("min_score", dict(q, corpus_uri=good, min_score="high")),
        ("corpus_file", dict(q, corpus_uri=t("f64.npy"))),
        ("corpus_file", dict(q, corpus_uri=t("d1.npy"))),
        ("corpus_file", dict(q, corpus_uri=t("text.npy"))),
        ("corpus_file", dict(q, corpus_uri=t("missing.npy"))),
        ("corpus_file", dict(q, corpus_uri="s3://bucket/corpus.npy")),
        ("corpus_file", dict(q, corpus_uri=17)),
        ("corpus_empty", dict(q, corpus_uri=t("empty.npy"))),
        ("corpus_empty", dict(q, corpus_texts=[])),
        ("corpus_nonfinite", dict(q, corpus_uri=t("inf.npy"))),
        ("dim", dict(q, corpus_uri=t("d64.npy"))),
        ("dim", {"query_vectors": [[1.0] * 64], "corpus_uri": good}),
    ]
    for key, payload in cases:
        with pytest.raises(ValueError) as ei:
            search(payload)
        assert str(ei.value) == ms.ERRORS[key], (key, payload)
    monkeypatch.setenv("SEARCH_INDEX_MAX_GB", str(9 * 256 * 4 / 2 ** 30))  # 9 rows of 256 floats
    rs.clear_cache()
    with pytest.raises(ValueError) as ei:
        search(dict(q, corpus_uri=good))
    assert str(ei.value) == ms.ERRORS["corpus_too_large"]
    assert {k for k, _ in cases} | {"corpus_too_large"} == set(ms.ERRORS)
    with pytest.raises(ValueError) as ei:
        search(None)
    assert str(ei.value) == ms.ERRORS["missing_queries"]
    with pytest.raises(FileNotFoundError):  # no fallback stub
        search({"queries": ["a"], "corpus_uri": good, "model_path": "/nope/model.safetensors"})


def test_batch_handler_gives_every_job_its_single_job_result(search, tmp_path):
    from ops import map_search as ms

    path = _corpus(tmp_path)
    batch = registry.get_batch_op("map_search")
    assert batch is not None
    payloads = [
        {"queries": TEXTS[:3], "corpus_uri": path, "model_path": MODEL, "top_k": 2},
        {"queries": TEXTS[3:5], "corpus_uri": path, "model_path": MODEL, "top_k": 40},
        {"queries": TEXTS[5:], "corpus_uri": path, "model_path": MODEL, "top_k": 7, "min_score": 0.1},
    ]
    res = batch([dict(p) for p in payloads])
    assert [r[0] for r in res] == ["ok", "err", "ok"]
    assert isinstance(res[1][1], ValueError) and str(res[1][1]) == ms.ERRORS["top_k"]
    for n in (0, 2):
        one, got = search(dict(payloads[n])), res[n][1]
        assert set(one) == set(got), n
        for key in one:
            if key not in ("elapsed_ms", "queries_per_sec", "index_cached"):
                assert got[key] == one[key], (n, key)  # ids equal, scores ==
    # jobs of other forms and other groups ride along on the single-job path
    mixed = batch([{"queries": TEXTS[:1], "corpus_texts": TEXTS, "model_path": MODEL, "top_k": 1},
                   {"query_vectors": np.load(path)[:2].tolist(), "corpus_uri": path, "top_k": 1},
                   {"queries": TEXTS[:1], "corpus_uri": path, "model_path": MODEL, "metric": "dot", "top_k": 1},
                   {"corpus_uri": path}])
    assert [r[0] for r in mixed] == ["ok", "ok", "ok", "err"] and str(mixed[3][1]) == ms.ERRORS["missing_queries"]
    assert mixed[0][1]["ids"] == [[0]] and mixed[1][1]["ids"] == [[0], [1]] and mixed[2][1]["ids"] == [[0]]
