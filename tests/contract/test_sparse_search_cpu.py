"""map_sparse_search on CPU engines: every error, the query_terms form against a dense int64 computation, the npz
round trip of map_sparse_embed and lease batching."""
import os

import numpy as np
import pytest

from agent_tpu_amd.runtime import search as rs
from agent_tpu_amd.runtime import sparse_index as rsi
from agent_tpu_amd.utils.synthetic import make_text_rows

MODEL = "bert-tiny?mlm=1&batch=4&seq=40&seed=3"
CONTRACT = os.path.join(os.path.dirname(__file__), "..", "..", "ops", "map_sparse_search.CONTRACT.md")
N, V = 9000, 50  # two blocks


@pytest.fixture()
def ops_(monkeypatch):
    monkeypatch.setenv("CLASSIFY_DEVICE", "cpu")
    for name in ("TASKS", "SEARCH_INDEX_MAX_GB"):
        monkeypatch.delenv(name, raising=False)
    rs.clear_cache()
    from ops import get_batch_op, get_op, map_sparse_search
    yield get_op("map_sparse_search"), get_batch_op("map_sparse_search"), map_sparse_search.ERRORS
    rs.clear_cache()


def matrix():
    rng = np.random.default_rng(0)
    dense = ((rng.random((N, V)) < 0.1) * (4 * rng.random((N, V)))).astype(np.float32)
    dense[:, 2] = 0
    dense[::3, 2] = 1.0  # token 2: ties
    return dense


@pytest.fixture(scope="module")
def corpus(tmp_path_factory):
    dense = matrix()
    path = str(tmp_path_factory.mktemp("sparse") / "c.npz")
    _save(path, dense)
    return dense, path


def _save(path, dense):
    r, c = np.nonzero(dense)
    rsi.save_csr(path, np.concatenate([[0], np.cumsum((dense != 0).sum(1))]), c, dense[r, c], dense.shape)


def _brute(dense, ids, ws, k):
    c = np.rint(dense[:, ids].astype(np.float16).astype(np.float64) * np.asarray(ws, np.float32).astype(np.float64)
                * 2.0 ** 32).astype(np.int64).sum(1)
    s = c.astype(np.float32) * np.float32(2.0 ** -32)
    order = np.argsort(-s, kind="stable")[:k]
    order = order[c[order] > 0]
    return order.tolist(), s[order].tolist()


def test_query_terms_equal_the_dense_int64_computation(ops_, corpus):
    run, _, _ = ops_
    dense, path = corpus
    rng = np.random.default_rng(1)
    qs = [([2], [1.0]), (list(range(V)), rng.random(V).tolist()), ([7, 3, 11], [0.3, 1e-9, 255.5]), ([], [])]
    out = run({"corpus_uri": path, "top_k": 32,
               "query_terms": [{"token_ids": i, "weights": w} for i, w in qs]})
    assert (out["row_count"], out["corpus_rows"], out["vocab_size"], out["nnz"]) == (4, N, V, int((dense != 0).sum()))
    for got, (ids, ws) in zip(out["results"], qs):
        want = _brute(dense, ids, ws, 32) if ids else ([], [])
        assert (got["ids"], got["scores"], got["hits"]) == (want[0], want[1], len(want[0]))
    assert out["results"][0]["ids"] == list(range(0, 96, 3))  # equal scores: by id
    assert run({"corpus_uri": path, "query_terms": []})["index_cached"] is True
    packed = path[:-4] + "_z.npz"  # compressed members (scipy's default) cannot be mapped: the same index
    with np.load(path) as z:
        np.savez_compressed(packed, **{n: z[n] for n in z.files})
    assert run({"corpus_uri": packed, "top_k": 32, "query_terms": [{"token_ids": qs[1][0], "weights": qs[1][1]}]}
               )["results"][0] == out["results"][1]


def _bad_corpus(tmp_path, kind):
    dense = np.zeros((3, 8), np.float32)
    dense[0, 1], dense[2, 5] = 1.0, 2.0
    path = str(tmp_path / f"{kind}.npz")
    if kind == "corpus_file":
        np.savez(path, indptr=np.arange(4))
    elif kind == "corpus_values":
        dense[0, 1] = 300.0
        _save(path, dense)
    else:
        _save(path, dense[:0])
    return path


def test_every_error_message(ops_, corpus, tmp_path, monkeypatch):
    run, _, errors = ops_
    _, path = corpus
    q = {"query_terms": [{"token_ids": [1], "weights": [1.0]}]}
    cases = {
        "corpus": q, "missing": {"corpus_uri": path}, "both": dict(q, corpus_uri=path, queries=["a"]),
        "queries": {"corpus_uri": path, "queries": "a"},
        "query_terms": {"corpus_uri": path, "query_terms": [{"token_ids": [1, 2], "weights": [1.0]}]},
        "token_ids": {"corpus_uri": path, "query_terms": [{"token_ids": [1, 1], "weights": [1.0, 1.0]}]},
        "weights": {"corpus_uri": path, "query_terms": [{"token_ids": [1], "weights": [256.5]}]},
        "top_k": dict(q, corpus_uri=path, top_k=33), "max_query_terms": dict(q, corpus_uri=path, max_query_terms=0),
        "mlm": {"corpus_uri": path, "queries": ["a"], "model_path": "bert-tiny?batch=4&seq=40"},
        "vocab": {"corpus_uri": path, "queries": ["a"], "model_path": MODEL},
        "corpus_file": dict(q, corpus_uri=_bad_corpus(tmp_path, "corpus_file")),
        "corpus_values": dict(q, corpus_uri=_bad_corpus(tmp_path, "corpus_values")),
        "corpus_empty": dict(q, corpus_uri=_bad_corpus(tmp_path, "corpus_empty")),
        "sparse_too_large": dict(q, corpus_uri=path),
    }
    assert set(cases) == set(errors)
    with pytest.raises(ValueError) as e:  # an id past the vocabulary of this corpus
        run({"corpus_uri": path, "query_terms": [{"token_ids": [V], "weights": [1.0]}]})
    assert str(e.value) == errors["token_ids"]
    text = open(CONTRACT).read()
    for key, payload in cases.items():
        if key == "sparse_too_large":
            monkeypatch.setenv("SEARCH_INDEX_MAX_GB", "1e-6")
            rs.clear_cache()
        with pytest.raises(ValueError) as e:
            run(payload)
        assert str(e.value) == errors[key] and f"`{errors[key]}`" in text, key


def test_npz_round_trip_and_text_search(ops_, tmp_path):
    run, _, _ = ops_
    from ops import get_op
    texts = make_text_rows(12, words_per_row=7, seed=8) + [""]
    path = str(tmp_path / "rows.npz")
    want = get_op("map_sparse_embed")({"texts": texts, "model_path": MODEL, "max_terms": 64, "min_weight": 0.5})
    got = get_op("map_sparse_embed")({"texts": texts, "model_path": MODEL, "max_terms": 64, "min_weight": 0.5,
                                      "output": "npz", "output_uri": path})
    assert "terms" not in got and got["shape"] == [13, want["vocab_size"]] and got["nnz"] == want["nnz"]
    with np.load(path, allow_pickle=False) as z:
        indptr, indices, data = z["indptr"], z["indices"], z["data"]
        assert z["format"].item() == b"csr" and z["shape"].tolist() == got["shape"] and data.dtype == np.float32
    assert got["stored"] == len(data) == sum(len(t["token_ids"]) for t in want["terms"]) and data.min() >= 0.5
    for r, t in enumerate(want["terms"]):
        pairs = sorted(zip(t["token_ids"], t["weights"]))
        assert indices[indptr[r]:indptr[r + 1]].tolist() == [p[0] for p in pairs]  # ascending tokens
        np.testing.assert_allclose(data[indptr[r]:indptr[r + 1]], [p[1] for p in pairs], atol=1e-6, rtol=0)
    from ops.map_sparse_embed import OUTPUT_ERRORS
    for bad, key in (({"output": "csv"}, "output"), ({"output": "npz"}, "output_uri")):
        with pytest.raises(ValueError) as e:
            get_op("map_sparse_embed")(dict({"texts": texts, "model_path": MODEL}, **bad))
        assert str(e.value) == OUTPUT_ERRORS[key]
    out = run({"corpus_uri": path, "queries": texts[:3], "model_path": MODEL, "top_k": 3, "max_query_terms": 64})
    assert [r["ids"][0] for r in out["results"]] == [0, 1, 2] and out["model_path"]  # a text retrieves itself first


def test_lease_batching_gives_single_job_results(ops_, corpus):
    run, batch, errors = ops_
    _, path = corpus
    jobs = [{"corpus_uri": path, "query_terms": [{"token_ids": [2, 9], "weights": [1.0, 0.7]}], "top_k": 4},
            {"corpus_uri": path, "query_terms": [{"token_ids": [4], "weights": [2.0]}, {"token_ids": [2], "weights": [3.0]}],
             "top_k": 32},
            {"corpus_uri": path, "query_terms": [{"token_ids": [4], "weights": [-1.0]}]}]
    out = batch(jobs)
    skip = ("elapsed_ms", "rows_per_sec", "index_cached")
    for (kind, got), job in zip(out[:2], jobs):
        want = run(job)
        assert kind == "ok" and {k: v for k, v in got.items() if k not in skip} == \
            {k: v for k, v in want.items() if k not in skip}
    assert out[2][0] == "err" and str(out[2][1]) == errors["weights"]
