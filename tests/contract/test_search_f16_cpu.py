"""map_search with a float16-resident corpus on a CPU engine: ``corpus_dtype`` and its environment
default, the loader (rounding, range, size, cache, resident bytes), the twin's ``row_scale`` and
lease batching.

Cosine tolerance (tests/kernels/test_search_f16_gpu.py): ``(D + 2) * 2^-24 * scale * sum_k |q_k c_k|``
in fp64 for an fp32 chain of length D over the stored fp16 values and one fp32 multiply by the
once-rounded scale. The queries here are unit vectors whose fp32 normalisation is exact.
"""
import os

import numpy as np
import pytest
import torch

import ops as registry
from agent_tpu_amd import ops
from agent_tpu_amd.runtime import search as rs

U = 2.0 ** -24
MODEL = "bert-tiny?batch=8&seq=32&seed=4"
TEXTS = ["the quick brown fox", "jumps over, the lazy dog!", "x", "seven rows in all", "an index of sentence vectors",
         "nearest neighbours by cosine", "a corpus row"]
N, D = 21, 64


@pytest.fixture
def search(monkeypatch):
    monkeypatch.setenv("CLASSIFY_DEVICE", "cpu")
    monkeypatch.delenv("TASKS", raising=False)
    monkeypatch.delenv("SEARCH_INDEX_DTYPE", raising=False)
    rs.clear_cache()
    yield registry.get_op("map_search")
    rs.clear_cache()


def _rows(seed=3):
    gen = torch.Generator().manual_seed(seed)
    return torch.randn(N, D, generator=gen) * torch.linspace(0.5, 3.0, N).unsqueeze(1)  # norms differ: dot != cosine


def _unit_queries():
    """+-1/8 in all 64 places: norm exactly 1 and the fp32 normalisation returns them unchanged."""
    gen = torch.Generator().manual_seed(9)
    return (torch.randint(0, 2, (4, D), generator=gen).float() * 2 - 1) / 8


def _save(tmp_path, name, arr):
    path = str(tmp_path / name)
    np.save(path, arr)
    return path


def test_corpus_dtype_values_and_the_environment_default(search, tmp_path, monkeypatch):
    from ops import map_search as ms

    contract = open(os.path.join(os.path.dirname(ms.__file__), "map_search.CONTRACT.md")).read()
    for msg in ms.F16_ERRORS.values():
        assert msg in contract, msg
    for key, msg in rs.F16_ERRORS.items():
        assert ms.F16_ERRORS[key] == msg
    assert ms.F16_ERRORS["corpus_dtype"] == "payload.corpus_dtype must be 'float32' or 'float16'"
    path = _save(tmp_path, "c.npy", _rows().half().numpy())
    job = {"query_vectors": _unit_queries().tolist(), "corpus_uri": path, "top_k": 3, "metric": "dot"}
    for bad in ("bfloat16", "fp16", 16, None, ["float16"]):
        with pytest.raises(ValueError) as ei:
            search(dict(job, corpus_dtype=bad))
        assert str(ei.value) == ms.F16_ERRORS["corpus_dtype"], bad
    with pytest.raises(ValueError) as ei:  # validated with corpus_texts too, before any model is loaded
        search({"queries": ["a"], "corpus_texts": ["b"], "model_path": "/nope/model.safetensors", "corpus_dtype": "half"})
    assert str(ei.value) == ms.F16_ERRORS["corpus_dtype"]
    assert "corpus_dtype" not in search(dict(job))
    assert "corpus_dtype" not in search(dict(job, corpus_dtype="float32"))
    assert search(dict(job, corpus_dtype="float16"))["corpus_dtype"] == "float16"
    monkeypatch.setenv("SEARCH_INDEX_DTYPE", "float16")
    assert search(dict(job))["corpus_dtype"] == "float16"
    assert "corpus_dtype" not in search(dict(job, corpus_dtype="float32"))  # the payload wins
    monkeypatch.setenv("SEARCH_INDEX_DTYPE", "int8")
    with pytest.raises(ValueError) as ei:
        search(dict(job))
    assert str(ei.value) == ms.F16_ERRORS["corpus_dtype_env"]
    assert search(dict(job, corpus_dtype="float16"))["corpus_dtype"] == "float16"  # ... over a bad default too


def test_float16_file_with_dot_equals_the_default_path_exactly(search, tmp_path):
    c16 = _rows().half()
    path = _save(tmp_path, "c16.npy", c16.numpy())
    q = _unit_queries()
    job = {"query_vectors": q.tolist(), "corpus_uri": path, "top_k": 6, "metric": "dot"}
    plain, half = search(dict(job)), search(dict(job, corpus_dtype="float16"))
    assert half["ids"] == plain["ids"] and half["scores"] == plain["scores"]  # both are q @ c16.float().T
    ws, wi = ops.sim_topk_ref(q, c16.float(), 6)
    assert half["ids"] == wi.tolist() and half["scores"] == ws.tolist()
    assert half["index_cached"] is False and search(dict(job, corpus_dtype="float16"))["index_cached"] is True


def test_cosine_scores_within_the_bound_of_fp64(search, tmp_path):
    c16 = _rows().half()
    path = _save(tmp_path, "c16.npy", c16.numpy())
    q = _unit_queries()
    res = search({"query_vectors": q.tolist(), "corpus_uri": path, "top_k": 6, "corpus_dtype": "float16"})
    c = c16.double()
    scale = 1.0 / c.norm(dim=1)
    exact = (q.double() @ c.T) * scale
    tol = (D + 2) * U * scale * (q.double().abs() @ c.abs().T)
    assert not torch.equal(torch.sort(exact, dim=1, descending=True).indices[:, :6],
                           torch.sort(q.double() @ c.T, dim=1, descending=True).indices[:, :6])  # the scale matters
    for a, (ids, scores) in enumerate(zip(res["ids"], res["scores"])):
        ids = torch.tensor(ids)
        assert len(set(ids.tolist())) == 6
        assert ((torch.tensor(scores, dtype=torch.float64) - exact[a, ids]).abs() <= tol[a, ids]).all(), a
        kth_v, kth_i = torch.sort(exact[a], descending=True, stable=True)
        assert (exact[a, ids] >= kth_v[5] - tol[a, ids] - tol[a, kth_i[5]]).all(), a
        assert scores == sorted(scores, reverse=True)
    # the resident rows are the file's, unnormalised, beside the fp32 scale
    corpus = rs.load_corpus(path, normalize=True, dtype="float16")
    assert corpus.cached and corpus.vectors.dtype == torch.float16 and torch.equal(corpus.vectors, c16)
    assert corpus.scale.dtype == torch.float32 and torch.equal(corpus.scale, scale.float())
    assert rs.load_corpus(path, normalize=False, dtype="float16").scale is None


def test_float32_file_is_rounded_to_nearest_and_the_range_is_checked(search, tmp_path):
    from ops import map_search as ms

    c = _rows()
    c[0, 0], c[0, 1], c[0, 2] = 1.0 + 2.0 ** -11, 1.0 + 3 * 2.0 ** -11, 65519.0  # ties to even; the largest that rounds in
    path = _save(tmp_path, "c32.npy", c.numpy())
    q = _unit_queries()
    res = search({"query_vectors": q.tolist(), "corpus_uri": path, "top_k": 5, "metric": "dot", "corpus_dtype": "float16"})
    c16 = torch.from_numpy(c.numpy().astype(np.float16))  # numpy rounds to nearest even
    assert c16[0, 0] == 1.0 and c16[0, 1] == 1.0 + 2.0 ** -9 and c16[0, 2] == 65504.0
    assert not torch.equal(c16.float(), c)
    ws, wi = ops.sim_topk_ref(q, c16.float(), 5)
    assert res["ids"] == wi.tolist() and res["scores"] == ws.tolist()
    assert torch.equal(rs.load_corpus(path, normalize=False, dtype="float16").vectors, c16)
    for value, key in ((1e5, "corpus_f16_range"), (65520.0, "corpus_f16_range"), (-1e5, "corpus_f16_range")):
        big = c.clone()
        big[7, 3] = value
        bad = _save(tmp_path, "big.npy", big.numpy())
        rs.clear_cache()
        with pytest.raises(ValueError) as ei:
            search({"query_vectors": q.tolist(), "corpus_uri": bad, "corpus_dtype": "float16"})
        assert str(ei.value) == ms.F16_ERRORS[key] == "corpus values exceed the float16 range", value
        assert search({"query_vectors": q.tolist(), "corpus_uri": bad, "metric": "dot"})["ok"]  # fine as float32
    for value, dtype in ((np.inf, np.float32), (np.nan, np.float32), (np.inf, np.float16)):
        arr = c.numpy().astype(dtype) if dtype == np.float32 else _rows().numpy().astype(dtype)
        arr[20, 63] = value
        bad = _save(tmp_path, "nonfinite.npy", arr)
        rs.clear_cache()
        with pytest.raises(ValueError) as ei:
            search({"query_vectors": q.tolist(), "corpus_uri": bad, "corpus_dtype": "float16"})
        assert str(ei.value) == ms.ERRORS["corpus_nonfinite"]
    assert rs.cache_info()["entries"] == []  # a refused corpus is not kept


def test_loading_in_row_chunks_gives_the_same_rows_and_scales(search, tmp_path, monkeypatch):
    path = _save(tmp_path, "c32.npy", _rows().numpy())
    whole = rs.load_corpus(path, 2, 17, True, dtype="float16")
    rs.clear_cache()
    monkeypatch.setattr(rs, "CHUNK_BYTES", 5 * D * 4)  # 5 rows per chunk: 17 = 5 + 5 + 5 + 2
    parts = rs.load_corpus(path, 2, 17, True, dtype="float16")
    assert not parts.cached and parts.start == 2 and parts.total == N and parts.vectors.shape == (17, D)
    assert torch.equal(parts.vectors, whole.vectors) and torch.equal(parts.scale, whole.scale)


def test_size_limit_counts_resident_bytes(search, tmp_path, monkeypatch):
    from ops import map_search as ms

    path = _save(tmp_path, "c16.npy", _rows().half().numpy())
    job = {"query_vectors": _unit_queries().tolist(), "corpus_uri": path, "top_k": 2}
    monkeypatch.setenv("SEARCH_INDEX_MAX_GB", str((N * D * 2 + N * 4) / 2 ** 30))  # the cosine float16 slice exactly
    assert search(dict(job, corpus_dtype="float16"))["ok"]
    with pytest.raises(ValueError) as ei:
        search(dict(job))
    assert str(ei.value) == ms.ERRORS["corpus_too_large"]
    monkeypatch.setenv("SEARCH_INDEX_MAX_GB", str((N * D * 2 + N * 4 - 1) / 2 ** 30))
    rs.clear_cache()
    with pytest.raises(ValueError) as ei:
        search(dict(job, corpus_dtype="float16"))
    assert str(ei.value) == ms.F16_ERRORS["corpus_too_large_f16"] == "corpus slice exceeds SEARCH_INDEX_MAX_GB of float16"
    assert search(dict(job, corpus_dtype="float16", metric="dot"))["ok"]  # no scale: N * 4 bytes fewer


def test_lru_holds_both_dtypes_of_a_file_and_counts_real_bytes(search, tmp_path, monkeypatch):
    monkeypatch.setenv("SEARCH_INDEX_LRU_SIZE", "3")
    path = _save(tmp_path, "c16.npy", _rows().half().numpy())
    job = {"query_vectors": _unit_queries().tolist(), "corpus_uri": path, "top_k": 2}
    assert search(dict(job))["index_cached"] is False
    assert rs.cache_info()["resident_bytes"] == N * D * 4
    assert search(dict(job, corpus_dtype="float16"))["index_cached"] is False
    info = rs.cache_info()
    assert len(info["entries"]) == 2 and len(set(info["entries"])) == 1
    assert info["resident_bytes"] == N * D * 4 + N * D * 2 + N * 4
    assert search(dict(job))["index_cached"] is True and search(dict(job, corpus_dtype="float16"))["index_cached"] is True
    assert search(dict(job, corpus_dtype="float16", metric="dot"))["index_cached"] is False
    assert rs.cache_info()["resident_bytes"] == N * D * 4 + N * D * 2 + N * 4 + N * D * 2


def test_twin_row_scale_changes_the_ranking():
    q = torch.tensor([[1.0, 0.0]])
    c = torch.tensor([[3.0, 0.0], [2.0, 5.0], [1.0, 1.0]])
    assert ops.sim_topk_ref(q, c, 3)[1].tolist() == [[0, 1, 2]]
    s, i = ops.sim_topk_ref(q, c, 3, row_scale=torch.tensor([0.25, 1.0, 4.0]))
    assert i.tolist() == [[2, 1, 0]] and s.tolist() == [[4.0, 2.0, 0.75]]
    s, i = ops.sim_topk_ref(q, c.half(), 2, id_base=10, dtype=torch.float64, row_scale=torch.tensor([0.25, 1.0, 4.0]))
    assert i.tolist() == [[12, 11]] and s.dtype == torch.float64 and s.tolist() == [[4.0, 2.0]]
    # the wrapper's CPU path is the twin; its argument checks hold there too (D = 64: a kernel shape)
    q, c = torch.nn.functional.pad(q, (0, 62)), torch.nn.functional.pad(c, (0, 62))
    s, i = ops.sim_topk(q, c.half(), 3, row_scale=torch.tensor([0.25, 1.0, 4.0]))
    assert i.tolist() == [[2, 1, 0]] and s.dtype == torch.float32
    for bad in (lambda: ops.sim_topk(q, c, 3, row_scale=torch.ones(3)),
                lambda: ops.sim_topk(q, c.half(), 3, row_scale=torch.ones(2)),
                lambda: ops.sim_topk(q, c.half(), 3, row_scale=torch.ones(3).double()),
                lambda: ops.sim_topk(q, c.half(), 3, row_scale=torch.ones(6)[::2]),
                lambda: ops.sim_topk(q.half(), c.half(), 3),
                lambda: ops.sim_topk(q, c.bfloat16(), 3)):
        with pytest.raises(ValueError):
            bad()


def _corpus(tmp_path):
    path = str(tmp_path / "emb16.npy")
    res = registry.get_op("map_embed")({"texts": TEXTS, "model_path": MODEL, "output": "npy", "output_uri": path,
                                        "dtype": "float16"})
    assert res["ok"] and res["shape"] == [len(TEXTS), 256]
    return path


def test_lease_batch_keeps_the_dtypes_apart(search, tmp_path):
    path = _corpus(tmp_path)
    batch = registry.get_batch_op("map_search")
    payloads = [{"queries": TEXTS[:3], "corpus_uri": path, "model_path": MODEL, "top_k": 3, "corpus_dtype": "float16"},
                {"queries": TEXTS[:3], "corpus_uri": path, "model_path": MODEL, "top_k": 3},
                {"queries": TEXTS[3:], "corpus_uri": path, "model_path": MODEL, "top_k": 2, "corpus_dtype": "float16"},
                {"queries": TEXTS[:1], "corpus_uri": path, "model_path": MODEL, "corpus_dtype": "float64"}]
    res = batch([dict(p) for p in payloads])
    assert [r[0] for r in res] == ["ok", "ok", "ok", "err"]
    assert str(res[3][1]) == "payload.corpus_dtype must be 'float32' or 'float16'"
    assert res[0][1]["corpus_dtype"] == "float16" == res[2][1]["corpus_dtype"] and "corpus_dtype" not in res[1][1]
    for n in (0, 1, 2):
        one, got = search(dict(payloads[n])), res[n][1]
        assert set(one) == set(got), n
        for key in one:
            if key not in ("elapsed_ms", "queries_per_sec", "index_cached"):
                assert got[key] == one[key], (n, key)
    # cosine over unnormalised fp16 rows times the scale is not cosine over renormalised fp32 rows, bit for bit
    assert res[0][1]["ids"] == res[1][1]["ids"]
    assert np.allclose(res[0][1]["scores"], res[1][1]["scores"], atol=1e-5, rtol=0)


def test_corpus_texts_ignores_corpus_dtype(search):
    job = {"queries": TEXTS[2:4], "corpus_texts": TEXTS, "model_path": MODEL, "top_k": 4}
    plain, half = search(dict(job)), search(dict(job, corpus_dtype="float16"))
    assert "corpus_dtype" not in half and set(half) == set(plain)
    assert half["ids"] == plain["ids"] and half["scores"] == plain["scores"]
