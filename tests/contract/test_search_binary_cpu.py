"""map_search with ``compression: {"type": "binary"}`` on a CPU engine. The reference is independent of the twins:
bits by a float64 comparison, the +-1 product in float64, the stable descending sort of rows in ascending id. The
refined search equals the uncompressed one on a seeded mixture (unit centres, noise 0.05 per column, rows normalised,
queries that are noisy corpus rows) whose exact top-k lies inside the Hamming shortlist: asserted first."""
import os

import numpy as np
import pytest
import torch

import ops as registry
from agent_tpu_amd import ops
from agent_tpu_amd.runtime import binary as rb
from agent_tpu_amd.runtime import search as rs
from ops import map_search as ms

MODEL = "bert-tiny?batch=8&seq=32&seed=4"
BIN = {"type": "binary"}
RECIPES = [(2048, 128, 32, 10, 512), (4096, 64, 64, 5, 256)]  # N, D, centres, k, R


def mixture(N, D, centres, seed=1):
    gen = torch.Generator().manual_seed(seed)
    cen = torch.nn.functional.normalize(torch.randn(centres, D, generator=gen), dim=1)
    x = cen[torch.randint(0, centres, (N,), generator=gen)] + 0.05 * torch.randn(N, D, generator=gen)
    x = torch.nn.functional.normalize(x, dim=1)
    q = x[torch.randperm(N, generator=gen)[:16]] + 0.05 * torch.randn(16, D, generator=gen)
    return q.contiguous(), x.contiguous()


def hamming_scores(q, x, thr):
    pm = lambda v: (v.double() > thr.double()).double() * 2 - 1  # noqa: E731
    return pm(q) @ pm(x).T


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
    out = {}
    for N, D, centres, _, _ in RECIPES:
        q, x = mixture(N, D, centres)
        path = str(tmp_path_factory.mktemp("binary") / f"mix{D}.npy")
        np.save(path, x.numpy())
        out[D] = (q, x, path)
    return out


@pytest.mark.parametrize("metric", ["cosine", "dot"])
@pytest.mark.parametrize("threshold", ["zero", "mean"])
def test_plain_result_is_the_hamming_order_and_has_the_compression_key(search, data, threshold, metric):
    q, x, path = data[128]
    job = {"query_vectors": q.tolist(), "corpus_uri": path, "top_k": 10, "metric": metric}
    plain = search(dict(job))
    res = search(dict(job, compression=dict(BIN, threshold=threshold)))
    assert list(res) == list(plain)[:-2] + ["compression", "ids", "scores"]
    assert res["compression"] == {"type": "binary", "threshold": threshold, "bits": 128, "bytes_per_row": 16}
    qn = rs.normalize_rows(q) if metric == "cosine" else q  # the rows are unit already: their normalisation is a no-op
    rows = rs.normalize_rows(x) if metric == "cosine" else x
    thr = torch.zeros(128)
    if threshold == "mean":  # every row is in the sample (N <= 65536): the column mean, summed in fp64, rounded once
        thr = rows.double().sum(0).div(x.shape[0]).float()
    s = hamming_scores(qn, rows, thr)
    order = torch.sort(s, dim=1, descending=True, stable=True).indices[:, :10]
    assert res["ids"] == order.tolist() and res["scores"] == torch.gather(s, 1, order).tolist()
    assert (torch.gather(s, 1, order)[:, 1:] == torch.gather(s, 1, order)[:, :-1]).any()  # integer scores tie
    idx = rb.load_index(path, 0, -1, torch.device("cpu"), threshold, metric == "cosine")
    assert idx.cached and not res["index_cached"] and idx.codes.shape == (2048, 4) and torch.equal(idx.thr, thr)


@pytest.mark.parametrize("N,D,centres,k,R", RECIPES)
def test_refined_equals_the_uncompressed_search(search, data, N, D, centres, k, R):
    q, x, path = data[D]
    job = {"query_vectors": q.tolist(), "corpus_uri": path, "top_k": k}
    want = search(dict(job))
    # containment first, with the test's own reference: per segment the Hamming top-32 in the total order
    s = hamming_scores(rs.normalize_rows(q), x, torch.zeros(D))
    seg = ops.segment_rows(N, R // 32)
    short = [set() for _ in range(16)]
    for lo in range(0, N, seg):
        order = torch.sort(s[:, lo:lo + seg], dim=1, descending=True, stable=True).indices[:, :32] + lo
        for a in range(16):
            short[a] |= set(order[a].tolist())
    assert all(set(ids) <= short[a] and len(short[a]) == R for a, ids in enumerate(want["ids"]))
    res = search(dict(job, compression=BIN, refine={"candidates": R, "vectors": "float32"}))
    assert res["refine"] == {"candidates": R, "vectors": "float32", "store": "host", "rescored_rows": R}
    assert res["compression"]["bytes_per_row"] == D // 8
    assert res["ids"] == want["ids"] and res["scores"] == want["scores"]  # bit for bit
    plain = search(dict(job, compression=BIN))
    assert plain["ids"] != want["ids"] and "refine" not in plain


CASES = [
    ("binary", {"compression": dict(BIN, subvectors=8)}), ("binary", {"compression": dict(BIN, threshold="median")}),
    ("binary", {"compression": dict(BIN, threshold=0)}),
    ("binary", {"compression": dict(BIN, bits=1), "filter": {"ids": [1]}}),  # malformed comes first
    ("binary_corpus", {"compression": BIN, "corpus_uri": None}),
    ("binary_f16", {"compression": BIN, "corpus_dtype": "float16"}),
    ("binary_filter", {"compression": BIN, "filter": {"ids": [1]}}),
    ("binary_index", {"compression": BIN, "index": {"type": "ivf"}}),
    ("binary_dim", {"compression": BIN, "dim": 96}),
    ("binary_too_large", {"compression": BIN, "max_gb": 2047 * 16 / 2 ** 30}),
]


@pytest.mark.parametrize("key,extra", CASES)
def test_binary_errors(search, data, tmp_path, monkeypatch, key, extra):
    q, x, path = data[128]
    extra = dict(extra)
    dim = extra.pop("dim", 128)
    if dim != 128:
        path = str(tmp_path / "odd.npy")
        np.save(path, x[:300, :dim].numpy())
    if "max_gb" in extra:
        monkeypatch.setenv("SEARCH_INDEX_MAX_GB", str(extra.pop("max_gb")))
    job = dict({"query_vectors": q[:2, :dim].tolist(), "corpus_uri": path}, **extra)
    if job["corpus_uri"] is None:
        job = dict(job, corpus_texts=["a"], queries=["b"])
        del job["corpus_uri"], job["query_vectors"]
    with pytest.raises(ValueError) as e:
        search(job)
    assert str(e.value) == ms.BINARY_ERRORS[key] and not rs.cache_info()["entries"]


def test_the_contract_lists_the_errors_and_other_types_stay_pq_errors(search, data):
    q, x, path = data[128]
    contract = open(os.path.join(os.path.dirname(ms.__file__), "map_search.CONTRACT.md")).read()
    for msg in ms.BINARY_ERRORS.values():
        assert msg in contract, msg
    assert set(ms.BINARY_ERRORS) == {k for k, _ in CASES}
    assert ms.BINARY_ERRORS["binary_too_large"] == rb.ERRORS["binary_too_large"]
    for cp in ({"type": "bits"}, {"type": ["binary"]}, {"threshold": "zero"}, "binary"):
        with pytest.raises(ValueError) as e:
            search({"query_vectors": q[:2].tolist(), "corpus_uri": path, "compression": cp})
        assert str(e.value) == ms.PQ_ERRORS["compression"]


def test_batch_handler_keeps_binary_and_pq_jobs_apart(search, tmp_path):
    from agent_tpu_amd.models.bert import config_for

    texts = ["the quick brown fox", "jumps over, the lazy dog!", "x", "seven rows in all", "nearest neighbours"]
    H = config_for("bert-tiny").hidden
    path = str(tmp_path / "corpus.npy")
    np.save(path, torch.randn(300, H, generator=torch.Generator().manual_seed(8)).numpy())
    job = {"corpus_uri": path, "model_path": MODEL}
    pq = {"type": "pq", "subvectors": H // 8, "train_rows": 256, "train_iterations": 2}
    payloads = [dict(job, queries=texts[:2], top_k=2, compression=BIN),
                dict(job, queries=texts[2:4], top_k=7, compression={"threshold": "zero", "type": "binary"}),  # the same
                dict(job, queries=texts[4:], top_k=3, compression=dict(BIN, threshold="mean")),
                dict(job, queries=texts[:2], top_k=3, compression=BIN, refine={"candidates": 64}),
                dict(job, queries=texts[:2], top_k=3, compression=pq),
                dict(job, queries=texts[:2], top_k=3, compression=pq, refine={"candidates": 64})]
    calls, real_b, real_p = [], ms.search_queries_binary, ms.search_queries_pq
    ms.search_queries_binary = lambda *a, **kw: calls.append(("binary", a[5], a[8])) or real_b(*a, **kw)
    ms.search_queries_pq = lambda *a, **kw: calls.append(("pq", a[8])) or real_p(*a, **kw)
    try:
        res = registry.get_batch_op("map_search")([dict(p) for p in payloads])
    finally:
        ms.search_queries_binary, ms.search_queries_pq = real_b, real_p
    assert [r[0] for r in res] == ["ok"] * 6
    assert sorted(calls, key=str) == sorted([("binary", ("zero",), None), ("binary", ("mean",), None),
                                             ("binary", ("zero",), (64, "float16", "host")), ("pq", None),
                                             ("pq", (64, "float16", "host"))], key=str)  # jobs 0 and 1 share one search
    one = search(dict(payloads[1]))  # a job of a shared search keeps its single-job result
    assert res[1][1]["ids"] == one["ids"] and res[1][1]["scores"] == one["scores"] and len(one["ids"][0]) == 7
