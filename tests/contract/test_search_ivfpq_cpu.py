"""map_search ``index: {"type": "ivfpq"}`` on a CPU engine (the PyTorch twins of ``ops/pq_ivf.py``): result keys, errors,
the LRU entry, slices merged as the DP ranks merge them, and residual coding against flat PQ on a mixture corpus."""
import os

import numpy as np
import pytest
import torch

import ops as registry
from agent_tpu_amd import ops
from agent_tpu_amd.runtime import ivfpq
from agent_tpu_amd.runtime import search as rs

MODEL = "bert-tiny?batch=8&seq=32&seed=4"
IX = {"type": "ivfpq", "subvectors": 16, "clusters": 12, "train_rows": 512, "train_iterations": 5}


@pytest.fixture
def search(monkeypatch):
    monkeypatch.setenv("CLASSIFY_DEVICE", "cpu")
    for name in ("TASKS", "SEARCH_INDEX_DTYPE", "SEARCH_INDEX_MAX_GB"):
        monkeypatch.delenv(name, raising=False)
    monkeypatch.setenv("SEARCH_INDEX_LRU_SIZE", "8")  # no entry of a test is evicted
    rs.clear_cache()
    yield registry.get_op("map_search")
    rs.clear_cache()


@pytest.fixture(scope="module")
def data(tmp_path_factory):
    """A seeded mixture as bench/search.py's: 12 unit-norm centres, per-column noise 0.1, 1500 rows of 64 columns."""
    gen = torch.Generator().manual_seed(3)
    centres = rs.normalize_rows(torch.randn(12, 64, generator=gen))
    c = (centres[torch.randint(0, 12, (1500,), generator=gen)] + 0.1 * torch.randn(1500, 64, generator=gen)).contiguous()
    q = (c[::15] + 0.02 * torch.randn(100, 64, generator=gen)).contiguous()
    cpath = str(tmp_path_factory.mktemp("ivfpq") / "mixture.npy")
    np.save(cpath, c.numpy())
    return q, c, cpath


def test_result_keys_the_index_and_the_lru(search, data):
    q, c, cpath = data
    job = {"query_vectors": q[:4].tolist(), "corpus_uri": cpath, "top_k": 6}
    plain = search(dict(job))
    first = search(dict(job, index=dict(IX, nprobe=2)))
    assert list(first) == list(plain)[:-2] + ["index", "ids", "scores"]
    assert first["index"] == dict(IX, nprobe=2, converged=first["index"]["converged"], bytes_per_row=20)
    assert first["index_cached"] is False and all(len(r) == 6 for r in first["ids"])
    assert search(dict(job, index=dict(IX, nprobe=12)))["index_cached"] is True  # nprobe does not name the index
    assert search(dict(job, index=dict(IX, clusters=11)))["index_cached"] is False
    idx = ivfpq.load_index(cpath, 0, -1, torch.device("cpu"), 12, 16, 512, 5)
    assert idx.cached and idx.codes.shape == (1500, 16) and idx.offsets.tolist()[-1] == 1500
    labels = ops.kmeans_assign(rs.normalize_rows(c), idx.centroids)[0]
    assert torch.equal(ops.ivf_labels(idx.row_ids, idx.offsets), labels.long())
    ws, wi, _ = ops.sim_topk_ivfpq_ref(rs.normalize_rows(q[:4]), idx.codebooks, idx.codes, idx.row_ids, idx.offsets,
                                       idx.centroids, 6, 2)
    assert first["ids"] == wi.tolist() and first["scores"] == ws.tolist()
    dflt = search(dict(job, index={"type": "ivfpq", "subvectors": 8}))["index"]  # IVF's and PQ's defaults
    assert (dflt["clusters"], dflt["nprobe"], dflt["train_rows"], dflt["train_iterations"]) == (39, 8, 1500, 10)


def test_ivfpq_errors_are_fixed_and_listed_and_the_others_are_unchanged(search, data, monkeypatch, tmp_path):
    from ops import map_search as ms

    q, c, cpath = data
    contract = open(os.path.join(os.path.dirname(ms.__file__), "map_search.CONTRACT.md")).read()
    assert all(msg in contract for msg in ms.IVFPQ_ERRORS.values())
    assert ms.IVFPQ_ERRORS["ivfpq_too_large"] == ivfpq.ERRORS["ivfpq_too_large"]
    assert set(ms.IVF_ERRORS) == {"index", "index_corpus", "index_metric", "index_f16", "index_filter", "index_too_large"}
    assert set(ms.PQ_ERRORS) == {"compression", "compression_corpus", "compression_rows", "compression_filter",
                                 "compression_index", "compression_f16", "compression_too_large"}
    small, odd = str(tmp_path / "small.npy"), str(tmp_path / "odd.npy")
    np.save(small, c[:255].numpy())
    np.save(odd, c[:300, :32].numpy())
    job = {"query_vectors": q[:2].tolist(), "corpus_uri": cpath}
    ix = lambda **kw: {"index": dict(IX, **kw)}  # noqa: E731
    pqc = {"type": "pq", "subvectors": 16}
    cases = [("ivfpq", {"index": {"type": "ivfpq"}}), ("ivfpq", ix(subvectors=6)), ("ivfpq", ix(subvectors=32)),
             ("ivfpq", ix(bits=8)), ("ivfpq", ix(clusters=0)), ("ivfpq", ix(clusters=513)), ("ivfpq", ix(nprobe=13)),
             ("ivfpq", ix(nprobe=33, clusters=40)), ("ivfpq", ix(train_rows=255)), ("ivfpq", ix(train_rows=1501)),
             ("ivfpq", ix(train_iterations=0)), ("ivfpq", ix(subvectors=True)),
             ("ivfpq_metric", dict(ix(), metric="dot")), ("ivfpq_rows", dict(ix(), corpus_uri=small)),
             ("ivfpq_dim", dict(ix(subvectors=8), corpus_uri=odd, query_vectors=[[1.0] * 32])),
             ("ivfpq_filter", dict(ix(), filter={"ids": [1]})), ("ivfpq_compression", dict(ix(), compression=pqc)),
             ("ivfpq_f16", dict(ix(), corpus_dtype="float16"))]
    for key, extra in cases:
        with pytest.raises(ValueError) as ei:
            search(dict(job, **extra))
        assert str(ei.value) == ms.IVFPQ_ERRORS[key], (key, extra)
    with pytest.raises(ValueError) as ei:
        search(dict({"queries": ["a"], "corpus_texts": ["a", "b"], "model_path": MODEL}, **ix()))
    assert str(ei.value) == ms.IVFPQ_ERRORS["ivfpq_corpus"]
    # 1500 x (16 + 4) bytes: refused before any allocation when they do not fit
    monkeypatch.setenv("SEARCH_INDEX_MAX_GB", repr(29999 / 2 ** 30))
    with pytest.raises(ValueError) as ei:
        search(dict(job, **ix()))
    assert str(ei.value) == ms.IVFPQ_ERRORS["ivfpq_too_large"] and rs.cache_info()["entries"] == []
    monkeypatch.setenv("SEARCH_INDEX_MAX_GB", repr(30000 / 2 ** 30))  # far below the fp32 slice (384000 bytes)
    assert search(dict(job, **ix()))["ok"]
    assert {k for k, _ in cases} | {"ivfpq_corpus", "ivfpq_too_large"} == set(ms.IVFPQ_ERRORS)
    # today's refusals keep their messages
    for want, extra in ((ms.PQ_ERRORS["compression_index"], {"compression": pqc, "index": {"type": "ivf"}}),
                        (ms.IVF_ERRORS["index"], {"index": {"type": "pq"}}), (ms.IVF_ERRORS["index"], {"index": "ivfpq"})):
        with pytest.raises(ValueError) as ei:
            search(dict(job, **extra))
        assert str(ei.value) == want


def test_slices_cut_at_one_two_and_three_ranges_merge_to_the_same_result(search, data):
    """The DP argument without processes."""
    q, c, cpath = data
    qn = rs.normalize_rows(q[:9])
    whole = None
    for cuts in ([0, 1500], [0, 700, 1500], [0, 1, 801, 1500]):
        parts = []
        for lo, hi in zip(cuts[:-1], cuts[1:]):
            idx = ivfpq.load_index(cpath, lo, hi - lo, torch.device("cpu"), 12, 16, 512, 5)
            parts.append(ivfpq.search(qn, idx, 10, 3, id_base=lo)[:2])
        s, i = rs.merge_topk(torch.cat([p[0] for p in parts], 1), torch.cat([p[1] for p in parts], 1), 10)
        whole = whole or (s, i)
        assert torch.equal(i, whole[1]) and torch.equal(s.view(torch.int32), whole[0].view(torch.int32)), cuts


def test_residual_codes_recall_no_less_than_flat_pq(search, data):
    """recall@10 against the exact search, 100 queries, M = 16, train_rows 512, 5 iterations, nprobe = clusters:
    measured 0.712 for IVF-PQ and 0.600 for flat PQ."""
    q, c, cpath = data
    job = {"query_vectors": q.tolist(), "corpus_uri": cpath, "top_k": 10}
    exact = search(dict(job))["ids"]
    flat = search(dict(job, compression={"type": "pq", "subvectors": 16, "train_rows": 512, "train_iterations": 5}))["ids"]
    ours = search(dict(job, index=dict(IX, nprobe=12)))["ids"]
    recall = lambda got: sum(len(set(a) & set(b)) for a, b in zip(got, exact)) / (10 * len(exact))  # noqa: E731
    print("recall@10: ivfpq", recall(ours), "flat pq", recall(flat))
    assert recall(ours) >= recall(flat)
