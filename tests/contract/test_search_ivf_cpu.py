"""map_search ``index`` (IVF) on a CPU engine: the ``sim_topk_ivf`` twin against the masked ``sim_topk`` twin
query by query, the plan's work items, every new error, the defaults, the result keys, the LRU entry and the
lease-batch grouping key.

Every comparison is exact. The twin tests use small-integer data with duplicated rows (ties occur) and
hand-made labels. The op tests need the cosine metric: their rows have sixteen entries of +-1, so a normalised
row is sixteen entries of +-0.25 and every dot product is an exact multiple of 1/16 in any summation order.
"""
import os

import numpy as np
import pytest
import torch

import ops as registry
from agent_tpu_amd import ops
from agent_tpu_amd.runtime import ivf
from agent_tpu_amd.runtime import search as rs

MODEL = "bert-tiny?batch=8&seq=32&seed=4"
PAD_ID = 2 ** 62
NEG = float("-inf")


def _ints(seed=3, N=101, nq=6, D=64):
    gen = torch.Generator().manual_seed(seed)
    c = torch.randint(-2, 3, (N, D), generator=gen).float()
    c[7], c[40], c[N - 1] = c[3], c[3], c[3]  # ties
    q = torch.randint(-2, 3, (nq, D), generator=gen).float()
    q[0] = c[3]
    return q, c


def _index(c, labels, K):
    """(vectors, row_ids, offsets) of hand-made labels: the stable sort the builder does."""
    order = torch.sort(labels, stable=True).indices
    offsets = torch.zeros(K + 1, dtype=torch.int32)
    offsets[1:] = torch.cumsum(torch.bincount(labels, minlength=K), 0).to(torch.int32)
    return c[order].contiguous(), order.to(torch.int32), offsets


def _case(K=7, seed=3, N=101, nq=6):
    q, c = _ints(seed, N, nq)
    gen = torch.Generator().manual_seed(seed + 100)
    labels = torch.randint(0, K - 1, (N,), generator=gen)  # cluster K - 1 stays empty
    labels[3], labels[7], labels[40], labels[N - 1] = 0, 0, 2, 2  # the tied rows: two clusters
    cent = torch.randint(-2, 3, (K, 64), generator=gen).float()
    return q, c, labels, cent, _index(c, labels, K)


def _sign_rows(n, D, gen):
    """Rows of sixteen +-1 entries: normalised, sixteen +-0.25, exactly."""
    x = torch.zeros(n, D)
    for r in range(n):
        pos = torch.randperm(D, generator=gen)[:16]
        x[r, pos] = torch.randint(0, 2, (16,), generator=gen).float() * 2 - 1
    return x


# ------------------------------------------------------------------------------------------- twins
def test_twin_equals_the_masked_twin_query_by_query():
    K = 7
    q, c, labels, cent, (vec, rid, off) = _case(K)
    assert torch.equal(ops.ivf_labels(rid, off), labels)
    for nprobe in (1, 3, K):
        probes = ops.sim_topk_ref(q, cent, nprobe)[1]
        for k in (1, 8, 32):
            for fn in (ops.sim_topk_ivf_ref, ops.sim_topk_ivf):  # the wrapper's CPU path is the twin
                s, i, n = fn(q, vec, rid, off, cent, k, nprobe, 1000)
                assert s.shape == i.shape == (q.shape[0], k) and s.dtype == torch.float32 and i.dtype == torch.int64
                for a in range(q.shape[0]):
                    bits = torch.isin(labels, probes[a])
                    ws, wi = ops.sim_topk_ref(q[a:a + 1], c, k, 1000, mask=ops.row_mask_from_bits(bits))
                    m = int(n[a])
                    assert m == min(k, int(bits.sum())) == ws.shape[1]
                    assert torch.equal(s[a, :m], ws[0]) and torch.equal(i[a, :m], wi[0]), (nprobe, k, a)
                    assert (s[a, m:] == NEG).all() and (i[a, m:] == PAD_ID).all()


def test_probing_every_cluster_is_the_exact_search():
    K = 7
    q, c, labels, cent, (vec, rid, off) = _case(K)
    for k in (1, 10, 32):
        s, i, n = ops.sim_topk_ivf_ref(q, vec, rid, off, cent, k, K, 5)
        ws, wi = ops.sim_topk_ref(q, c, k, 5)
        assert torch.equal(s, ws) and torch.equal(i, wi) and n.tolist() == [k] * q.shape[0]
    assert i[0, :4].tolist() == [8, 12, 45, 105]  # the four copies of q[0]'s row tie: ascending original id


def test_a_query_alone_equals_the_query_in_a_batch_and_short_lists_are_padded():
    K = 7
    q, c, labels, cent, (vec, rid, off) = _case(K, nq=40)
    s, i, n = ops.sim_topk_ivf_ref(q, vec, rid, off, cent, 32, 1)
    assert (n < 32).any()  # some clusters hold fewer than 32 rows
    for a in (0, 1, 17, 39):
        s1, i1, n1 = ops.sim_topk_ivf_ref(q[a:a + 1].contiguous(), vec, rid, off, cent, 32, 1)
        assert torch.equal(s1[0], s[a]) and torch.equal(i1[0], i[a]) and int(n1[0]) == int(n[a])
    # a query whose only probed cluster is empty: all padding, count 0
    cent2 = cent.clone()
    cent2[K - 1] = q[5] * 100
    s2, i2, n2 = ops.sim_topk_ivf_ref(q[5:6].contiguous(), vec, rid, off, cent2, 4, 1)
    assert int(n2[0]) == 0 and (s2 == NEG).all() and (i2 == PAD_ID).all()
    # an empty slice (a DP rank beyond the corpus): the same
    s3, i3, n3 = ops.sim_topk_ivf(q, vec[:0], rid[:0], torch.zeros(K + 1, dtype=torch.int32), cent, 4, 2)
    assert s3.shape == (40, 4) and (i3 == PAD_ID).all() and n3.tolist() == [0] * 40


def test_a_nan_outside_the_probed_clusters_cannot_leak():
    K = 7
    q, c, labels, cent, (vec, rid, off) = _case(K)
    q = q[:2].contiguous()  # four probe slots over six non-empty clusters: some cluster is not probed
    probes = ops.sim_topk_ref(q, cent, 2)[1]
    clean = ops.sim_topk_ivf_ref(q, vec, rid, off, cent, 8, 2)
    unprobed = sorted(set(range(K - 1)) - set(probes.flatten().tolist()))
    assert unprobed
    v2 = vec.clone()
    v2[int(off[unprobed[0]]):int(off[unprobed[0] + 1])] = float("nan")
    got = ops.sim_topk_ivf_ref(q, v2, rid, off, cent, 8, 2)
    assert all(torch.equal(a, b) for a, b in zip(got, clean)) and torch.isfinite(got[0][got[1] != PAD_ID]).all()


@pytest.mark.parametrize("nq,nprobe,K", [(1, 1, 1), (1, 3, 7), (17, 3, 7), (40, 7, 7), (40, 1, 7), (100, 2, 3)])
def test_plan_puts_every_pair_into_exactly_one_item_of_one_cluster(nq, nprobe, K):
    gen = torch.Generator().manual_seed(nq + nprobe)
    probes = torch.stack([torch.randperm(K, generator=gen)[:nprobe] for _ in range(nq)])
    if nq == 40 and nprobe == 1:
        probes[:] = 4  # forty queries of one cluster: three items
    bound = min(nq * nprobe, K) + nq * nprobe // 16
    cl, iq, sl = ops.ivf_plan(probes, K, bound)
    assert cl.shape == (bound,) and iq.shape == sl.shape == (bound, 16) and cl.dtype == iq.dtype == sl.dtype == torch.int32
    seen = set()
    for it in range(bound):
        slots = [(int(a), int(b)) for a, b in zip(iq[it], sl[it]) if b >= 0]
        if cl[it] < 0:
            assert not slots
            continue
        assert slots and int(sl[it, 0]) >= 0
        for a, b in slots:
            assert int(probes[a, b]) == int(cl[it]) and (a, b) not in seen
            seen.add((a, b))
        assert all(0 <= int(a) < nq for a in iq[it])  # padding repeats a valid query
    assert len(seen) == nq * nprobe
    if nq == 40 and nprobe == 1:
        assert (cl >= 0).sum() == 3


def test_twin_rejections():
    K = 7
    q, c, labels, cent, (vec, rid, off) = _case(K)
    ops.sim_topk_ivf(q, vec, rid, off, cent, 4, 2)
    for bad in (lambda: ops.sim_topk_ivf(q, vec, rid, off, cent, 4, 0), lambda: ops.sim_topk_ivf(q, vec, rid, off, cent, 4, K + 1),
                lambda: ops.sim_topk_ivf(q, vec, rid, off, cent, 33, 1), lambda: ops.sim_topk_ivf(q, vec, rid.long(), off, cent, 4, 1),
                lambda: ops.sim_topk_ivf(q, vec, rid, off[:-1], cent, 4, 1), lambda: ops.sim_topk_ivf(q, vec.half(), rid, off, cent, 4, 1),
                lambda: ops.sim_topk_ivf(q, vec, rid[:-1], off, cent, 4, 1), lambda: ops.sim_topk_ivf(q, vec, rid, off, cent, 4, 2, splits=129)):
        with pytest.raises(ValueError):
            bad()


# --------------------------------------------------------------------------------------------- op
@pytest.fixture
def search(monkeypatch):
    monkeypatch.setenv("CLASSIFY_DEVICE", "cpu")
    monkeypatch.delenv("TASKS", raising=False)
    monkeypatch.delenv("SEARCH_INDEX_DTYPE", raising=False)
    rs.clear_cache()
    yield registry.get_op("map_search")
    rs.clear_cache()


@pytest.fixture
def data(tmp_path):
    gen = torch.Generator().manual_seed(11)
    c = _sign_rows(101, 64, gen)
    c[7], c[40], c[100] = c[3], c[3], c[3]  # ties
    q = _sign_rows(6, 64, gen)
    q[0] = c[3]
    cpath = str(tmp_path / "signs.npy")
    np.save(cpath, c.numpy())
    return q, c, cpath


def test_probing_every_cluster_equals_the_job_without_an_index(search, data):
    q, c, cpath = data
    job = {"query_vectors": q.tolist(), "corpus_uri": cpath, "top_k": 6}
    plain = search(dict(job))
    assert list(plain) == ["ok", "op", "query_count", "corpus_rows", "dim", "top_k", "metric", "elapsed_ms",
                           "queries_per_sec", "index_cached", "ids", "scores"]  # a job without an index keeps its keys
    assert plain["ids"][0][:4] == [3, 7, 40, 100] and plain["scores"][0][:4] == [1.0] * 4
    full = search(dict(job, index={"type": "ivf", "clusters": 5, "nprobe": 5, "train_iterations": 4}))
    assert full["ids"] == plain["ids"] and full["scores"] == plain["scores"]
    assert list(full) == list(plain)[:-2] + ["index", "ids", "scores"]
    assert full["index_cached"] is False and set(full["index"]) == {"type", "clusters", "nprobe", "train_iterations",
                                                                    "converged"}
    assert full["index"]["type"] == "ivf" and full["index"]["clusters"] == 5 and full["index"]["nprobe"] == 5
    assert 1 <= full["index"]["train_iterations"] <= 4 and isinstance(full["index"]["converged"], bool)


def test_probed_lists_equal_the_masked_twin_over_the_index_labels_and_the_entry_is_cached(search, data):
    q, c, cpath = data
    job = {"query_vectors": q.tolist(), "corpus_uri": cpath, "top_k": 32,
           "index": {"type": "ivf", "clusters": 9, "nprobe": 2, "train_iterations": 3}}
    first = search(dict(job))
    second = search(dict(job))
    assert first["index_cached"] is False and second["index_cached"] is True
    assert second["ids"] == first["ids"] and second["scores"] == first["scores"] and second["index"] == first["index"]
    idx = ivf.load_index(cpath, 0, -1, torch.device("cpu"), 9, 3)
    assert idx.cached and idx.offsets.tolist()[0] == 0 and idx.offsets.tolist()[-1] == 101
    assert idx.row_ids.dtype == torch.int32 and sorted(idx.row_ids.tolist()) == list(range(101))
    labels = ops.ivf_labels(idx.row_ids, idx.offsets)
    x = rs.normalize_rows(c)
    assert torch.equal(ivf.original_rows(idx), x)
    assert torch.equal(labels, ops.kmeans_assign(x, idx.centroids)[0].long())  # the arg-max over the final centroids
    for a in range(1, 101):  # ascending original row inside a cluster
        assert labels[idx.row_ids[a]] > labels[idx.row_ids[a - 1]] or idx.row_ids[a] > idx.row_ids[a - 1]
    qn = rs.normalize_rows(q)
    probes = ops.sim_topk_ref(qn, idx.centroids, 2)[1]
    ragged = False
    for a in range(6):
        bits = torch.isin(labels, probes[a])
        ws, wi = ops.sim_topk_ref(qn[a:a + 1], x, 32, mask=ops.row_mask_from_bits(bits))
        assert first["ids"][a] == wi[0].tolist() and first["scores"][a] == ws[0].tolist()
        ragged |= len(first["ids"][a]) < 32
    assert ragged  # two of nine clusters of 101 rows: fewer than top_k somewhere, and the list is shorter
    # the entry sits in the LRU next to the original-order slice, and its bytes are reported
    info = rs.cache_info()
    assert info["entries"] == [os.path.realpath(cpath)] * 2
    assert info["resident_bytes"] == 2 * 101 * 64 * 4 + 101 * 4 + 10 * 4 + 9 * 64 * 4
    # another (clusters, train_iterations) is another entry; another nprobe is not
    assert search(dict(job, index={"type": "ivf", "clusters": 9, "nprobe": 1, "train_iterations": 3}))["index_cached"] is True
    assert search(dict(job, index={"type": "ivf", "clusters": 9, "nprobe": 2, "train_iterations": 2}))["index_cached"] is False
    # min_score cuts after the search, as without an index
    cut = search(dict(job, min_score=0.5))
    assert cut["ids"] == [[i for i, s in zip(r, sc) if s >= 0.5] for r, sc in zip(first["ids"], first["scores"])]


def test_defaults(search, data):
    q, c, cpath = data
    res = search({"query_vectors": q.tolist(), "corpus_uri": cpath, "index": {"type": "ivf"}})
    assert res["index"]["clusters"] == 11 and res["index"]["nprobe"] == 8  # ceil(sqrt(101)), min(8, clusters)
    assert 1 <= res["index"]["train_iterations"] <= 10 and res["top_k"] == 10
    res = search({"query_vectors": q.tolist(), "corpus_uri": cpath, "index": {"type": "ivf", "clusters": 3}})
    assert res["index"]["clusters"] == 3 and res["index"]["nprobe"] == 3
    assert [ivf.default_clusters(n) for n in (1, 2, 4, 5, 101, 2 ** 20, 4096 ** 2, 4096 ** 2 + 1, 10 ** 9)] == \
        [1, 2, 2, 3, 11, 1024, 4096, 4096, 4096]


def test_index_errors_are_fixed_and_listed_in_the_contract(search, data, monkeypatch):
    from ops import map_search as ms

    q, c, cpath = data
    contract = open(os.path.join(os.path.dirname(ms.__file__), "map_search.CONTRACT.md")).read()
    for msg in ms.IVF_ERRORS.values():
        assert msg in contract, msg
    assert set(ms.IVF_ERRORS) == {"index", "index_corpus", "index_metric", "index_f16", "index_filter", "index_too_large"}
    assert ms.IVF_ERRORS["index_too_large"] == ivf.ERRORS["index_too_large"]
    job = {"query_vectors": q.tolist(), "corpus_uri": cpath}
    ix = lambda **kw: {"index": dict({"type": "ivf"}, **kw)}  # noqa: E731
    cases = [
        ("index", {"index": None}), ("index", {"index": "ivf"}), ("index", {"index": {}}), ("index", {"index": {"type": "pq"}}),
        ("index", ix(rows=3)), ("index", ix(clusters=0)), ("index", ix(clusters=4097)), ("index", ix(clusters=2.0)),
        ("index", ix(clusters=True)), ("index", ix(clusters=102)),  # more clusters than corpus rows
        ("index", ix(nprobe=0)), ("index", ix(nprobe=33)), ("index", ix(nprobe="8")), ("index", ix(clusters=4, nprobe=5)),
        ("index", ix(nprobe=12)),  # above the default clusters of this corpus, 11
        ("index", ix(train_iterations=0)), ("index", ix(train_iterations=101)), ("index", ix(train_iterations=None)),
        ("index_metric", dict(ix(), metric="dot")),
        ("index_f16", dict(ix(), corpus_dtype="float16")),
        ("index_filter", dict(ix(), filter={"ids": [1]})),
    ]
    seen = set()
    for key, extra in cases:
        with pytest.raises(ValueError) as ei:
            search(dict(job, **extra))
        assert str(ei.value) == ms.IVF_ERRORS[key], (key, extra)
        seen.add(key)
    with pytest.raises(ValueError) as ei:
        search(dict({"queries": ["a"], "corpus_texts": ["a", "b"], "model_path": MODEL}, **ix()))
    assert str(ei.value) == ms.IVF_ERRORS["index_corpus"]
    monkeypatch.setenv("SEARCH_INDEX_DTYPE", "float16")
    with pytest.raises(ValueError) as ei:
        search(dict(job, **ix()))
    assert str(ei.value) == ms.IVF_ERRORS["index_f16"]
    assert search(dict(job, corpus_dtype="float32", **ix()))["ok"]  # the payload wins
    monkeypatch.delenv("SEARCH_INDEX_DTYPE")
    # one fp32 copy of the slice fits (25856 bytes), the build's two do not: refused before any allocation
    rs.clear_cache()
    monkeypatch.setenv("SEARCH_INDEX_MAX_GB", repr(40000 / 2 ** 30))
    assert search(dict(job))["ok"]
    rs.clear_cache()
    with pytest.raises(ValueError) as ei:
        search(dict(job, **ix()))
    assert str(ei.value) == ms.IVF_ERRORS["index_too_large"] and rs.cache_info()["entries"] == []
    assert seen | {"index_corpus", "index_too_large"} == set(ms.IVF_ERRORS)
    # the other errors come first, as before
    with pytest.raises(ValueError) as ei:
        search(dict(job, top_k=0, index="x"))
    assert str(ei.value) == ms.ERRORS["top_k"]


def test_batch_handler_groups_by_the_canonical_index(search, tmp_path):
    texts = ["the quick brown fox", "jumps over, the lazy dog!", "MI355X " * 30, "x", "seven rows in all",
             "an index of sentence vectors", "nearest neighbours by cosine", "a corpus row", "another corpus row",
             "the last one"]
    path = str(tmp_path / "corpus.npy")
    assert registry.get_op("map_embed")({"texts": texts, "model_path": MODEL, "output": "npy", "output_uri": path})["ok"]
    batch = registry.get_batch_op("map_search")
    job = {"corpus_uri": path, "model_path": MODEL}
    ix = lambda **kw: dict({"type": "ivf", "clusters": 3, "nprobe": 2, "train_iterations": 5}, **kw)  # noqa: E731
    payloads = [
        dict(job, queries=texts[:3], top_k=2, index=ix()),
        dict(job, queries=texts[3:5], top_k=7, index=dict(reversed(list(ix().items())))),  # the same index, written differently
        dict(job, queries=texts[5:7], top_k=3, index=ix(nprobe=3)),  # differs only in nprobe: its own group
        dict(job, queries=texts[7:], top_k=3, index=ix(clusters=4)),
        dict(job, queries=texts[:2], top_k=3, index=ix(train_iterations=6)),
        dict(job, queries=texts[:2], top_k=3),
        dict(job, queries=texts[:2], top_k=3, index=ix(nprobe=4)),
        dict(job, queries=texts[:2], top_k=3, index=ix(clusters=11)),
    ]
    calls = []
    from ops import map_search as ms

    real = ms.search_queries_ivf

    def counting(*a, **kw):
        calls.append(a[4])
        return real(*a, **kw)

    ms.search_queries_ivf = counting
    try:
        res = batch([dict(p) for p in payloads])
    finally:
        ms.search_queries_ivf = real
    assert [r[0] for r in res] == ["ok"] * 6 + ["err", "err"]
    assert str(res[6][1]) == str(res[7][1]) == ms.IVF_ERRORS["index"]
    assert sorted(calls) == sorted([(3, 2, 5), (3, 3, 5), (4, 2, 5), (3, 2, 6), (11, 2, 5)])  # jobs 0 and 1 share a search
    for n in range(6):
        one, got = search(dict(payloads[n])), res[n][1]
        assert set(one) == set(got), n
        for key in one:
            if key not in ("elapsed_ms", "queries_per_sec", "index_cached"):
                assert got[key] == one[key], (n, key)
    assert res[2][1]["index"]["nprobe"] == 3 and "index" not in res[5][1]
