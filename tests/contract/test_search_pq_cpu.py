"""map_search ``compression`` (product quantization) on a CPU engine: the PyTorch twins of ``ops/pq.py``, every
new error, the defaults, the result keys, the LRU entry, the lease-batch grouping, and two checks of what the
approximate scores mean, both with bounds that the test computes from the data.

**ADC consistency.** A returned score is ``sum_m lut[m][code_m]``, i.e. the products ``q_d * xhat_d`` of the query
and the row's reconstruction ``xhat = decode(codes)`` summed in fp32 in one association; ``dot(q, xhat)`` in fp64
sums the same products. An fp32 sum of ``D`` terms in any association is within ``(D - 1) u sum |terms|`` of the
exact one, and each fp32 product adds ``u |term|`` (``u = 2^-24``); the test allows ``2 D u sum |q_d * xhat_d|``.

**Quality.** ``|dot(q, x) - dot(q, xhat)| <= sum_m ||q_m|| ||x_m - xhat_m||`` (Cauchy-Schwarz per sub-space). If a
query's exact top-1 leads the runner-up by more than twice the largest such bound over the rows, the order of the
two cannot flip, so the PQ top-1 must be the exact top-1. The fixture (``_blobs``) is built so that at least 90 %
of its queries qualify: each sub-space has sixteen well-separated blobs, a row takes one blob per sub-space plus
small noise, so rows differ in most sub-spaces (large margins) and 256 codewords resolve every blob (small bounds).
"""
import os

import numpy as np
import pytest
import torch

import ops as registry
from agent_tpu_amd import ops
from agent_tpu_amd.runtime import pq
from agent_tpu_amd.runtime import search as rs

MODEL = "bert-tiny?batch=8&seq=32&seed=4"
U = 2.0 ** -24


def _blobs(N=600, D=64, M=16, seed=2, noise=0.02):
    gen = torch.Generator().manual_seed(seed)
    dsub = D // M
    proto = torch.randn(M, 16, dsub, generator=gen)
    proto = proto / proto.norm(dim=2, keepdim=True)  # sixteen unit blobs per sub-space
    pick = torch.randint(0, 16, (N, M), generator=gen)
    x = proto[torch.arange(M)[None, :], pick] + noise * torch.randn(N, M, dsub, generator=gen)
    return x.reshape(N, D).contiguous()


# ------------------------------------------------------------------------------------------- twins
def test_pq_ok_and_the_interleaved_layout():
    assert [ops.pq_ok(D, M) for D, M in ((64, 4), (64, 8), (64, 16), (768, 96), (768, 48), (1024, 128))] == [True] * 6
    assert [ops.pq_ok(D, M) for D, M in ((64, 2), (64, 32), (768, 192), (2048, 256), (66, 16), (24, 6), (64, 0))] == [False] * 7
    gen = torch.Generator().manual_seed(0)
    for N in (1, 63, 64, 65, 200):
        codes = torch.randint(0, 256, (N, 8), generator=gen).to(torch.uint8)
        pc = ops.pq_interleave(codes)
        assert pc.rows == N and pc.M == 8 and pc.data.shape == ((N + 63) // 64, 2, 64, 4)
        assert torch.equal(ops.pq_deinterleave(pc), codes)
        r, m = torch.arange(N)[:, None], torch.arange(8)[None, :]
        assert torch.equal(pc.data[r // 64, m // 4, r % 64, m % 4], codes)  # byte e of (b, m4, lane)
        assert int(pc.data.sum()) == int(codes.sum())  # the padding rows of the last block are zero


def test_encode_picks_the_nearest_codeword_lowest_id_on_ties():
    gen = torch.Generator().manual_seed(1)
    books = torch.randn(4, 256, 4, generator=gen)
    books[:, 9] = books[:, 4]  # duplicated codeword
    bias = ops.pq_bias(books)
    assert bias.dtype == torch.float32 and torch.allclose(bias.double(), -0.5 * (books.double() ** 2).sum(2), rtol=1e-7, atol=0)
    x = torch.randn(50, 16, generator=gen)
    x[0] = books[:, 9].reshape(-1)
    for fn in (ops.pq_encode, ops.pq_encode_ref):  # the wrapper's CPU path is the twin
        codes = fn(x, books, bias)
        assert codes.dtype == torch.uint8 and codes.shape == (50, 4) and codes[0].tolist() == [4] * 4
        d = ((x.view(50, 4, 1, 4) - books[None]) ** 2).sum(3)  # [50, 4, 256]
        assert torch.equal(torch.gather(d, 2, codes.long()[:, :, None])[:, :, 0], d.min(2).values)
    zero = ops.pq_encode(torch.zeros(3, 16), books, torch.zeros(4, 256))  # every score +-0.0: they tie, id 0
    assert zero.tolist() == [[0] * 4] * 3
    assert torch.equal(ops.pq_decode(codes, books)[0], x[0])


def test_scan_is_a_fixed_chain_whatever_the_batch_and_orders_ties_by_id():
    gen = torch.Generator().manual_seed(2)
    lut = torch.randint(-1, 1, (5, 8, 256), generator=gen).float()
    lut[:, :, 0] = -0.0
    codes = (torch.randint(0, 256, (100, 8), generator=gen) % 5).to(torch.uint8)
    codes[::9] = 0
    s, i = ops.pq_scan_topk(lut, codes, 32, 1000)
    assert s.shape == i.shape == (5, 32) and i[:, 0].tolist() == [1000] * 5
    assert (s[:, 0] == 0).all() and torch.signbit(s[:, 0]).all()  # -0.0 ties with +0.0: row 0 first
    assert (i[:, 1:] > i[:, :-1])[s[:, 1:] == s[:, :-1]].all()
    for a in range(5):
        s1, i1 = ops.pq_scan_topk(lut[a:a + 1].contiguous(), ops.pq_interleave(codes), 7, 1000, splits=3)
        assert torch.equal(i1[0], i[a, :7]) and torch.equal(s1[0], s[a, :7])
    s2, i2 = ops.pq_scan_topk(lut, codes[:3].contiguous(), 10)
    assert s2.shape == (5, 3)  # kk = min(k, N)
    want = torch.stack([sum(lut[a, m, codes[:, m].long()] for m in range(8)) for a in range(5)])
    assert torch.equal(torch.gather(want, 1, i - 1000), s)


def test_twin_rejections():
    gen = torch.Generator().manual_seed(3)
    books, x = torch.randn(4, 256, 4, generator=gen), torch.randn(9, 16, generator=gen)
    bias, lut = ops.pq_bias(books), ops.pq_lut(x, books)
    codes = ops.pq_encode(x, books, bias)
    ops.pq_scan_topk(lut, codes, 4)
    for bad in (lambda: ops.pq_encode(x, books[:, :255].contiguous(), bias), lambda: ops.pq_encode(x.double(), books, bias),
                lambda: ops.pq_encode(x, books, bias[:3]), lambda: ops.pq_lut(x[:, :12].contiguous(), books),
                lambda: ops.pq_lut(x, torch.randn(8, 256, 2)), lambda: ops.pq_scan_topk(lut, codes, 0),
                lambda: ops.pq_scan_topk(lut, codes, 33), lambda: ops.pq_scan_topk(lut, codes.int(), 4),
                lambda: ops.pq_scan_topk(lut, codes[:, :3].contiguous(), 4), lambda: ops.pq_scan_topk(lut, codes, 4, splits=257),
                lambda: ops.pq_scan_topk(lut, ops.PqCodes(ops.pq_interleave(codes).data, 200, 4), 4)):
        with pytest.raises(ValueError):
            bad()


# --------------------------------------------------------------------------------------------- op
@pytest.fixture
def search(monkeypatch):
    monkeypatch.setenv("CLASSIFY_DEVICE", "cpu")
    monkeypatch.delenv("TASKS", raising=False)
    monkeypatch.delenv("SEARCH_INDEX_DTYPE", raising=False)
    monkeypatch.delenv("SEARCH_INDEX_MAX_GB", raising=False)
    monkeypatch.setenv("SEARCH_INDEX_LRU_SIZE", "8")  # no entry of a test is evicted
    rs.clear_cache()
    yield registry.get_op("map_search")
    rs.clear_cache()


@pytest.fixture(scope="module")
def data(tmp_path_factory):
    c = _blobs()
    q = c[::6].contiguous()  # 100 queries that are corpus rows
    cpath = str(tmp_path_factory.mktemp("pq") / "blobs.npy")
    np.save(cpath, c.numpy())
    return q, c, cpath


def _pq(**kw):
    return {"compression": dict({"type": "pq", "subvectors": 16}, **kw)}


def test_defaults_result_keys_cache_entry_and_a_job_without_the_key(search, data):
    q, c, cpath = data
    job = {"query_vectors": q[:4].tolist(), "corpus_uri": cpath, "top_k": 6}
    plain = search(dict(job))
    assert list(plain) == ["ok", "op", "query_count", "corpus_rows", "dim", "top_k", "metric", "elapsed_ms",
                           "queries_per_sec", "index_cached", "ids", "scores"]  # today's keys
    ws, wi = ops.sim_topk_ref(rs.normalize_rows(q[:4]), rs.normalize_rows(c), 6)
    assert plain["ids"] == wi.tolist() and plain["scores"] == ws.tolist()  # and today's values
    rs.clear_cache()
    first = search(dict(job, **_pq()))
    assert list(first) == list(plain)[:-2] + ["compression", "ids", "scores"]
    assert first["compression"] == {"type": "pq", "subvectors": 16, "train_rows": 600, "train_iterations": 10,
                                    "bytes_per_row": 16}
    assert first["index_cached"] is False and first["corpus_rows"] == 600 and first["top_k"] == 6
    assert all(len(r) == 6 for r in first["ids"]) and [r[0] for r in first["ids"]] == [0, 6, 12, 18]
    # the entry: codes and codebooks, and nothing else: the fp32 slice was never loaded
    info = rs.cache_info()
    assert info["entries"] == [os.path.realpath(cpath)]
    assert info["resident_bytes"] == 600 * 16 + 16 * 256 * 4 * 4
    second = search(dict(job, **_pq()))
    assert second["index_cached"] is True and second["ids"] == first["ids"] and second["scores"] == first["scores"]
    assert rs.cache_info()["entries"] == [os.path.realpath(cpath)]
    # explicit values equal to the defaults are the same entry; other values are another
    assert search(dict(job, **_pq(train_rows=600, train_iterations=10)))["index_cached"] is True
    other = search(dict(job, **_pq(train_rows=300, train_iterations=2)))
    assert other["index_cached"] is False and other["compression"]["train_rows"] == 300
    assert search(dict(job, metric="dot", **_pq()))["index_cached"] is False  # not normalised: its own codes
    # the index itself: the sample is the seeded one, the codes are the encoder's over the final codebooks
    idx = pq.load_index(cpath, 0, -1, torch.device("cpu"), 16, 600, 10, True)
    assert idx.cached and idx.codes.shape == (600, 16) and idx.codebooks.shape == (16, 256, 4)
    x = rs.normalize_rows(c)
    assert torch.equal(idx.codes, ops.pq_encode_ref(x, idx.codebooks, ops.pq_bias(idx.codebooks)))
    assert torch.equal(pq.sample_rows(600, 300), torch.sort(torch.randperm(600, generator=torch.Generator().manual_seed(0))[:300]).values)
    assert torch.equal(pq.train(x[pq.sample_rows(600, 600)], 16, 10), idx.codebooks)
    ws, wi = ops.sim_topk_pq_ref(rs.normalize_rows(q[:4]), idx.codebooks, idx.codes, 6)
    assert first["ids"] == wi.tolist() and first["scores"] == ws.tolist()
    # min_score cuts after the search, top_k above the corpus is the corpus
    cut = search(dict(job, min_score=0.9, **_pq()))
    assert cut["ids"] == [[i for i, s in zip(r, sc) if s >= 0.9] for r, sc in zip(first["ids"], first["scores"])]
    assert [len(r) for r in cut["ids"]] == [1] * 4


def test_compression_errors_are_fixed_and_listed_in_the_contract(search, data, monkeypatch, tmp_path):
    from ops import map_search as ms

    q, c, cpath = data
    contract = open(os.path.join(os.path.dirname(ms.__file__), "map_search.CONTRACT.md")).read()
    for msg in ms.PQ_ERRORS.values():
        assert msg in contract, msg
    assert set(ms.PQ_ERRORS) == {"compression", "compression_corpus", "compression_rows", "compression_filter",
                                 "compression_index", "compression_f16", "compression_too_large"}
    assert ms.PQ_ERRORS["compression_too_large"] == pq.ERRORS["compression_too_large"]
    small = str(tmp_path / "small.npy")
    np.save(small, c[:255].numpy())
    job = {"query_vectors": q[:2].tolist(), "corpus_uri": cpath}
    cp = lambda **kw: {"compression": dict({"type": "pq", "subvectors": 16}, **kw)}  # noqa: E731
    cases = [
        ("compression", {"compression": None}), ("compression", {"compression": "pq"}), ("compression", {"compression": {}}),
        ("compression", {"compression": {"type": "pq"}}),  # subvectors is required
        ("compression", {"compression": {"type": "sq", "subvectors": 16}}), ("compression", cp(bits=8)),
        ("compression", cp(subvectors=0)), ("compression", cp(subvectors=6)), ("compression", cp(subvectors=132)),
        ("compression", cp(subvectors=16.0)), ("compression", cp(subvectors=True)),
        ("compression", cp(subvectors=32)), ("compression", cp(subvectors=64)),  # dsub 2 and 1 at dim 64
        ("compression", cp(train_rows=255)), ("compression", cp(train_rows=601)),  # more than the corpus
        ("compression", cp(train_rows=1048577)), ("compression", cp(train_rows="all")),
        ("compression", cp(train_iterations=0)), ("compression", cp(train_iterations=101)),
        ("compression", cp(train_iterations=None)),
        ("compression_rows", dict(cp(), corpus_uri=small)),
        ("compression_filter", dict(cp(), filter={"ids": [1]})),
        ("compression_index", dict(cp(), index={"type": "ivf"})),
        ("compression_f16", dict(cp(), corpus_dtype="float16")),
    ]
    seen = set()
    for key, extra in cases:
        with pytest.raises(ValueError) as ei:
            search(dict(job, **extra))
        assert str(ei.value) == ms.PQ_ERRORS[key], (key, extra)
        seen.add(key)
    with pytest.raises(ValueError) as ei:
        search(dict({"queries": ["a"], "corpus_texts": ["a", "b"], "model_path": MODEL}, **cp()))
    assert str(ei.value) == ms.PQ_ERRORS["compression_corpus"]
    # `index` keeps its own refusal of a type it does not know
    with pytest.raises(ValueError) as ei:
        search(dict(job, index={"type": "pq"}))
    assert str(ei.value) == ms.IVF_ERRORS["index"]
    # the environment's default dtype does not apply to codes; the result does not name it
    monkeypatch.setenv("SEARCH_INDEX_DTYPE", "float16")
    res = search(dict(job, **cp()))
    assert res["ok"] and "corpus_dtype" not in res
    monkeypatch.delenv("SEARCH_INDEX_DTYPE")
    # 600 x 16 bytes of codes: refused before any allocation when they do not fit
    rs.clear_cache()
    monkeypatch.setenv("SEARCH_INDEX_MAX_GB", repr(9599 / 2 ** 30))
    with pytest.raises(ValueError) as ei:
        search(dict(job, **cp()))
    assert str(ei.value) == ms.PQ_ERRORS["compression_too_large"] and rs.cache_info()["entries"] == []
    monkeypatch.setenv("SEARCH_INDEX_MAX_GB", repr(9600 / 2 ** 30))  # far below the fp32 slice (153600 bytes)
    assert search(dict(job, **cp()))["ok"]
    assert seen | {"compression_corpus", "compression_too_large"} == set(ms.PQ_ERRORS)
    # the other errors come first, as before; a non-finite corpus is refused with the loader's message
    with pytest.raises(ValueError) as ei:
        search(dict(job, top_k=0, compression="x"))
    assert str(ei.value) == ms.ERRORS["top_k"]
    monkeypatch.delenv("SEARCH_INDEX_MAX_GB")
    bad = c.clone()
    bad[599, 3] = float("nan")  # found in the training sample or, when the row is not in it, while encoding
    badpath = str(tmp_path / "bad.npy")
    np.save(badpath, bad.numpy())
    with pytest.raises(ValueError) as ei:
        search(dict(job, corpus_uri=badpath, **cp(train_rows=256)))
    assert str(ei.value) == ms.ERRORS["corpus_nonfinite"]
    with pytest.raises(ValueError) as ei:
        search(dict(job, query_vectors=[[1.0] * 32], **cp()))
    assert str(ei.value) == ms.ERRORS["dim"]


def test_adc_scores_are_the_dot_product_with_the_reconstruction(search, data):
    q, c, cpath = data
    for metric in ("cosine", "dot"):
        res = search({"query_vectors": q.tolist(), "corpus_uri": cpath, "top_k": 32, "metric": metric, **_pq()})
        idx = pq.load_index(cpath, 0, -1, torch.device("cpu"), 16, 600, 10, metric == "cosine")
        assert idx.cached
        xhat = ops.pq_decode(idx.codes, idx.codebooks).double()
        qn = (rs.normalize_rows(q) if metric == "cosine" else q).double()
        worst = 0.0
        for a in range(q.shape[0]):
            rows = torch.tensor(res["ids"][a])
            got = torch.tensor(res["scores"][a], dtype=torch.float64)
            terms = qn[a][None, :] * xhat[rows]
            bound = 2 * 64 * U * terms.abs().sum(1)
            err = (got - terms.sum(1)).abs()
            worst = max(worst, float((err / bound).max()))
            assert (err <= bound).all(), (metric, a)
        print(f"adc consistency ({metric}): worst error / bound = {worst:.3f}")


def test_pq_top1_is_the_exact_top1_wherever_the_margin_exceeds_the_reconstruction_bound(search, data):
    q, c, cpath = data
    exact = search({"query_vectors": q.tolist(), "corpus_uri": cpath, "top_k": 2})
    res = search({"query_vectors": q.tolist(), "corpus_uri": cpath, "top_k": 2, **_pq()})
    idx = pq.load_index(cpath, 0, -1, torch.device("cpu"), 16, 600, 10, True)
    x = rs.normalize_rows(c).double()
    qn = rs.normalize_rows(q).double()
    err = (x - ops.pq_decode(idx.codes, idx.codebooks).double()).view(600, 16, 4).norm(dim=2)  # [rows, M]
    qualify = 0
    for a in range(q.shape[0]):
        bound = float((qn[a].view(16, 4).norm(dim=1)[None, :] * err).sum(1).max())  # the largest over the rows
        margin = exact["scores"][a][0] - exact["scores"][a][1]
        if margin > 2 * bound:
            qualify += 1
            assert res["ids"][a][0] == exact["ids"][a][0], (a, margin, bound)
    print(f"quality: {qualify} of {q.shape[0]} queries qualify")
    assert qualify >= 0.9 * q.shape[0]
    assert [r[0] for r in exact["ids"]] == list(range(0, 600, 6))  # a query is a corpus row: itself


def test_batch_handler_groups_by_the_canonical_compression(search, tmp_path):
    """``queries`` jobs (a model embeds them) over a 300-row corpus of the model's dim: batched results equal the
    job-by-job ones, jobs with equal canonical compression share one search."""
    from agent_tpu_amd.models.bert import config_for
    from ops import map_search as ms

    texts = ["the quick brown fox", "jumps over, the lazy dog!", "MI355X " * 30, "x", "seven rows in all",
             "an index of sentence vectors", "nearest neighbours by cosine"]
    H = config_for("bert-tiny").hidden
    path = str(tmp_path / "corpus.npy")
    np.save(path, torch.randn(300, H, generator=torch.Generator().manual_seed(8)).numpy())
    batch = registry.get_batch_op("map_search")
    job = {"corpus_uri": path, "model_path": MODEL}
    cp = lambda **kw: dict({"type": "pq", "subvectors": H // 8, "train_rows": 256, "train_iterations": 2}, **kw)  # noqa: E731
    payloads = [
        dict(job, queries=texts[:3], top_k=2, compression=cp()),
        dict(job, queries=texts[3:5], top_k=7, compression=dict(reversed(list(cp().items())))),  # written differently
        dict(job, queries=texts[5:], top_k=3, compression=cp(train_iterations=3)),
        dict(job, queries=texts[:2], top_k=3, compression=cp(subvectors=H // 16)),
        dict(job, queries=texts[:2], top_k=3),
        dict(job, queries=texts[:2], top_k=3, compression=cp(train_rows=301)),
        dict(job, queries=texts[:2], top_k=3, compression=cp(), filter={"ids": [1]}),
    ]
    calls = []
    real = ms.search_queries_pq

    def counting(*a, **kw):
        calls.append(a[5])
        return real(*a, **kw)

    ms.search_queries_pq = counting
    try:
        res = batch([dict(p) for p in payloads])
    finally:
        ms.search_queries_pq = real
    assert [r[0] for r in res] == ["ok"] * 5 + ["err", "err"]
    assert str(res[5][1]) == ms.PQ_ERRORS["compression"] and str(res[6][1]) == ms.PQ_ERRORS["compression_filter"]
    assert sorted(calls) == sorted([(H // 8, 256, 2), (H // 8, 256, 3), (H // 16, 256, 2), (H // 8, 301, 2)])  # 0 and 1 share
    for n in range(5):
        one, got = search(dict(payloads[n])), res[n][1]
        assert set(one) == set(got), n
        for key in one:
            if key not in ("elapsed_ms", "queries_per_sec", "index_cached"):
                assert got[key] == one[key], (n, key)
    assert res[2][1]["compression"]["train_iterations"] == 3 and "compression" not in res[4][1]
    assert res[0][1]["compression"]["bytes_per_row"] == H // 8
