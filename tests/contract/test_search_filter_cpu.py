"""map_search ``filter`` on a CPU engine: the masked sim_topk twin against a brute-force top-k over
the allowed rows, the mask twins, every new error, ``filter_rows`` with short and empty lists,
``min_score`` after the filter, unchanged results without a filter, the labels LRU and lease batching."""
import os

import numpy as np
import pytest
import torch

import ops as registry
from agent_tpu_amd import ops
from agent_tpu_amd.runtime import search as rs

MODEL = "bert-tiny?batch=8&seq=32&seed=4"


def _brute(q, c, k, allowed, id_base=0):
    """Brute force in fp64 over the allowed rows only: python sort on (-score, id)."""
    s = (q.double().unsqueeze(1) * c.double().unsqueeze(0)).sum(-1)
    ids, scores = [], []
    for row in s.tolist():
        order = sorted(allowed, key=lambda j: (-row[j], j))[:k]
        ids.append([id_base + j for j in order])
        scores.append([row[j] for j in order])
    return scores, ids


def _ints(seed=3, N=101, nq=6, D=64):
    gen = torch.Generator().manual_seed(seed)
    c = torch.randint(-2, 3, (N, D), generator=gen).float()
    c[7], c[40], c[N - 1] = c[3], c[3], c[3]  # ties
    q = torch.randint(-2, 3, (nq, D), generator=gen).float()
    q[0] = c[3]
    return q, c


def _np_words(bits):
    padded = np.zeros((len(bits) + 31) // 32 * 32, dtype=bool)
    padded[:len(bits)] = bits
    return np.packbits(padded, bitorder="little").view("<i4")


# ------------------------------------------------------------------------------------------- twins
def test_masked_twin_against_brute_force_over_the_allowed_rows():
    q, c = _ints()
    N = c.shape[0]
    allowed = [3, 7, 40, N - 1, 0, 5, 64, 65, 96]
    for rows in (allowed, list(range(0, N, 2)), [N - 1], [0], allowed[:3]):
        mask = ops.row_mask_from_ids(rows, N)
        assert mask.count == len(set(rows)) and mask.rows == N
        for k in (1, 4, 10, 32):
            ws, wi = _brute(q, c, k, sorted(set(rows)), 1000)
            for fn in (ops.sim_topk_ref, ops.sim_topk):  # the wrapper's CPU path is the twin
                s, i = fn(q, c, k, 1000, mask=mask)
                assert s.shape == i.shape == (q.shape[0], min(k, len(set(rows))))
                assert i.tolist() == wi and s.double().tolist() == ws  # integer data: exact, tie order included
    s, i = ops.sim_topk_ref(q, c, 10, mask=ops.row_mask_from_ids(allowed, N))
    assert i[0, :4].tolist() == [3, 7, 40, N - 1] and len(set(s[0, :4].tolist())) == 1  # the tied rows, ascending
    # a mask equals the search of the gathered rows, ids mapped back
    R = torch.tensor(sorted(allowed))
    s2, i2 = ops.sim_topk_ref(q, c[R].contiguous(), 10)
    assert torch.equal(s, s2) and torch.equal(i, R[i2])
    # nothing allowed: [nq, 0]; NaN in a masked row cannot leak
    s0, i0 = ops.sim_topk(q, c, 5, mask=ops.row_mask_from_ids([], N))
    assert s0.shape == i0.shape == (q.shape[0], 0) and s0.dtype == torch.float32 and i0.dtype == torch.int64
    c2 = c.clone()
    c2[1] = float("nan")
    s3, i3 = ops.sim_topk_ref(q, c2, 10, mask=ops.row_mask_from_ids(allowed, N))
    assert torch.equal(s3, s) and torch.equal(i3, i)
    # without a mask the twin is what it was
    assert ops.sim_topk_ref(q, c, 10)[0].shape == (q.shape[0], 10)


def test_mask_twins_against_packbits():
    for N in (1, 31, 32, 33, 63, 64, 65, 101):
        rng = np.random.default_rng(N)
        base = 50
        inside = rng.integers(base, base + N, size=max(1, N // 3))
        ids = np.concatenate([inside, inside, [0, base - 1, base + N, 2 ** 40]]).tolist()
        bits = np.zeros(N, dtype=bool)
        bits[inside - base] = True
        for exclude, want in ((False, bits), (True, ~bits)):
            m = ops.row_mask_from_ids(ids, N, base=base, exclude=exclude)
            words = _np_words(want)
            assert m.words.dtype == torch.int32 and np.array_equal(m.words.numpy(), words)
            assert np.array_equal(m.live.numpy(), np.nonzero(words)[0]) and m.live.dtype == torch.int32
            assert m.count == int(want.sum()) and m.rows == N
            assert np.array_equal(ops.row_mask_bits(m).numpy(), want)
        lab = rng.integers(-5, 5, size=N).astype(np.int64)
        lab[0] = -2 ** 63
        lab[N - 1] = 2 ** 63 - 1
        t = torch.from_numpy(lab)
        assert np.array_equal(ops.row_mask_from_labels(t, values=[3, -2 ** 63, 3]).words.numpy(),
                              _np_words(np.isin(lab, [3, -2 ** 63])))
        assert np.array_equal(ops.row_mask_from_labels(t, lo=-1, hi=2).words.numpy(), _np_words((lab >= -1) & (lab <= 2)))
        assert ops.row_mask_from_labels(t, lo=2 ** 63 - 1, hi=2 ** 63 - 1).count == int((lab == 2 ** 63 - 1).sum())
        assert ops.row_mask_from_labels(t, lo=-2 ** 63, hi=2 ** 63 - 1).count == N
    for bad in (lambda: ops.row_mask_from_labels(t, values=[]), lambda: ops.row_mask_from_labels(t, values=list(range(257))),
                lambda: ops.row_mask_from_labels(t), lambda: ops.row_mask_from_labels(t, values=[1], lo=0, hi=1),
                lambda: ops.row_mask_from_labels(t, lo=0), lambda: ops.row_mask_from_labels(t.int(), values=[1]),
                lambda: ops.row_mask_from_ids([1], 0), lambda: ops.row_mask_from_ids(torch.tensor([1.5]), 4)):
        with pytest.raises(ValueError):
            bad()


def test_mask_rejections_on_the_cpu():
    q, c = _ints()
    N = c.shape[0]
    good = ops.row_mask_from_ids([1, 2, 3], N)
    for m in (good._replace(rows=N - 1), good._replace(words=good.words[:-1].contiguous()),
              good._replace(words=good.words.long()), good._replace(live=good.live.long()),
              good._replace(count=0), good._replace(count=N + 1), tuple(good)):
        for fn in (ops.sim_topk, ops.sim_topk_ref):
            with pytest.raises(ValueError):
                fn(q, c, 4, mask=m)


# --------------------------------------------------------------------------------------------- op
@pytest.fixture
def search(monkeypatch):
    monkeypatch.setenv("CLASSIFY_DEVICE", "cpu")
    monkeypatch.delenv("TASKS", raising=False)
    rs.clear_cache()
    yield registry.get_op("map_search")
    rs.clear_cache()


@pytest.fixture
def data(tmp_path):
    q, c = _ints()
    N = c.shape[0]
    labels = (np.arange(N) * 7 % 11).astype(np.int64)
    cpath, lpath = str(tmp_path / "ints.npy"), str(tmp_path / "labels.npy")
    np.save(cpath, c.numpy())
    np.save(lpath, labels.astype(np.int32))
    return q, c, labels, cpath, lpath


def test_each_filter_form_against_brute_force(search, data):
    q, c, labels, cpath, lpath = data
    N = c.shape[0]
    job = {"query_vectors": q.tolist(), "corpus_uri": cpath, "metric": "dot", "top_k": 6, "corpus_labels_uri": lpath}
    plain = search(dict(job))
    assert "filter_rows" not in plain
    ids = [3, 7, 40, N - 1, 0, 64, 65, 3]
    forms = [({"ids": ids}, sorted(set(ids))),
             ({"exclude_ids": ids}, [r for r in range(N) if r not in ids]),
             ({"labels": [4, 9, 4]}, [r for r in range(N) if labels[r] in (4, 9)]),
             ({"label_range": [2, 3]}, [r for r in range(N) if 2 <= labels[r] <= 3]),
             ({"label_range": [10, 10]}, [r for r in range(N) if labels[r] == 10]),
             ({"exclude_ids": []}, list(range(N)))]
    for flt, rows in forms:
        res = search(dict(job, filter=flt))
        ws, wi = _brute(q, c, 6, rows)
        assert res["filter_rows"] == len(rows) and res["corpus_rows"] == N, flt
        assert res["ids"] == wi and res["scores"] == ws, flt
        assert set(res) == set(plain) | {"filter_rows"}
    assert search(dict(job, filter={"exclude_ids": []}))["ids"] == plain["ids"]
    # the int64 label file and the file:// form
    l64 = lpath.replace("labels.npy", "labels64.npy")
    np.save(l64, labels)
    res = search(dict(job, filter={"labels": [4, 9]}, corpus_labels_uri="file://" + l64))
    assert res["ids"] == _brute(q, c, 6, forms[2][1])[1]
    # cosine, and the float16-resident corpus: the same rows are allowed
    for extra in ({"metric": "cosine"}, {"corpus_dtype": "float16"}, {"corpus_dtype": "float16", "metric": "cosine"}):
        res = search(dict(job, filter={"ids": ids}, **extra))
        assert res["filter_rows"] == 7 and all(len(set(x)) == 6 and set(x) <= set(ids) for x in res["ids"]), extra
        assert res["ids"][0][:4] == [3, 7, 40, N - 1]  # q[0] is that row: the four copies tie, ascending id


def test_short_lists_empty_lists_and_min_score_after_the_filter(search, data):
    q, c, labels, cpath, lpath = data
    job = {"query_vectors": q.tolist(), "corpus_uri": cpath, "metric": "dot", "top_k": 10, "corpus_labels_uri": lpath}
    res = search(dict(job, filter={"ids": [5, 3, 7]}))  # fewer allowed rows than top_k
    assert res["filter_rows"] == 3 and all(sorted(x) == [3, 5, 7] for x in res["ids"]) and res["top_k"] == 10
    assert all(len(x) == 3 for x in res["scores"])
    for flt in ({"ids": []}, {"label_range": [100, 200]}, {"labels": [-1]}, {"exclude_ids": list(range(c.shape[0]))}):
        res = search(dict(job, filter=flt))  # a filter that allows nothing is no error
        assert res["ok"] and res["filter_rows"] == 0 and res["ids"] == [[]] * 6 and res["scores"] == [[]] * 6
    full = search(dict(job, filter={"ids": [3, 5, 64]}))
    cut = (full["scores"][1][0] + full["scores"][1][1]) / 2
    low = search(dict(job, filter={"ids": [3, 5, 64]}, min_score=cut))
    assert low["filter_rows"] == 3 and low["ids"][1] == full["ids"][1][:1] and low["scores"][1] == full["scores"][1][:1]
    assert all(v >= cut for row in low["scores"] for v in row)
    assert search(dict(job, filter={"ids": [3]}, min_score=1e9))["ids"] == [[]] * 6


def test_results_without_a_filter_keep_their_keys(search, data):
    q, c, labels, cpath, lpath = data
    job = {"query_vectors": q.tolist(), "corpus_uri": cpath, "metric": "dot", "top_k": 6}
    res = search(dict(job))
    assert list(res) == ["ok", "op", "query_count", "corpus_rows", "dim", "top_k", "metric", "elapsed_ms",
                         "queries_per_sec", "index_cached", "ids", "scores"]
    ws, wi = _brute(q, c, 6, list(range(c.shape[0])))
    assert res["ids"] == wi and res["scores"] == ws
    # corpus_labels_uri without a label filter is ignored, even a bad one
    assert search(dict(job, corpus_labels_uri="/nope/labels.npy"))["ids"] == wi
    assert search(dict(job, corpus_labels_uri="/nope/labels.npy", filter={"ids": [1]}))["ids"] == [[1]] * 6


def test_ids_filters_work_with_corpus_texts(search):
    texts = ["the quick brown fox", "jumps over, the lazy dog!", "x", "seven rows in all", "a corpus row",
             "another corpus row", "the last one"]
    job = {"queries": texts[:3], "corpus_texts": texts, "model_path": MODEL, "top_k": 3}
    res = search(dict(job, filter={"ids": [1, 2, 6]}))
    assert res["filter_rows"] == 3 and [r[0] for r in res["ids"][1:]] == [1, 2] and sorted(res["ids"][0]) == [1, 2, 6]
    res = search(dict(job, filter={"exclude_ids": [0]}))
    assert res["filter_rows"] == 6 and 0 not in res["ids"][0]


def test_filter_errors_are_fixed_and_listed_in_the_contract(search, data, tmp_path):
    from ops import map_search as ms

    q, c, labels, cpath, lpath = data
    N = c.shape[0]
    contract = open(os.path.join(os.path.dirname(ms.__file__), "map_search.CONTRACT.md")).read()
    for key, msg in ms.FILTER_ERRORS.items():
        for m in ([msg.format(key="ids"), msg.format(key="exclude_ids")] if key == "filter_ids" else [msg]):
            assert m in contract, m
    assert ms.FILTER_ERRORS["labels_file"] == rs.LABEL_ERRORS["labels_file"]
    np.save(str(tmp_path / "short.npy"), labels[:-1])
    np.save(str(tmp_path / "l2d.npy"), labels.reshape(1, -1))
    np.save(str(tmp_path / "lf32.npy"), labels.astype(np.float32))
    np.save(str(tmp_path / "li16.npy"), labels.astype(np.int16))
    with open(tmp_path / "text.npy", "w") as f:
        f.write("not an npy file")
    t = lambda name: str(tmp_path / name)  # noqa: E731
    job = {"query_vectors": q.tolist(), "corpus_uri": cpath, "metric": "dot", "corpus_labels_uri": lpath}
    texts = {"queries": ["a"], "corpus_texts": ["a", "b"], "model_path": MODEL}
    ids_msg = lambda key: ms.FILTER_ERRORS["filter_ids"].format(key=key)  # noqa: E731
    cases = [
        ("filter", {"filter": None}), ("filter", {"filter": [1, 2]}), ("filter", {"filter": {}}),
        ("filter", {"filter": {"ids": [1], "labels": [1]}}), ("filter", {"filter": {"rows": [1]}}),
        (ids_msg("ids"), {"filter": {"ids": 3}}), (ids_msg("ids"), {"filter": {"ids": [1, "2"]}}),
        (ids_msg("ids"), {"filter": {"ids": [True]}}), (ids_msg("ids"), {"filter": {"ids": [1.0]}}),
        (ids_msg("ids"), {"filter": {"ids": [-1]}}), (ids_msg("ids"), {"filter": {"ids": [0, N]}}),
        (ids_msg("ids"), {"filter": {"ids": [2 ** 63]}}), (ids_msg("ids"), {"filter": {"ids": [0] * 1048577}}),
        (ids_msg("exclude_ids"), {"filter": {"exclude_ids": [N]}}),
        (ids_msg("exclude_ids"), {"filter": {"exclude_ids": (1, 2)}}),
        ("filter_labels", {"filter": {"labels": []}}), ("filter_labels", {"filter": {"labels": list(range(257))}}),
        ("filter_labels", {"filter": {"labels": [1, False]}}), ("filter_labels", {"filter": {"labels": [2 ** 63]}}),
        ("filter_labels", {"filter": {"labels": 4}}), ("filter_labels", {"filter": {"labels": [1.5]}}),
        ("filter_label_range", {"filter": {"label_range": [3, 2]}}),
        ("filter_label_range", {"filter": {"label_range": [1]}}),
        ("filter_label_range", {"filter": {"label_range": [1, 2, 3]}}),
        ("filter_label_range", {"filter": {"label_range": [1, 2.0]}}),
        ("filter_label_range", {"filter": {"label_range": [-2 ** 63 - 1, 0]}}),
        ("filter_label_range", {"filter": {"label_range": "1,2"}}),
        ("filter_labels_uri", {"filter": {"labels": [1]}, "corpus_labels_uri": None, "_drop": "corpus_labels_uri"}),
        ("labels_file", {"filter": {"labels": [1]}, "corpus_labels_uri": t("short.npy")}),
        ("labels_file", {"filter": {"labels": [1]}, "corpus_labels_uri": t("l2d.npy")}),
        ("labels_file", {"filter": {"label_range": [1, 2]}, "corpus_labels_uri": t("lf32.npy")}),
        ("labels_file", {"filter": {"labels": [1]}, "corpus_labels_uri": t("li16.npy")}),
        ("labels_file", {"filter": {"labels": [1]}, "corpus_labels_uri": t("text.npy")}),
        ("labels_file", {"filter": {"labels": [1]}, "corpus_labels_uri": t("missing.npy")}),
        ("labels_file", {"filter": {"labels": [1]}, "corpus_labels_uri": "s3://bucket/labels.npy"}),
        ("labels_file", {"filter": {"labels": [1]}, "corpus_labels_uri": 17}),
    ]
    seen = set()
    for key, extra in cases:
        payload = dict(job, **extra)
        payload.pop(payload.pop("_drop", "_none"), None)
        with pytest.raises(ValueError) as ei:
            search(payload)
        want = ms.FILTER_ERRORS.get(key, key)
        assert str(ei.value) == want, (key, extra)
        seen.add(want)
    # a label filter over corpus_texts has no file to go with
    for flt in ({"labels": [1]}, {"label_range": [0, 1]}):
        with pytest.raises(ValueError) as ei:
            search(dict(texts, filter=flt, corpus_labels_uri=lpath))
        assert str(ei.value) == ms.FILTER_ERRORS["filter_labels_uri"]
    with pytest.raises(ValueError) as ei:  # ids are checked against the rows of corpus_texts as well
        search(dict(texts, filter={"ids": [2]}))
    assert str(ei.value) == ids_msg("ids")
    assert seen == {m for k, m in ms.FILTER_ERRORS.items() if k != "filter_ids"} | {ids_msg("ids"), ids_msg("exclude_ids")}
    # the other errors come first, as before
    with pytest.raises(ValueError) as ei:
        search(dict(job, top_k=0, filter={"ids": "x"}))
    assert str(ei.value) == ms.ERRORS["top_k"]


def test_labels_lru_hits_and_reloads_a_rewritten_file(search, data, monkeypatch):
    q, c, labels, cpath, lpath = data
    N = c.shape[0]
    job = {"query_vectors": q.tolist(), "corpus_uri": cpath, "metric": "dot", "top_k": 4, "corpus_labels_uri": lpath,
           "filter": {"labels": [0]}}
    before = rs.cache_info()
    assert before["label_entries"] == [] and before["entries"] == []
    first = search(dict(job))
    info = rs.cache_info()
    assert info["label_entries"] == [os.path.realpath(lpath)] and info["label_bytes"] == N * 8  # resident as int64
    assert info["label_loads"] == before["label_loads"] + 1 and info["label_hits"] == before["label_hits"]
    assert info["entries"] == [os.path.realpath(cpath)] and info["resident_bytes"] == N * 64 * 4  # vectors only
    assert info["capacity"] == rs.lru_capacity()
    second = search(dict(job, filter={"label_range": [0, 0]}))  # another filter, the same labels: a hit
    info2 = rs.cache_info()
    assert info2["label_hits"] == info["label_hits"] + 1 and info2["label_loads"] == info["label_loads"]
    assert second["ids"] == first["ids"] and second["index_cached"] is True
    lab = rs.load_labels(lpath, 0, -1, torch.device("cpu"), N)
    assert lab.dtype == torch.int64 and lab.tolist() == labels.tolist()
    assert rs.load_labels(lpath, 10, 5, torch.device("cpu"), N).tolist() == labels[10:15].tolist()  # a slice: its own entry
    # a rewritten file is reloaded
    st = os.stat(lpath)
    np.save(lpath, ((labels + 1) % 11).astype(np.int32))
    os.utime(lpath, ns=(st.st_atime_ns, st.st_mtime_ns + 1_000_000))
    third = search(dict(job))
    rows = [r for r in range(N) if (labels[r] + 1) % 11 == 0]
    assert third["filter_rows"] == len(rows) and third["ids"] == _brute(q, c, 4, rows)[1] and third["ids"] != first["ids"]
    assert rs.cache_info()["label_loads"] == info2["label_loads"] + 2  # the slice above, and the rewritten file
    # the label LRU has the vector LRU's capacity
    monkeypatch.setenv("SEARCH_INDEX_LRU_SIZE", "1")
    rs.load_labels(lpath, 0, 3, torch.device("cpu"), N)
    assert len(rs.cache_info()["label_entries"]) == 1
    rs.clear_cache()
    assert rs.cache_info()["label_entries"] == []


def test_batch_handler_groups_by_filter(search, tmp_path):
    texts = ["the quick brown fox", "jumps over, the lazy dog!", "MI355X " * 30, "x", "seven rows in all",
             "an index of sentence vectors", "nearest neighbours by cosine", "a corpus row", "another corpus row",
             "the last one"]
    path, lpath = str(tmp_path / "corpus.npy"), str(tmp_path / "labels.npy")
    assert registry.get_op("map_embed")({"texts": texts, "model_path": MODEL, "output": "npy", "output_uri": path})["ok"]
    np.save(lpath, np.arange(10, dtype=np.int64) % 3)
    batch = registry.get_batch_op("map_search")
    job = {"corpus_uri": path, "model_path": MODEL, "corpus_labels_uri": lpath}
    payloads = [
        dict(job, queries=texts[:3], top_k=2, filter={"ids": [1, 5, 7, 9]}),
        dict(job, queries=texts[3:5], top_k=7, filter={"ids": [9, 7, 5, 1, 1]}),  # the same filter, written differently
        dict(job, queries=texts[5:7], top_k=3, filter={"exclude_ids": [1, 5, 7, 9]}),
        dict(job, queries=texts[7:], top_k=3, filter={"labels": [0, 2]}),
        dict(job, queries=texts[:2], top_k=3, filter={"label_range": [0, 0]}),
        dict(job, queries=texts[:2], top_k=3),
        dict(job, queries=texts[:2], top_k=3, filter={"ids": [10]}),
        dict(job, queries=texts[:2], top_k=3, filter={"labels": []}),
    ]
    calls = []
    from ops import map_search as ms

    real = ms.search_queries

    def counting(*a, **kw):
        calls.append(a[10] if len(a) > 10 else kw.get("flt"))
        return real(*a, **kw)

    ms.search_queries = counting
    try:
        res = batch([dict(p) for p in payloads])
    finally:
        ms.search_queries = real
    assert [r[0] for r in res] == ["ok"] * 6 + ["err", "err"]
    assert str(res[6][1]) == ms.FILTER_ERRORS["filter_ids"].format(key="ids")
    assert str(res[7][1]) == ms.FILTER_ERRORS["filter_labels"]
    assert len(calls) == 6  # jobs 0 and 1 share one search; the bad ids job reaches its own and fails there
    for n in range(6):
        one, got = search(dict(payloads[n])), res[n][1]
        assert set(one) == set(got), n
        for key in one:
            if key not in ("elapsed_ms", "queries_per_sec", "index_cached"):
                assert got[key] == one[key], (n, key)
    assert res[0][1]["filter_rows"] == 4 and len(res[1][1]["ids"][0]) == 4 and "filter_rows" not in res[5][1]
    assert res[4][1]["filter_rows"] == 4 and all(set(x) <= {0, 3, 6, 9} for x in res[4][1]["ids"])
