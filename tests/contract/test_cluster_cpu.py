"""map_cluster on a CPU engine: the fixed-point sums, the k-means twins, the loop and the op's forms and errors."""
import numpy as np
import pytest
import torch

import ops as registry
from agent_tpu_amd import ops
from agent_tpu_amd.runtime import cluster as rc
from agent_tpu_amd.runtime import search as rs


@pytest.fixture(autouse=True)
def _cpu_engine(monkeypatch):
    monkeypatch.setenv("CLASSIFY_DEVICE", "cpu")
    rs.clear_cache()
    yield
    rs.clear_cache()


def _run(payload):
    return registry.get_op("map_cluster")(payload)


def _blobs(N, K, D, seed):
    """Well-separated blobs: centre k is 40 on its own block of columns, integer noise in {-1, 0, 1}."""
    gen = torch.Generator().manual_seed(seed)
    centres = torch.zeros((K, D))
    w = D // K
    for k in range(K):
        centres[k, k * w:(k + 1) * w] = 40.0
    planted = torch.randint(0, K, (N,), generator=gen)
    x = centres[planted] + torch.randint(-1, 2, (N, D), generator=gen).float()
    return x.contiguous(), planted


# --------------------------------------------------------------------------------------- fixed-point sums
def test_fixed_shift_at_its_edges():
    assert ops.fixed_shift(2 ** 20, 1.0) == 42  # unit rows, 2^20 of them
    assert ops.fixed_shift(2 ** 20, 0.75) == 42 and ops.fixed_shift(2 ** 20, 1.0000001) == 41
    assert ops.fixed_shift(2 ** 20 + 1, 1.0) == 41
    assert ops.fixed_shift(1, 1.0) == 61 and ops.fixed_shift(2, 1.0) == 61 and ops.fixed_shift(3, 1.0) == 60
    assert ops.fixed_shift(1, 0.0) == 61  # all-zero input: every sum is zero whatever the shift
    assert ops.fixed_shift(4, 4.0) == 58 and ops.fixed_shift(4, 0.25) == 62 and ops.fixed_shift(4, 2.0 ** -30) == 90
    for n, a in ((1000, 3.7), (2 ** 31 - 256, 1.0), (5, 2.0 ** -100)):
        s = ops.fixed_shift(n, a)
        assert n * a * 2.0 ** s <= 2.0 ** 62 < 4 * max(n, 2) * a * 2.0 ** s  # fits, and is not wastefully small
    for bad in (lambda: ops.fixed_shift(0, 1.0), lambda: ops.fixed_shift(4, float("inf")), lambda: ops.fixed_shift(4, -1.0)):
        with pytest.raises(ValueError):
            bad()


def test_rounding_is_ties_to_even_also_for_negative_halves():
    v = torch.tensor([0.25, 0.75, 1.25, 1.75, -0.25, -0.75, -1.25, -1.75, 0.26, -0.26])
    from agent_tpu_amd.ops.cluster import to_fixed

    assert to_fixed(v, 1).tolist() == [0, 2, 2, 4, 0, -2, -2, -4, 1, -1]
    assert ops.fixed_sum(v[:8].contiguous(), 1).tolist() == [0]
    assert ops.fixed_sum(torch.zeros(5), 61).tolist() == [0]


def test_integer_sums_do_not_depend_on_row_order_or_on_a_split():
    gen = torch.Generator().manual_seed(0)
    N, K, D = 999, 7, 64
    x = torch.nn.functional.normalize(torch.randn(N, D, generator=gen), dim=1).contiguous()
    labels = torch.randint(0, K, (N,), generator=gen).to(torch.int32)
    s = ops.fixed_shift(N, float(x.abs().max()))
    sums, counts = ops.kmeans_update(x, labels, K, s)
    perm = torch.randperm(N, generator=gen)
    ps, pc = ops.kmeans_update(x[perm].contiguous(), labels[perm].contiguous(), K, s)
    assert torch.equal(ps, sums) and torch.equal(pc, counts)
    for ways in (1, 2, 3):
        ts, tc = torch.zeros_like(sums), torch.zeros_like(counts)
        for r in range(ways):
            lo, hi = r * N // ways, (r + 1) * N // ways
            a, b = ops.kmeans_update(x[lo:hi].contiguous(), labels[lo:hi].contiguous(), K, s)
            ts, tc = ts + a, tc + b
        assert torch.equal(ts, sums) and torch.equal(tc, counts), ways
    # the means are within 5e-10 of an fp64 reference (s = 52: rounding 2^-53 per value)
    mean64 = torch.stack([x[labels == k].double().mean(0) for k in range(K)])
    assert (sums.double() / (counts.double()[:, None] * 2.0 ** s) - mean64).abs().max() < 5e-10
    v = x.reshape(-1).contiguous()
    assert torch.equal(ops.fixed_sum(v, s), ops.fixed_sum(v.flip(0).contiguous(), s))


# ------------------------------------------------------------------------------------------------- twins
def test_assign_twin_orders_ties_by_id_and_counts_changes():
    gen = torch.Generator().manual_seed(1)
    x = torch.randint(-2, 3, (40, 64), generator=gen).float()
    c = torch.randint(-2, 3, (6, 64), generator=gen).float()
    c[4] = c[1]
    x[7] = 0.0
    labels, best, changed = ops.kmeans_assign(x, c)
    s = x.double() @ c.double().T
    want = [min(range(6), key=lambda j: (-row[j], j)) for row in s.tolist()]
    assert labels.tolist() == want and labels.dtype == torch.int32 and not (labels == 4).any() and labels[7] == 0
    assert torch.equal(best.double(), s.gather(1, labels.long()[:, None])[:, 0]) and changed.tolist() == [40]
    prev = labels.clone()
    prev[:5] = 5 - prev[:5]  # 0..5 -> 5..0: differs unless 2.5
    _, _, ch = ops.kmeans_assign(x, c, None, prev)
    assert ch.tolist() == [int((prev != labels).sum())]
    bias = torch.tensor([0.0, 0.0, 0.0, 0.0, 0.5, 0.0])  # the duplicate now wins where centroid 1 did
    lb, bb, _ = ops.kmeans_assign(x, c, bias)
    assert (lb[labels == 1] == 4).all() and torch.equal(bb[labels == 1], best[labels == 1] + 0.5)
    # a row's bits do not depend on the batch it is in
    l1, b1, _ = ops.kmeans_assign(x[11:12].contiguous(), c)
    assert l1[0] == labels[11] and b1[0] == best[11]
    with pytest.raises(ValueError):
        ops.kmeans_assign(x, c[:, :32].contiguous())
    with pytest.raises(ValueError):
        ops.kmeans_assign(x, c, torch.zeros(5))
    assert ops.kmeans_ok(768, 4096) and not ops.kmeans_ok(768, 4097) and not ops.kmeans_ok(96, 4) and not ops.kmeans_ok(64, 0)


def test_finalize_twin_means_norms_and_empty_clusters():
    gen = torch.Generator().manual_seed(2)
    x = torch.randn(50, 64, generator=gen)
    labels = torch.randint(0, 3, (50,), generator=gen).to(torch.int32)
    labels[labels == 1] = 2
    s = ops.fixed_shift(50, float(x.abs().max()))
    sums, counts = ops.kmeans_update(x, labels, 3, s)
    old = torch.randn(3, 64, generator=gen)
    c, b = ops.kmeans_finalize(sums, counts, old, s, "l2")
    assert counts.tolist()[1] == 0 and torch.equal(c[1], old[1])
    for k in (0, 2):
        assert (c[k].double() - x[labels == k].double().mean(0)).abs().max() < 1e-7
    assert torch.allclose(b.double(), -0.5 * (c.double() ** 2).sum(1), rtol=1e-7, atol=0)
    cc, bb = ops.kmeans_finalize(sums, counts, old, s, "cosine")
    assert bb is None and torch.equal(cc[1], old[1])
    assert (cc[[0, 2]].double().norm(dim=1) - 1.0).abs().max() < 1e-7
    assert torch.allclose(cc[0], torch.nn.functional.normalize(c[0], dim=0), atol=1e-7)
    with pytest.raises(ValueError):
        ops.kmeans_finalize(sums, counts, old, s, "dot")


# -------------------------------------------------------------------------------------------------- loop
@pytest.mark.parametrize("metric", ["cosine", "l2"])
def test_blobs_converge_to_the_planted_partition(metric):
    x, planted = _blobs(400, 4, 64, 5)
    r = _run({"vectors": x.tolist(), "k": 4, "metric": metric, "seed": 2})
    assert r["ok"] and r["op"] == "map_cluster" and r["converged"] is True and r["changed_last"] == 0
    assert r["row_count"] == 400 and r["dim"] == 64 and r["k"] == 4 and r["metric"] == metric and r["dp_world_size"] == 1
    assert len(set(zip(planted.tolist(), r["labels"]))) == 4 and r["empty_clusters"] == 0
    assert sorted(r["sizes"]) == sorted(torch.bincount(planted).tolist()) and 2 <= r["iterations"] <= 25
    again = _run({"vectors": x.tolist(), "k": 4, "metric": metric, "seed": 2})
    for key in ("labels", "centroids", "sizes", "objective", "iterations"):
        assert again[key] == r[key], key  # the same seed: the same result
    cent = torch.tensor(r["centroids"])
    xs = rs.normalize_rows(x) if metric == "cosine" else x
    lab = torch.tensor(r["labels"])
    if metric == "cosine":
        want = (xs.double() * cent.double()[lab]).sum()
    else:
        want = ((xs.double() - cent.double()[lab]) ** 2).sum()
    assert abs(r["objective"] - float(want)) <= 1e-4 * abs(float(want))
    assert "index_cached" not in r and "representatives" not in r


def test_duplicate_centroids_k_one_and_k_rows():
    x, _ = _blobs(30, 3, 64, 6)
    # two equal initial centroids: the tie goes to the lower id, the other cluster is empty and keeps its centroid
    init = [x[0].tolist(), x[0].tolist()]
    r = _run({"vectors": x.tolist(), "k": 2, "metric": "l2", "init_centroids": init, "max_iter": 1})
    assert r["sizes"] == [30, 0] and r["empty_clusters"] == 1 and set(r["labels"]) == {0}
    assert r["centroids"][1] == x[0].tolist()
    assert np.allclose(r["centroids"][0], x.double().mean(0).numpy(), atol=1e-5)
    one = _run({"vectors": x.tolist(), "k": 1})
    assert one["sizes"] == [30] and one["converged"] and one["iterations"] == 2 and set(one["labels"]) == {0}
    every = _run({"vectors": x.tolist(), "k": 30, "metric": "l2", "output": "summary"})
    assert "labels" not in every and "centroids" not in every and sum(every["sizes"]) == 30 and every["converged"]
    assert every["objective"] == 0.0 or every["empty_clusters"] > 0  # every row its own centroid unless rows repeat


def test_init_centroids_max_iter_and_tol():
    x, planted = _blobs(200, 4, 64, 7)
    init = torch.stack([x[int((planted == k).nonzero()[0, 0])] for k in range(4)])
    r = _run({"vectors": x.tolist(), "k": 4, "metric": "l2", "init_centroids": init.tolist()})
    assert r["labels"] == planted.tolist() and r["converged"]  # the clusters are named by the given centroids
    one = _run({"vectors": x.tolist(), "k": 4, "metric": "l2", "init_centroids": init.tolist(), "max_iter": 1})
    assert one["iterations"] == 1 and one["converged"] is False and one["changed_last"] == 200
    assert one["labels"] == planted.tolist()
    loose = _run({"vectors": x.tolist(), "k": 4, "metric": "l2", "init_centroids": init.tolist(), "tol": 0.999})
    assert loose["iterations"] == 2 and loose["converged"] is True
    km = rc.kmeans(x, 4, "l2", init=init)
    assert km.labels.tolist() == planted.tolist() and km.sizes.tolist() == torch.bincount(planted).tolist()


def test_representatives_are_ordered_members(tmp_path):
    x, planted = _blobs(120, 3, 64, 8)
    x[5] = x[2]  # equal rows: equal scores come back in ascending id
    path = str(tmp_path / "v.npy")
    np.save(path, x.numpy())
    for metric in ("cosine", "l2"):
        r = _run({"vectors_uri": path, "k": 3, "metric": metric, "seed": 1, "representatives": 5})
        assert len(r["representatives"]) == 3 and r["index_cached"] is False
        for k, rep in enumerate(r["representatives"]):
            assert 1 <= len(rep["ids"]) <= 5 and len(rep["ids"]) == len(rep["scores"])
            assert all(r["labels"][i] == k for i in rep["ids"])
            pairs = [(-s, i) for s, i in zip(rep["scores"], rep["ids"])]
            assert pairs == sorted(pairs)
        assert _run({"vectors_uri": path, "k": 3, "metric": metric, "seed": 1})["index_cached"] is True
    r = _run({"vectors_uri": path, "k": 3, "metric": "l2", "seed": 1, "representatives": 32})
    members = {k: [i for i, l in enumerate(r["labels"]) if l == k] for k in range(3)}
    for k, rep in enumerate(r["representatives"]):
        assert len(rep["ids"]) == min(32, len(members[k])) and set(rep["ids"]) <= set(members[k])


def test_npy_output_and_texts_form(tmp_path):
    x, _ = _blobs(50, 2, 64, 9)
    path = str(tmp_path / "v.npy")
    np.save(path, x.numpy().astype("<f2"))  # a float16 file is widened on load
    out = str(tmp_path / "res.npy")
    r = _run({"vectors_uri": "file://" + path, "k": 2, "output": "npy", "output_uri": out, "seed": 3})
    assert "labels" not in r and r["labels_uri"] == str(tmp_path / "res.labels.npy")
    lab, cen = np.load(r["labels_uri"]), np.load(r["centroids_uri"])
    assert lab.dtype == np.int32 and lab.shape == (50,) and cen.dtype == np.float32 and cen.shape == (2, 64)
    rows = _run({"vectors_uri": path, "k": 2, "seed": 3})
    assert rows["labels"] == lab.tolist() and rows["centroids"] == cen.tolist()
    assert not [p for p in tmp_path.iterdir() if p.name.endswith(".part")]
    t = _run({"texts": ["alpha beta", "gamma", None, "alpha beta", "delta"], "k": 2,
              "model_path": "bert-tiny?batch=8&seq=32&seed=4"})
    assert t["row_count"] == 5 and t["dim"] == 256 and len(t["labels"]) == 5 and t["labels"][0] == t["labels"][3]


# ------------------------------------------------------------------------------------------------ errors
def test_every_error_string(tmp_path, monkeypatch):
    from ops.map_cluster import ERRORS

    v = [[1.0, 0.0], [0.0, 1.0], [1.0, 1.0]]
    cases = [
        ({"k": 2}, "source"), ({"k": 2, "vectors": v, "texts": ["a", "b"]}, "source"),
        ({"k": 2, "texts": "ab"}, "texts"), ({"k": 2, "texts": ["a", 3]}, "texts"),
        ({"k": 2, "vectors": [[1.0], [1.0, 2.0]]}, "vectors"),
        ({"k": 2, "vectors": [[1.0, float("nan")], [0.0, 1.0]]}, "vectors"),
        ({"k": 2, "vectors": []}, "vectors"), ({"k": 2, "vectors": [[], []]}, "vectors"),
        ({"vectors": v}, "k"), ({"k": 0, "vectors": v}, "k"), ({"k": 4097, "vectors": v}, "k"), ({"k": True, "vectors": v}, "k"),
        ({"k": 2.0, "vectors": v}, "k"), ({"k": 4, "vectors": v}, "k_rows"), ({"k": 2, "texts": ["a"]}, "k_rows"),
        ({"k": 1, "texts": []}, "rows_empty"),
        ({"k": 2, "vectors": v, "metric": "dot"}, "metric"), ({"k": 2, "vectors": v, "pooling": "max"}, "pooling"),
        ({"k": 2, "vectors": v, "max_iter": 0}, "max_iter"), ({"k": 2, "vectors": v, "max_iter": 301}, "max_iter"),
        ({"k": 2, "vectors": v, "tol": 1}, "tol"), ({"k": 2, "vectors": v, "tol": -0.1}, "tol"),
        ({"k": 2, "vectors": v, "tol": "x"}, "tol"), ({"k": 2, "vectors": v, "seed": -1}, "seed"),
        ({"k": 2, "vectors": v, "seed": 1.5}, "seed"),
        ({"k": 2, "vectors": v, "init_centroids": [[1.0, 0.0]]}, "init_centroids"),
        ({"k": 2, "vectors": v, "init_centroids": [[1.0], [2.0]]}, "init_centroids"),
        ({"k": 2, "vectors": v, "init_centroids": "x"}, "init_centroids"),
        ({"k": 2, "vectors": v, "representatives": 33}, "representatives"),
        ({"k": 2, "vectors": v, "representatives": -1}, "representatives"),
        ({"k": 2, "vectors": v, "output": "base64"}, "output"), ({"k": 2, "vectors": v, "output": "npy"}, "output_uri"),
        ({"k": 2, "vectors": v, "output": "npy", "output_uri": "s3://b/x.npy"}, "output_uri"),
        ({"k": 2, "vectors_uri": "http://host/x.npy"}, "corpus_file"), ({"k": 2, "vectors_uri": 5}, "corpus_file"),
        ({"k": 2, "vectors_uri": str(tmp_path / "missing.npy")}, "corpus_file"),
    ]
    np.save(str(tmp_path / "one_d.npy"), np.zeros(8, dtype=np.float32))
    np.save(str(tmp_path / "empty.npy"), np.zeros((0, 64), dtype=np.float32))
    bad = np.ones((4, 64), dtype=np.float32)
    bad[2, 3] = np.inf
    np.save(str(tmp_path / "inf.npy"), bad)
    np.save(str(tmp_path / "ok.npy"), np.eye(4, 64, dtype=np.float32))
    cases += [({"k": 2, "vectors_uri": str(tmp_path / "one_d.npy")}, "corpus_file"),
              ({"k": 2, "vectors_uri": str(tmp_path / "empty.npy")}, "corpus_empty"),
              ({"k": 2, "vectors_uri": str(tmp_path / "inf.npy")}, "corpus_nonfinite"),
              ({"k": 5, "vectors_uri": str(tmp_path / "ok.npy")}, "k_rows"),
              ({"k": 2, "vectors_uri": str(tmp_path / "ok.npy"), "init_centroids": [[1.0, 0.0], [0.0, 1.0]]}, "init_centroids")]
    for payload, key in cases:
        with pytest.raises(ValueError) as e:
            _run(payload)
        assert str(e.value) == ERRORS[key], (payload, key)
    monkeypatch.setenv("MAP_EMBED_MAX_JSON_VALUES", "100")
    with pytest.raises(ValueError) as e:
        _run({"k": 2, "vectors_uri": str(tmp_path / "ok.npy")})
    assert str(e.value) == ERRORS["too_large"]
    assert _run({"k": 2, "vectors_uri": str(tmp_path / "ok.npy"), "output": "summary"})["ok"]
    monkeypatch.setenv("SEARCH_INDEX_MAX_GB", "0.0000001")
    rs.clear_cache()
    with pytest.raises(ValueError) as e:
        _run({"k": 2, "vectors_uri": str(tmp_path / "ok.npy"), "output": "summary"})
    assert str(e.value) == ERRORS["corpus_too_large"]
    text = open(registry.__file__.replace("__init__.py", "map_cluster.CONTRACT.md")).read()
    for msg in ERRORS.values():
        assert msg in text, msg
