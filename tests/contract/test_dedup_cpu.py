"""map_dedup on a CPU engine: the join and connected-components twins, the runtime and the op's forms and errors."""
import struct

import numpy as np
import pytest
import torch

import ops as registry
from agent_tpu_amd import ops
from agent_tpu_amd.runtime import dedup as rd
from agent_tpu_amd.runtime import search as rs


@pytest.fixture(autouse=True)
def _cpu_engine(monkeypatch):
    monkeypatch.setenv("CLASSIFY_DEVICE", "cpu")
    rs.clear_cache()
    yield
    rs.clear_cache()


def _run(payload):
    return registry.get_op("map_dedup")(payload)


def _planted(N, D, seed, groups=10):
    """Integer rows: rows 3k + 1 and 3k + 2 copy row 3k, the second with one coordinate zeroed."""
    gen = torch.Generator().manual_seed(seed)
    x = torch.randint(-2, 3, (N, D), generator=gen).float()
    group = list(range(N))
    for k in range(groups):
        a = 3 * k
        x[a + 1] = x[a]
        x[a + 2] = x[a]
        x[a + 2, k] = 0.0
        group[a + 1] = group[a + 2] = a
    return x.contiguous(), group


def _threshold(x, group):
    S = x.long() @ x.long().T
    g = torch.tensor(group)
    planted = g[:, None] == g[None, :]
    t = int(S[planted & ~torch.eye(len(group), dtype=torch.bool)].min())
    assert int(S[~planted].max()) < t
    return t


# ------------------------------------------------------------------------------------------------- twins
def test_join_twin_on_toy_data():
    x = torch.zeros((4, 64))
    x[0, 0] = x[1, 0] = x[3, 0] = 2.0  # rows 0, 1, 3 identical; row 2 orthogonal
    x[2, 1] = 2.0
    pairs, scores, count = ops.sim_join(x, x, 4.0)
    assert pairs.tolist() == [[0, 1], [0, 3], [1, 3]] and scores.tolist() == [4.0] * 3 and count.tolist() == [3]
    assert pairs.dtype == torch.int32 and scores.dtype == torch.float32 and count.dtype == torch.int64
    assert ops.sim_join(x, x, 4.000001)[2].tolist() == [0]  # >= on the fp32 value
    assert ops.sim_join(x, x, 0.0)[0].tolist() == [[0, 1], [0, 2], [0, 3], [1, 2], [1, 3], [2, 3]]  # never (i, i)
    # a block of the self-join: ids are x_base + i, and only I < J passes
    p, s, c = ops.sim_join(x[1:3].contiguous(), x, 4.0, x_base=1)
    assert p.tolist() == [[1, 3]] and c.tolist() == [1]
    # a rectangle: every pair is live, the x side is the lower id
    p, _, _ = ops.sim_join(x[:2].contiguous(), x[2:].contiguous(), 4.0, x_base=0, y_base=2)
    assert p.tolist() == [[0, 3], [1, 3]]
    # cap: the true count, the first cap pairs
    p, s, c = ops.sim_join(x, x, 4.0, cap=2)
    assert p.tolist() == [[0, 1], [0, 3]] and s.shape == (2,) and c.tolist() == [3]
    assert ops.sim_join(x, x, 4.0, cap=0)[2].tolist() == [3]
    # a pair's bits do not depend on the batch it is in
    gen = torch.Generator().manual_seed(0)
    r = torch.randn(50, 128, generator=gen)
    pa, sa, _ = ops.sim_join(r, r, -100.0)
    pb, sb, _ = ops.sim_join(r[17:18].contiguous(), r, -100.0, x_base=17)
    assert torch.equal(sa[pa[:, 0] == 17], sb) and torch.equal(pa[pa[:, 0] == 17], pb)
    assert ops.sim_join_ok(64) and ops.sim_join_ok(1024) and not ops.sim_join_ok(96) and not ops.sim_join_ok(1088)
    for bad in (lambda: ops.sim_join(x, x[:, :32].contiguous(), 1.0), lambda: ops.sim_join(x[:, :32].contiguous(), x[:, :32].contiguous(), 1.0),
                lambda: ops.sim_join(x, x, 1.0, x_base=-1), lambda: ops.sim_join(x, x, 1.0, cap=-1),
                lambda: ops.sim_join(x, x, 1.0, y_base=2 ** 31 - 256), lambda: ops.sim_join(x, x, "1")):
        with pytest.raises(ValueError):
            bad()


def test_sort_pairs_orders_by_i_then_j():
    pairs = torch.tensor([[3, 9], [0, 70000], [3, 4], [0, 2]], dtype=torch.int32)
    p, s = ops.sort_pairs(pairs, torch.tensor([1.0, 2.0, 3.0, 4.0]))
    assert p.tolist() == [[0, 2], [0, 70000], [3, 4], [3, 9]] and s.tolist() == [4.0, 2.0, 3.0, 1.0]


def test_cc_twin_on_toy_graphs():
    e = torch.tensor([[4, 2], [7, 9], [9, 8], [2, 0], [0, 4], [0, 4]], dtype=torch.int32)
    assert ops.cc_min_labels(e, 12).tolist() == [0, 1, 0, 3, 0, 5, 6, 7, 7, 7, 10, 11]
    labels, rounds = ops.cc_min_labels(torch.empty((0, 2), dtype=torch.int32), 5, with_rounds=True)
    assert labels.tolist() == [0, 1, 2, 3, 4] and rounds == 0 and labels.dtype == torch.int32
    path = torch.tensor([[i + 1, i] for i in range(999)], dtype=torch.int32)
    labels, rounds = ops.cc_min_labels(path[torch.randperm(999, generator=torch.Generator().manual_seed(1))].contiguous(),
                                       1000, with_rounds=True)
    assert labels.tolist() == [0] * 1000 and rounds <= 20  # see test_dedup_gpu.py for the bound
    with pytest.raises(ValueError):
        ops.cc_min_labels(torch.tensor([[0, 5]], dtype=torch.int32), 5)
    with pytest.raises(ValueError):
        ops.cc_min_labels(torch.tensor([[0, 1]], dtype=torch.int64), 5)


def test_runtime_does_not_depend_on_the_block_size_or_the_rank_split(monkeypatch):
    x, group = _planted(150, 64, 3)
    t = float(_threshold(x, group))
    want = rd.near_duplicates(x, t)
    assert want.labels.tolist() == group and want.pairs.shape[0] == 30
    assert want.pairs.tolist() == sorted(want.pairs.tolist())
    monkeypatch.setattr(rd, "MIN_CAP", 1)  # blocks of 2 rows: cap = 8, block 0 of a lower threshold has more
    low = rd.near_duplicates(x, 0.0, block_rows=2)
    ref = rd.near_duplicates(x, 0.0, block_rows=4096)
    assert torch.equal(low.pairs, ref.pairs) and torch.equal(low.scores, ref.scores) and low.pairs.shape[0] > 1000
    for block_rows in (1, 7, 64):
        got = rd.near_duplicates(x, t, block_rows=block_rows)
        assert torch.equal(got.pairs, want.pairs) and torch.equal(got.scores, want.scores)
        assert torch.equal(got.labels, want.labels)
        # the blocks of the ranks of a world of 3 partition the pairs
        parts = []
        for r in range(3):
            for b, b0 in enumerate(range(0, 150, block_rows)):
                if b % 3 == r:
                    parts.append(rd.join_block(x, b0, min(b0 + block_rows, 150), t)[0])
        assert sorted(torch.cat(parts).tolist()) == want.pairs.tolist()
    with pytest.raises(ValueError):
        rd.near_duplicates(x, t, total=151)


# ---------------------------------------------------------------------------------------------------- op
def test_output_forms_and_counts(tmp_path):
    x, group = _planted(100, 64, 4)
    t = _threshold(x, group)
    path = str(tmp_path / "v.npy")
    np.save(path, x.numpy())
    r = _run({"vectors_uri": path, "threshold": t, "metric": "dot"})
    assert r["ok"] and r["op"] == "map_dedup" and r["row_count"] == 100 and r["dim"] == 64 and r["metric"] == "dot"
    assert r["threshold"] == float(t) and r["dp_world_size"] == 1 and r["index_cached"] is False
    assert r["group"] == group and r["keep"] == [i for i in range(100) if group[i] == i]
    assert r["pair_count"] == 30 and r["group_count"] == 10 and r["duplicate_count"] == 20 and r["kept_count"] == 80
    assert r["largest_group"] == 3 and "pairs" not in r and "group_uri" not in r
    assert _run({"vectors_uri": path, "threshold": t, "metric": "dot"})["index_cached"] is True
    s = _run({"vectors_uri": "file://" + path, "threshold": t, "metric": "dot", "output": "summary"})
    assert "group" not in s and "keep" not in s and s["pair_count"] == 30
    out = str(tmp_path / "res.npy")
    n = _run({"vectors_uri": path, "threshold": 0.9, "output": "npy", "output_uri": out})
    assert n["metric"] == "cosine" and n["group_uri"] == str(tmp_path / "res.group.npy") and "group" not in n
    g = np.load(n["group_uri"])
    assert g.dtype == np.int32 and g.tolist() == group
    assert not [p for p in tmp_path.iterdir() if p.name.endswith(".part")]
    none = _run({"vectors": x[:64].tolist(), "threshold": 1e6, "metric": "dot"})
    assert none["pair_count"] == 0 and none["group_count"] == 0 and none["duplicate_count"] == 0
    assert none["largest_group"] == 1 and none["keep"] == list(range(64)) and "index_cached" not in none
    one = _run({"vectors": x[:1].tolist(), "threshold": 0.5})
    assert one["row_count"] == 1 and one["group"] == [0] and one["pair_count"] == 0
    np.save(str(tmp_path / "h.npy"), x.numpy().astype("<f2"))  # a float16 file is widened on load
    assert _run({"vectors_uri": str(tmp_path / "h.npy"), "threshold": t, "metric": "dot"})["group"] == group
    txt = _run({"texts": ["alpha beta", "gamma", None, "alpha beta", ""], "threshold": 0.99999,
                "model_path": "bert-tiny?batch=8&seq=32&seed=4"})
    assert txt["row_count"] == 5 and txt["dim"] == 256 and txt["group"][3] == 0 and txt["group"][4] == 2


def test_max_pairs_order():
    x = torch.zeros((6, 64))
    x[0, :4] = torch.tensor([2.0, 0.0, 0.0, 0.0])
    x[1, :4] = torch.tensor([2.0, 0.0, 0.0, 0.0])
    x[2, :4] = torch.tensor([2.0, 1.0, 0.0, 0.0])
    x[3, :4] = torch.tensor([2.0, 1.0, 0.0, 0.0])
    x[4, :4] = torch.tensor([1.0, 0.0, 0.0, 0.0])
    x[5, :4] = torch.tensor([0.0, 0.0, 3.0, 0.0])
    r = _run({"vectors": x.tolist(), "threshold": 2, "metric": "dot", "max_pairs": 100})
    want = [(2, 3, 5.0), (0, 1, 4.0), (0, 2, 4.0), (0, 3, 4.0), (1, 2, 4.0), (1, 3, 4.0), (0, 4, 2.0), (1, 4, 2.0),
            (2, 4, 2.0), (3, 4, 2.0)]
    assert [(p["i"], p["j"], p["score"]) for p in r["pairs"]] == want and r["pair_count"] == 10
    assert r["group"] == [0, 0, 0, 0, 0, 5] and r["largest_group"] == 5 and r["group_count"] == 1
    r3 = _run({"vectors": x.tolist(), "threshold": 2, "metric": "dot", "max_pairs": 3, "output": "summary"})
    assert [(p["i"], p["j"]) for p in r3["pairs"]] == [(2, 3), (0, 1), (0, 2)] and r3["pair_count"] == 10
    # single linkage: rows 4 and 2 are in one group through the chain, whatever their own score


def test_threshold_is_rounded_once_to_fp32():
    x = torch.zeros((2, 64))
    x[:, 0] = 1.0
    x[0, 1] = x[1, 1] = 2.0 ** -12  # score = 1 + 2^-24 in exact arithmetic, 1.0 in fp32 (ties to even)
    assert ops.sim_join(x, x, 1.0)[1].tolist() == [1.0]
    f32 = lambda v: struct.unpack("<f", struct.pack("<f", v))[0]  # noqa: E731
    for t, hit in ((1.0, True), (1.0 + 2.0 ** -25, True), (1.0 + 2.0 ** -24, True), (1.0 + 2.0 ** -23, False),
                   (1.00000012, False), (0.1, True), (1, True)):
        r = _run({"vectors": x.tolist(), "threshold": t, "metric": "dot", "max_pairs": 1})
        assert r["threshold"] == f32(t) and isinstance(r["threshold"], float), t
        assert r["pair_count"] == (1 if hit else 0), t  # 1 + 2^-24 rounds to 1.0: the pair at 1.0 passes


# ------------------------------------------------------------------------------------------------ errors
def test_every_error_string(tmp_path, monkeypatch):
    from ops.map_dedup import ERRORS

    v = torch.eye(3, 64).tolist()
    cases = [
        ({"threshold": 0.5}, "source"), ({"threshold": 0.5, "vectors": v, "texts": ["a", "b"]}, "source"),
        ({"threshold": 0.5, "texts": "ab"}, "texts"), ({"threshold": 0.5, "texts": ["a", 3]}, "texts"),
        ({"threshold": 0.5, "texts": []}, "rows_empty"),
        ({"threshold": 0.5, "vectors": [[1.0], [1.0, 2.0]]}, "vectors"),
        ({"threshold": 0.5, "vectors": [[1.0, float("nan")], [0.0, 1.0]]}, "vectors"),
        ({"threshold": 0.5, "vectors": []}, "vectors"), ({"threshold": 0.5, "vectors": [[], []]}, "vectors"),
        ({"threshold": 0.5, "vectors": [[1.0, 0.0], [0.0, 1.0]]}, "dim"),
        ({"threshold": 0.5, "vectors": torch.eye(2, 96).tolist()}, "dim"),
        ({"vectors": v}, "threshold"), ({"threshold": None, "vectors": v}, "threshold"),
        ({"threshold": "0.5", "vectors": v}, "threshold"), ({"threshold": True, "vectors": v}, "threshold"),
        ({"threshold": float("nan"), "vectors": v}, "threshold"), ({"threshold": float("inf"), "vectors": v}, "threshold"),
        ({"threshold": 1e39, "vectors": v}, "threshold"),
        ({"threshold": 0.5, "vectors": v, "metric": "l2"}, "metric"),
        ({"threshold": 0.5, "vectors": v, "pooling": "max"}, "pooling"),
        ({"threshold": 0.5, "vectors": v, "max_pairs": -1}, "max_pairs"),
        ({"threshold": 0.5, "vectors": v, "max_pairs": 65537}, "max_pairs"),
        ({"threshold": 0.5, "vectors": v, "max_pairs": 1.0}, "max_pairs"),
        ({"threshold": 0.5, "vectors": v, "output": "base64"}, "output"),
        ({"threshold": 0.5, "vectors": v, "output": "npy"}, "output_uri"),
        ({"threshold": 0.5, "vectors": v, "output": "npy", "output_uri": "s3://b/x.npy"}, "output_uri"),
        ({"threshold": 0.5, "vectors_uri": "http://host/x.npy"}, "corpus_file"),
        ({"threshold": 0.5, "vectors_uri": 5}, "corpus_file"),
        ({"threshold": 0.5, "vectors_uri": str(tmp_path / "missing.npy")}, "corpus_file"),
    ]
    np.save(str(tmp_path / "one_d.npy"), np.zeros(8, dtype=np.float32))
    np.save(str(tmp_path / "empty.npy"), np.zeros((0, 64), dtype=np.float32))
    bad = np.ones((4, 64), dtype=np.float32)
    bad[2, 3] = np.inf
    np.save(str(tmp_path / "inf.npy"), bad)
    np.save(str(tmp_path / "odd.npy"), np.ones((4, 96), dtype=np.float32))
    np.save(str(tmp_path / "ok.npy"), np.eye(4, 64, dtype=np.float32))
    cases += [({"threshold": 0.5, "vectors_uri": str(tmp_path / "one_d.npy")}, "corpus_file"),
              ({"threshold": 0.5, "vectors_uri": str(tmp_path / "empty.npy")}, "corpus_empty"),
              ({"threshold": 0.5, "vectors_uri": str(tmp_path / "inf.npy")}, "corpus_nonfinite"),
              ({"threshold": 0.5, "vectors_uri": str(tmp_path / "odd.npy")}, "dim")]
    for payload, key in cases:
        with pytest.raises(ValueError) as e:
            _run(payload)
        assert str(e.value) == ERRORS[key], (payload, key)
    monkeypatch.setenv("MAP_EMBED_MAX_JSON_VALUES", "3")
    with pytest.raises(ValueError) as e:
        _run({"threshold": 0.5, "vectors_uri": str(tmp_path / "ok.npy")})
    assert str(e.value) == ERRORS["too_large"]
    assert _run({"threshold": 0.5, "vectors_uri": str(tmp_path / "ok.npy"), "output": "summary"})["ok"]
    monkeypatch.setenv("SEARCH_INDEX_MAX_GB", "0.0000001")
    rs.clear_cache()
    with pytest.raises(ValueError) as e:
        _run({"threshold": 0.5, "vectors_uri": str(tmp_path / "ok.npy"), "output": "summary"})
    assert str(e.value) == ERRORS["corpus_too_large"]
    text = open(registry.__file__.replace("__init__.py", "map_dedup.CONTRACT.md")).read()
    for msg in ERRORS.values():
        assert msg in text, msg
    keys = {key for _, key in cases} | {"too_large", "corpus_too_large"}
    assert keys == set(ERRORS), set(ERRORS) - keys
