"""The near-duplicate kernels (csrc/kernels/sim_join.hip) against their oracles, and the map_dedup op on the GPU.

Every comparison is exact. sim_join on small-integer data must equal an int64 matmul reference (every product and
partial sum is exact in fp32 in any order); on random fp32 data every emitted score must have the bits that
``sim_topk`` reports for that (query, row), and the emitted set must be ``{score >= t, I < J}`` of those scores.
The list's order is arbitrary, so it is compared sorted. cc_min_labels must equal a host union-find.
"""
import math

import numpy as np
import pytest
import torch

from agent_tpu_amd import ops
from agent_tpu_amd.runtime import dedup as rd

pytestmark = pytest.mark.gpu

_cache = {}


def _ints(D):
    """97 rows of {-2..2}; rows 3, 7 and 40 are identical."""
    if D not in _cache:
        gen = torch.Generator().manual_seed(100 + D)
        z = torch.randint(-2, 3, (97, D), generator=gen).float()
        z[7] = z[3]
        z[40] = z[3]
        _cache[D] = z.contiguous()
    return _cache[D]


def _got(pairs, scores, count):
    n = int(count.item())
    assert n <= pairs.shape[0]
    p, s = ops.sort_pairs(pairs[:n], scores[:n])
    return p.cpu(), s.cpu()


def _want(S, t, x_base, y_base):
    """Sorted pairs and scores of the score matrix ``S`` (any dtype that compares exactly with ``t``)."""
    I = torch.arange(S.shape[0])[:, None] + x_base
    J = torch.arange(S.shape[1])[None, :] + y_base
    hit = (S >= t) & (I < J)
    ij = hit.nonzero()
    return torch.stack([ij[:, 0] + x_base, ij[:, 1] + y_base], 1).to(torch.int32), S[hit]


@pytest.mark.parametrize("D", [64, 768, 1024])
@pytest.mark.parametrize("Ny", [1, 31, 33, 97])
@pytest.mark.parametrize("Nx", [1, 31, 33, 97])
def test_join_equals_the_int64_reference_on_exact_data(gpu, Nx, Ny, D):
    z = _ints(D)
    # (0, 0) is the self-join of a prefix; the other bases move the diagonal through the 32-row tiles and steps;
    # (0, 97) is a rectangle: every pair is live
    for x_base, y_base in ((0, 0), (5, 0), (0, 7), (40, 30), (0, 97)):
        x, y = z[:Nx].contiguous(), z[97 - Ny:].contiguous() if y_base == 30 else z[:Ny].contiguous()
        S = x.long() @ y.long().T
        I = torch.arange(Nx)[:, None] + x_base
        J = torch.arange(Ny)[None, :] + y_base
        live = S[I < J]
        if live.numel() == 0:
            t = 0
        else:
            t = int(live.sort().values[live.numel() // 2])  # an attained score: >= differs from > here
        wp, ws = _want(S, t, x_base, y_base)
        pairs, scores, count = ops.sim_join(x.to(gpu), y.to(gpu), float(t), x_base, y_base, cap=Nx * Ny)
        assert pairs.dtype == torch.int32 and scores.dtype == torch.float32 and count.dtype == torch.int64
        assert int(count.item()) == wp.shape[0], (x_base, y_base)
        gp, gs = _got(pairs, scores, count)
        assert torch.equal(gp, wp), (x_base, y_base)
        assert torch.equal(gs.double(), ws.double()), (x_base, y_base)
        assert not bool((gp[:, 0] >= gp[:, 1]).any())  # no (i, i), and the lower id first
        if live.numel():
            assert int((live == t).sum()) >= 1 and int(count.item()) >= int((live == t).sum())
        if (x_base, y_base) == (0, 0) and Nx >= 41 and Ny >= 41:  # identical rows pair with each other
            have = {tuple(p) for p in gp.tolist()}
            top = int(S[3, 3])
            if top >= t:
                assert {(3, 7), (3, 40), (7, 40)} <= have


def _topk_scores(x, y):
    """[Nx, Ny] scores as ``sim_topk`` reports them: y in blocks of 32 rows with k = 32 returns every score."""
    S = torch.empty((x.shape[0], y.shape[0]), dtype=torch.float32, device=x.device)
    for b in range(0, y.shape[0], 32):
        blk = y[b:b + 32].contiguous()
        s, i = ops.sim_topk(x, blk, 32)
        S[:, b:b + blk.shape[0]].scatter_(1, i, s)
    return S


def test_scores_have_the_bits_of_sim_topk(gpu):
    gen = torch.Generator().manual_seed(5)
    y = torch.randn(200, 768, generator=gen)
    y[150] = y[70]
    y = torch.nn.functional.normalize(y, dim=1).contiguous().to(gpu)
    x_base = 64
    x = y[x_base:x_base + 70].contiguous()  # a block of the self-join: the diagonal crosses its tiles
    S = _topk_scores(x, y).cpu()
    I = torch.arange(70)[:, None] + x_base
    J = torch.arange(200)[None, :]
    live = S[I < J].sort(descending=True).values
    for t in (float(live[200]), float(live[0]), 2.0, -2.0):  # attained scores, nothing, everything
        wp, ws = _want(S, torch.tensor(t, dtype=torch.float32), x_base, 0)
        gp, gs = _got(*ops.sim_join(x, y, t, x_base, 0, cap=70 * 200))
        assert torch.equal(gp, wp), t
        assert torch.equal(gs.view(torch.int32), ws.contiguous().view(torch.int32)), t
    assert (x_base + 6, 150) in {tuple(p) for p in gp.tolist()}


@pytest.fixture(scope="module")
def wide(gpu):
    """100 x 2100 at D = 64: four row tiles, 66 column steps (several panels at ``panel_rows`` 32 and 96, whose
    last panel is partial), about 2000 pairs."""
    gen = torch.Generator().manual_seed(11)
    y = torch.randint(-2, 3, (2100, 64), generator=gen).float().contiguous()
    x = y[1000:1100].contiguous()
    S = x.long() @ y.long().T
    I = torch.arange(100)[:, None] + 1000
    live = S[I < torch.arange(2100)[None, :]].sort(descending=True).values
    t = int(live[2000])
    wp, ws = _want(S, t, 1000, 0)
    return x.to(gpu), y.to(gpu), float(t), wp, ws.float()


def test_launch_shape_does_not_change_the_set(gpu, wide):
    x, y, t, wp, ws = wide
    for max_wgs in (1, 3, 0):
        for panel_rows in (0, 32, 96, 1024):
            gp, gs = _got(*ops.sim_join(x, y, t, 1000, 0, cap=4096, max_wgs=max_wgs, panel_rows=panel_rows))
            assert torch.equal(gp, wp) and torch.equal(gs, ws), (max_wgs, panel_rows)


def test_overflow_counts_everything_and_writes_nothing_past_cap(gpu, wide):
    x, y, t, wp, ws = wide
    total = wp.shape[0]
    full = {tuple(p): s for p, s in zip(wp.tolist(), ws.tolist())}
    for cap in (total // 2, 1, 0):
        pbuf = torch.full((cap + 64, 2), -7, dtype=torch.int32, device=gpu)
        sbuf = torch.full((cap + 64,), -7.0, dtype=torch.float32, device=gpu)
        pairs, scores, count = ops.sim_join(x, y, t, 1000, 0, cap=cap, out=(pbuf[:cap], sbuf[:cap]))
        assert int(count.item()) == total
        assert bool((pbuf[cap:] == -7).all()) and bool((sbuf[cap:] == -7.0).all())  # the canaries
        got = [tuple(p) for p in pairs.cpu().tolist()]
        assert len(set(got)) == cap and all(full[p] == s for p, s in zip(got, scores.cpu().tolist()))
    gp, gs = _got(*ops.sim_join(x, y, t, 1000, 0, cap=total))  # the rerun with cap = count
    assert torch.equal(gp, wp) and torch.equal(gs, ws)


def test_near_duplicates_blocks_and_the_cap_rerun(gpu, wide, monkeypatch):
    _, y, t, _, _ = wide
    want = rd.near_duplicates(y, t)
    S = (y.cpu().long() @ y.cpu().long().T)
    wp, ws = _want(S, int(t), 0, 0)
    assert torch.equal(want.pairs.cpu(), wp) and torch.equal(want.scores.cpu(), ws.float())
    monkeypatch.setattr(rd, "MIN_CAP", 8)  # blocks of 64 rows: cap = 256 < their counts
    for block_rows, max_wgs in ((64, 0), (1000, 3)):
        got = rd.near_duplicates(y, t, block_rows=block_rows, max_wgs=max_wgs)
        assert torch.equal(got.pairs, want.pairs) and torch.equal(got.scores, want.scores)
        assert torch.equal(got.labels, want.labels)
    assert want.labels.cpu().tolist() == _union_find(wp.tolist(), 2100)


# ------------------------------------------------------------------------------------ connected components
def _union_find(edges, N):
    parent = list(range(N))

    def find(a):
        while parent[a] != a:
            parent[a] = parent[parent[a]]
            a = parent[a]
        return a

    for u, v in edges:
        ru, rv = find(u), find(v)
        if ru != rv:
            parent[max(ru, rv)] = min(ru, rv)
    return [find(v) for v in range(N)]  # roots are component minima: the smaller root always wins


def _labels(edges, N, gpu):
    pairs = torch.tensor(edges, dtype=torch.int32).reshape(-1, 2).to(gpu)
    labels, rounds = ops.cc_min_labels(pairs, N, with_rounds=True)
    assert labels.dtype == torch.int32 and labels.shape == (N,)
    return labels.cpu().tolist(), rounds


def test_cc_path_in_any_edge_order_finishes_in_few_rounds(gpu):
    N = 1000
    asc = [(i, i + 1) for i in range(N - 1)]
    gen = torch.Generator().manual_seed(3)
    shuffled = [asc[i] if i % 2 else asc[i][::-1] for i in torch.randperm(N - 1, generator=gen).tolist()]
    # Trees of a path are segments with at most two neighbours. In a round every tree with a lower-rooted
    # neighbour is hooked away, and a surviving tree claims at most its two hooked neighbours, each shared by
    # at most two survivors: the trees shrink by a third per round. ceil(log_1.5 N) rounds and a last one
    # that changes nothing, plus one of slack for the rounding of the tree counts.
    bound = math.ceil(math.log(N) / math.log(1.5)) + 2
    for edges in (asc, asc[::-1], shuffled):
        labels, rounds = _labels(edges, N, gpu)
        assert labels == [0] * N
        assert rounds <= bound, (rounds, bound)
        want, wr = ops.cc_min_labels_ref(torch.tensor(edges, dtype=torch.int32), N, with_rounds=True)
        assert want.tolist() == labels and wr <= bound


def test_cc_small_graphs(gpu):
    star = [(5, v) for v in range(20) if v != 5]
    assert _labels(star, 20, gpu)[0] == [0] * 20
    two = [(0, 4), (4, 2), (7, 9), (9, 8), (8, 7), (2, 0), (0, 4), (0, 4)]  # a cycle and duplicate edges
    assert _labels(two, 12, gpu)[0] == [0, 1, 0, 3, 0, 5, 6, 7, 7, 7, 10, 11]
    labels, rounds = _labels([], 9, gpu)
    assert labels == list(range(9)) and rounds == 0
    assert _labels([(0, 0)], 1, gpu)[0] == [0]
    with pytest.raises(ValueError):
        _labels([(0, 12)], 12, gpu)


def test_cc_random_graph_equals_union_find(gpu):
    gen = torch.Generator().manual_seed(8)
    N, E = 2000, 3000
    edges = torch.randint(0, N, (E, 2), generator=gen).tolist()
    labels, rounds = _labels(edges, N, gpu)
    assert labels == _union_find(edges, N) and rounds <= N
    assert ops.cc_min_labels_ref(torch.tensor(edges, dtype=torch.int32), N).tolist() == labels


# ------------------------------------------------------------------------------------------------------ op
def _planted(N, D, seed):
    """Integer rows: rows 3k + 1 and 3k + 2 (k < 20) copy row 3k, the second with one coordinate zeroed."""
    gen = torch.Generator().manual_seed(seed)
    x = torch.randint(-2, 3, (N, D), generator=gen).float()
    group = list(range(N))
    for k in range(20):
        a = 3 * k
        x[a + 1] = x[a]
        x[a + 2] = x[a]
        x[a + 2, k] = 0.0
        group[a + 1] = group[a + 2] = a
    return x, group


def test_map_dedup_op_equals_the_cpu_path_key_for_key(gpu, tmp_path, monkeypatch):
    from ops.map_dedup import map_dedup

    monkeypatch.delenv("CLASSIFY_DEVICE", raising=False)
    N, D = 300, 64
    x, group = _planted(N, D, 21)
    S = x.long() @ x.long().T
    planted = torch.tensor(group)[:, None] == torch.tensor(group)[None, :]
    off = ~torch.eye(N, dtype=torch.bool)
    t = int(S[planted & off].min())
    assert int(S[~planted].max()) < t  # the data separate the planted groups
    path = str(tmp_path / "vec.npy")
    np.save(path, x.numpy())
    out = str(tmp_path / "out.npy")
    jobs = [{"vectors_uri": path, "threshold": t, "metric": "dot", "max_pairs": 50},
            {"vectors_uri": path, "threshold": 0.9, "max_pairs": 0},
            {"vectors": x[:100].tolist(), "threshold": t, "metric": "dot", "output": "summary", "max_pairs": 7}]
    for job in jobs:
        r = map_dedup(dict(job))
        monkeypatch.setenv("CLASSIFY_DEVICE", "cpu")
        h = map_dedup(dict(job))
        monkeypatch.delenv("CLASSIFY_DEVICE")
        assert set(r) == set(h)
        for key in set(r) - {"elapsed_ms", "rows_per_sec", "index_cached"}:
            assert r[key] == h[key], key
        assert r["ok"] and r["op"] == "map_dedup" and r["dim"] == D and r["dp_world_size"] == 1
        if "group" in r:
            assert r["group"] == group and r["keep"] == [i for i in range(N) if group[i] == i]
            assert r["pair_count"] == 60 and r["group_count"] == 20 and r["duplicate_count"] == 40
            assert r["kept_count"] == N - 40 and r["largest_group"] == 3
    r = map_dedup({"vectors_uri": path, "threshold": 0.9, "output": "npy", "output_uri": out})
    assert r["index_cached"] is True and "group" not in r and np.load(r["group_uri"]).tolist() == group
    texts = ["the quick brown fox", "completely different words here", "the quick brown fox", "zebra", None,
             "completely different words here", "", "the quick brown fox"]
    r = map_dedup({"texts": texts, "threshold": 0.9999, "model_path": "bert-tiny?batch=8&seq=32&seed=4"})
    assert r["group"] == [0, 1, 0, 3, 4, 1, 4, 0] and r["keep"] == [0, 1, 3, 4] and r["largest_group"] == 3
    monkeypatch.setenv("CLASSIFY_DEVICE", "cpu")
    h = map_dedup({"texts": texts, "threshold": 0.9999, "model_path": "bert-tiny?batch=8&seq=32&seed=4"})
    for key in ("group", "keep", "pair_count", "group_count", "duplicate_count", "kept_count", "largest_group", "dim"):
        assert r[key] == h[key], key
