"""IVF sim_topk (csrc/kernels/sim_topk_ivf.hip): the per-query cluster probe inside the top-k kernel, tested
directly with hand-made labels (not k-means), and map_search with ``index`` on the GPU engine.

The reference is the masked kernel itself. A (query, row) score is one fp32 accumulator fed in a column order
that depends on D alone, and the IVF kernel ranks by the original row id, so "query i over the clusters it
probes" has one right answer: ``ops.sim_topk(q[i:i+1], c, k, mask=label in probes_i)`` on the original-order
corpus, bit for bit. Every comparison below is ``torch.equal`` or list equality; no tolerance is involved. The
data is test_search_gpu.py's integer recipe with duplicated rows, so equal scores occur, and the rows of a
cluster are scattered over the corpus, so the (score desc, id asc) tie order is checked through ``row_ids``.
"""
import numpy as np
import pytest
import torch

from agent_tpu_amd import ops

pytestmark = pytest.mark.gpu

PAD_ID = 2 ** 62
NEG = float("-inf")
_cache = {}

# cluster sizes by corpus size: 0, 1, 31, 32, 33, and clusters that straddle the 32-row steps of the sorted rows
SIZES = {1: [0, 1], 33: [1, 0, 31, 1], 1000: [0, 1, 31, 32, 33, 0, 100, 403, 400]}


def _exact_case(D, N, nq):
    key = ("exact", D, N, nq)
    if key not in _cache:
        gen = torch.Generator().manual_seed(D + 3 * N + 5 * nq)
        col = torch.tensor([1.0, 2.0, -1.0, -2.0])[(torch.arange(D) * 7 + torch.arange(D) // 5) % 4]
        base = torch.randint(-1, 2, (max(1, (N + 2) // 3), D), generator=gen).float() * col
        c = base[torch.randint(0, base.shape[0], (N,), generator=gen)].contiguous()  # duplicated rows: ties
        q = torch.randint(-2, 3, (nq, D), generator=gen).float()
        _cache[key] = (q, c)
    return _cache[key]


def _index(gpu, D, n):
    """(c, labels, centroids, vectors, row_ids, offsets) on the device: the clusters' rows are scattered over
    the corpus by a seeded permutation; the sort is the builder's (stable: ascending original row in a cluster)."""
    key = ("index", D, n)
    if key not in _cache:
        _, c = _exact_case(D, n, 40)
        sizes = SIZES[n]
        K = len(sizes)
        assert sum(sizes) == n
        gen = torch.Generator().manual_seed(7 * n + D)
        labels = torch.empty(n, dtype=torch.int64)
        labels[torch.randperm(n, generator=gen)] = torch.repeat_interleave(torch.arange(K), torch.tensor(sizes))
        cent = torch.randint(-2, 3, (K, D), generator=gen).float()
        order = torch.sort(labels, stable=True).indices
        offsets = torch.zeros(K + 1, dtype=torch.int32)
        offsets[1:] = torch.cumsum(torch.tensor(sizes), 0).to(torch.int32)
        _cache[key] = tuple(t.to(gpu) for t in (c, labels, cent, c[order].contiguous(), order.to(torch.int32), offsets))
    return _cache[key]


def _reference(gpu, D, n, nq, k, nprobe):
    """Query by query: the masked kernel over the original-order corpus (computed once per shape, never changed)."""
    key = ("ref", D, n, nq, k, nprobe)
    if key not in _cache:
        q = _exact_case(D, n, nq)[0].to(gpu)
        c, labels, cent = _index(gpu, D, n)[:3]
        probes = ops.sim_topk(q, cent, nprobe)[1]
        rows = []
        for a in range(nq):
            bits = torch.isin(labels, probes[a])
            if not bool(bits.any()):
                rows.append((torch.empty(0, device=gpu), torch.empty(0, dtype=torch.int64, device=gpu)))
                continue
            s, i = ops.sim_topk(q[a:a + 1].contiguous(), c, k, 1000, mask=ops.row_mask_from_bits(bits))
            rows.append((s[0], i[0]))
        _cache[key] = rows
    return _cache[key]


def _check(got, want, what):
    s, i, n = got
    assert s.dtype == torch.float32 and i.dtype == torch.int64 and s.shape == i.shape and n.shape == (s.shape[0],)
    for a, (ws, wi) in enumerate(want):
        m = ws.numel()
        assert int(n[a]) == m, (what, a, int(n[a]), m)
        assert torch.equal(i[a, :m], wi), (what, a)
        assert torch.equal(s[a, :m], ws), (what, a)
        assert bool((s[a, m:] == NEG).all()) and bool((i[a, m:] == PAD_ID).all()), (what, a)


# every nq and every k, and each nq with a small and a large k: KM 8 / 16 / 32, one item and several per cluster
SHAPES = [(1, 1), (16, 8), (17, 16), (40, 32), (1, 32), (40, 8), (17, 1), (16, 16)]


@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("n", [1, 33, 1000])
def test_each_query_equals_the_masked_search_of_its_probed_clusters(gpu, D, n):
    c, labels, cent, vec, rid, off = _index(gpu, D, n)
    K = cent.shape[0]
    for nq, k in SHAPES:
        q = _exact_case(D, n, nq)[0].to(gpu)
        for nprobe in sorted({1, min(3, K), K}):
            want = _reference(gpu, D, n, nq, k, nprobe)
            for splits in (1, 3):
                got = ops.sim_topk_ivf(q, vec, rid, off, cent, k, nprobe, 1000, splits=splits)
                assert got[0].shape == (nq, k)
                _check(got, want, (D, n, nq, k, nprobe, splits))
            _check(ops.sim_topk_ivf(q, vec, rid, off, cent, k, nprobe, 1000), want, (D, n, nq, k, nprobe, "auto"))


@pytest.mark.parametrize("D", [64, 128])
def test_probing_every_cluster_equals_the_unmasked_kernel(gpu, D):
    n = 1000
    c, labels, cent, vec, rid, off = _index(gpu, D, n)
    K = cent.shape[0]
    for nq, k in SHAPES:
        q = _exact_case(D, n, nq)[0].to(gpu)
        ws, wi = ops.sim_topk(q, c, k, 77)
        for splits in (1, 3):
            s, i, cnt = ops.sim_topk_ivf(q, vec, rid, off, cent, k, K, 77, splits=splits)
            assert torch.equal(i, wi) and torch.equal(s, ws) and cnt.tolist() == [k] * nq, (D, nq, k, splits)
    sc, ic = ws.cpu(), wi.cpu()  # the duplicated rows tie: equal scores come back in ascending id
    same = sc[:, 1:] == sc[:, :-1]
    assert same.any() and (ic[:, 1:][same] > ic[:, :-1][same]).all()


def test_a_query_alone_equals_the_query_inside_a_batch_of_40(gpu):
    D, n, k = 64, 1000, 16
    c, labels, cent, vec, rid, off = _index(gpu, D, n)
    q = _exact_case(D, n, 40)[0].to(gpu)
    for nprobe in (1, 3):
        s, i, cnt = ops.sim_topk_ivf(q, vec, rid, off, cent, k, nprobe)
        for a in (0, 15, 16, 39):
            s1, i1, c1 = ops.sim_topk_ivf(q[a:a + 1].contiguous(), vec, rid, off, cent, k, nprobe)
            assert torch.equal(s1[0], s[a]) and torch.equal(i1[0], i[a]) and int(c1[0]) == int(cnt[a]), (nprobe, a)
        s2, i2, c2 = ops.sim_topk_ivf(q, vec, rid, off, cent, k, nprobe)
        assert torch.equal(s2, s) and torch.equal(i2, i) and torch.equal(c2, cnt)  # a second run


def test_a_nan_row_of_an_unprobed_cluster_in_a_shared_step_cannot_leak(gpu):
    """Clusters 1 .. 4 (1, 31, 32 and 33 rows at sorted rows 0 .. 96) share 32-row steps. Every row outside the
    probed clusters is NaN (and 1e30): by select, never times 0."""
    D, n, k = 64, 1000, 8
    c, labels, cent, vec, rid, off = _index(gpu, D, n)
    q = _exact_case(D, n, 17)[0][:3].contiguous().to(gpu)  # three queries: at most three of the seven clusters with rows
    for target in (2, 3, 4, 7):
        cent2 = cent.clone()
        cent2[target] = 100.0 * q[0]  # query 0 probes the target; the other two probe what they like
        probes = ops.sim_topk(q, cent2, 1)[1]
        assert int(probes[0, 0]) == target
        clean = ops.sim_topk_ivf(q, vec, rid, off, cent2, k, 1, splits=3)
        probed = torch.zeros(cent.shape[0], dtype=torch.bool, device=gpu)
        probed[probes.flatten()] = True
        pos = torch.repeat_interleave(torch.arange(cent.shape[0], device=gpu), (off[1:] - off[:-1]).long())
        assert int((~probed[pos]).sum()) >= 97  # four clusters with rows are not probed: at least 1 + 31 + 32 + 33
        for poison in (float("nan"), 1e30):
            v2 = vec.clone()
            v2[~probed[pos]] = poison
            got = ops.sim_topk_ivf(q, v2, rid, off, cent2, k, 1, splits=3)
            assert all(torch.equal(a, b) for a, b in zip(got, clean)), (target, poison)
            assert bool(torch.isfinite(got[0][got[1] != PAD_ID]).all())


@pytest.mark.parametrize("n", [1, 33, 1000])
def test_nothing_outside_the_index_is_read(gpu, n):
    """``vectors``, ``row_ids`` and ``offsets`` each as a view inside a larger poisoned buffer."""
    D, k, pad = 64, 8, 64
    c, labels, cent, vec, rid, off = _index(gpu, D, n)
    K = cent.shape[0]
    q = _exact_case(D, n, 17)[0].to(gpu)

    def inside(t, poison):
        big = torch.full((t.shape[0] + 2 * pad,) + tuple(t.shape[1:]), poison, dtype=t.dtype, device=gpu)
        big[pad:pad + t.shape[0]] = t
        view = big[pad:pad + t.shape[0]]
        assert view.is_contiguous()
        return view

    for nprobe in sorted({1, K}):
        clean = ops.sim_topk_ivf(q, vec, rid, off, cent, k, nprobe, splits=3)
        for poison in (float("nan"), 1e30):
            got = ops.sim_topk_ivf(q, inside(vec, poison), inside(rid, 5), inside(off, n), cent, k, nprobe, splits=3)
            assert all(torch.equal(a, b) for a, b in zip(got, clean)), (n, nprobe, poison)


@pytest.mark.parametrize("nq,nprobe,K", [(1, 1, 1), (1, 3, 7), (17, 3, 7), (40, 7, 7), (40, 1, 7), (256, 32, 1024),
                                         (300, 32, 4096), (5000, 2, 3)])
def test_plan_kernel_puts_every_pair_into_exactly_one_item_of_one_cluster(gpu, nq, nprobe, K):
    gen = torch.Generator().manual_seed(nq + nprobe + K)
    probes = torch.rand(nq, K, generator=gen).argsort(1)[:, :nprobe].contiguous()  # distinct clusters per query
    if (nq, nprobe) == (40, 1):
        probes[:] = 4  # forty queries of one cluster: three items
    bound = min(nq * nprobe, K) + nq * nprobe // 16
    cl, iq, sl = (t.cpu() for t in ops.ivf_plan(probes.to(gpu), K, bound))
    assert cl.shape == (bound,) and iq.shape == sl.shape == (bound, 16) and cl.dtype == iq.dtype == sl.dtype == torch.int32
    real, valid = cl >= 0, sl >= 0
    assert not bool(valid[~real].any()) and bool(valid[real][:, 0].all())  # slot 0 of an item is a pair
    pairs = iq[valid].long() * nprobe + sl[valid].long()
    assert torch.equal(pairs.sort().values, torch.arange(nq * nprobe))  # every pair exactly once
    assert torch.equal(probes.flatten()[pairs], cl[:, None].expand(-1, 16)[valid].long())  # in an item of its cluster
    assert bool(((iq >= 0) & (iq < nq)).all()) and bool((sl < nprobe).all())
    assert torch.equal(torch.where(valid, iq, iq[:, :1])[real], iq[real])  # padding repeats the item's first query
    counts = torch.bincount(probes.flatten(), minlength=K)
    assert int(real.sum()) == int(((counts + 15) // 16).sum())
    twin = ops.ivf_plan(probes, K, bound)  # the PyTorch twin: the same items up to the order inside a cluster
    assert torch.equal(twin[0], cl) and torch.equal((twin[2] >= 0).sum(1), valid.sum(1))


def test_self_hit_on_a_kmeans_built_index(gpu):
    """Distinct random unit rows, the index built by k-means: with ``nprobe = 1`` a stored row used as a query
    probes its own cluster (its label is ``sim_topk(x, centroids, 1)`` bit for bit) and finds itself first."""
    from agent_tpu_amd.runtime import ivf
    from agent_tpu_amd.runtime.search import normalize_rows

    N, D, K = 600, 64, 8
    x = normalize_rows(torch.randn(N, D, generator=torch.Generator().manual_seed(5))).contiguous().to(gpu)
    vec, rid, off, cent, iters, _ = ivf.build(x, K, 10)
    assert vec.shape == (N, D) and off.tolist()[-1] == N and 1 <= iters <= 10
    assert torch.equal(ops.ivf_labels(rid, off), ops.sim_topk(x, cent, 1)[1][:, 0])
    assert torch.equal(vec, x[rid.long()])
    s, i, cnt = ops.sim_topk_ivf(x, vec, rid, off, cent, 4, 1)
    assert i[:, 0].tolist() == list(range(N))
    assert bool((cnt >= 1).all())


def test_rejections(gpu):
    c, labels, cent, vec, rid, off = _index(gpu, 64, 33)
    q = _exact_case(64, 33, 17)[0].to(gpu)
    ops.sim_topk_ivf(q, vec, rid, off, cent, 4, 2)
    K = cent.shape[0]
    for bad in (lambda: ops.sim_topk_ivf(q, vec, rid, off, cent, 4, K + 1), lambda: ops.sim_topk_ivf(q, vec, rid, off, cent, 4, 0),
                lambda: ops.sim_topk_ivf(q, vec, rid, off, cent, 33, 1), lambda: ops.sim_topk_ivf(q, vec, rid.long(), off, cent, 4, 1),
                lambda: ops.sim_topk_ivf(q, vec, rid.cpu(), off, cent, 4, 1), lambda: ops.sim_topk_ivf(q, vec, rid, off[:-1], cent, 4, 1),
                lambda: ops.sim_topk_ivf(q, vec.half(), rid, off, cent, 4, 1), lambda: ops.sim_topk_ivf(q, vec, rid, off, cent, 4, 2, splits=129),
                lambda: ops.sim_topk_ivf(q[:, :32].contiguous(), vec[:, :32].contiguous(), rid, off, cent[:, :32].contiguous(), 4, 1)):
        with pytest.raises(ValueError):
            bad()


# -------------------------------------------------------------------------------------------- the op
def test_map_search_with_an_index_on_the_gpu_engine(gpu, tmp_path, monkeypatch):
    """Rows of sixteen +-1 entries (normalised: +-0.25 exactly). ``nprobe == clusters`` equals the job without
    ``index``; ``nprobe = 2`` equals the masked ``sim_topk`` built from the index's own labels; a second call
    finds the entry in the LRU."""
    from agent_tpu_amd.runtime import ivf
    from agent_tpu_amd.runtime import search as rs
    from ops.map_search import map_search

    monkeypatch.delenv("CLASSIFY_DEVICE", raising=False)
    monkeypatch.delenv("SEARCH_INDEX_DTYPE", raising=False)
    rs.clear_cache()
    N, D, K = 300, 64, 6
    gen = torch.Generator().manual_seed(21)
    c = torch.zeros(N, D)
    for r in range(N):
        c[r, torch.randperm(D, generator=gen)[:16]] = torch.randint(0, 2, (16,), generator=gen).float() * 2 - 1
    c[7], c[140], c[299] = c[3], c[3], c[3]
    q = torch.cat([c[3:4], c[100:108]])
    path = str(tmp_path / "corpus.npy")
    np.save(path, c.numpy())
    job = {"query_vectors": q.tolist(), "corpus_uri": path, "top_k": 32}
    try:
        plain = map_search(dict(job))
        full = map_search(dict(job, index={"type": "ivf", "clusters": K, "nprobe": K, "train_iterations": 5}))
        assert full["ids"] == plain["ids"] and full["scores"] == plain["scores"]
        assert plain["ids"][0][:4] == [3, 7, 140, 299] and full["index_cached"] is False
        assert set(full) == set(plain) | {"index"} and full["index"]["clusters"] == K
        two = map_search(dict(job, index={"type": "ivf", "clusters": K, "nprobe": 2, "train_iterations": 5}))
        assert two["index_cached"] is True and two["index"]["nprobe"] == 2
        idx = ivf.load_index(path, 0, -1, gpu, K, 5)
        assert idx.cached and idx.vectors.is_cuda
        x = rs.normalize_rows(c.to(gpu))
        labels = ops.ivf_labels(idx.row_ids, idx.offsets)
        assert torch.equal(labels, ops.sim_topk(x, idx.centroids, 1)[1][:, 0])
        qn = rs.normalize_rows(q.to(gpu))
        probes = ops.sim_topk(qn, idx.centroids, 2)[1]
        for a in range(q.shape[0]):
            ws, wi = ops.sim_topk(qn[a:a + 1].contiguous(), x, 32, mask=ops.row_mask_from_bits(torch.isin(labels, probes[a])))
            assert two["ids"][a] == wi[0].tolist() and two["scores"][a] == ws[0].tolist(), a
        assert rs.cache_info()["resident_bytes"] == 2 * N * D * 4 + N * 4 + (K + 1) * 4 + K * D * 4
    finally:
        rs.clear_cache()
