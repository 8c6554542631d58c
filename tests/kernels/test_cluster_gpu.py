"""The k-means kernels (csrc/kernels/kmeans.hip) against their oracles, the loop against its CPU twin, and the
map_cluster op on the GPU.

kmeans_assign without a bias must equal ``sim_topk(x, c, 1)`` bit for bit (the same fp32 accumulator in the same
column order). With a bias the data are small integers: every product, partial sum and the bias add are exact
in fp32 in any order, so the labels and scores must equal the fp32 PyTorch reference exactly. kmeans_update and
kmeans_finalize must equal their int64 / fp64 twins exactly: integer sums are order-free and every fp64
operation rounds once.
"""
import numpy as np
import pytest
import torch

from agent_tpu_amd import ops
from agent_tpu_amd.runtime import cluster as rc

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
CHUNK = 64  # kKmChunk: rows of one label per workgroup pass of kmeans_update
_cache = {}


def _random_case(N, K, D):
    key = (N, K, D)
    if key not in _cache:
        gen = torch.Generator().manual_seed(7 * N + 3 * K + D)
        x = torch.randn(N, D, generator=gen)
        c = torch.randn(K, D, generator=gen)
        if K >= 2:  # duplicated centroids: exact ties, the lower id must win
            c[K - 1] = c[0]
        if K >= 17:
            c[5] = c[11]
        if N >= 31:  # +-0.0 scores: a zero row scores +0.0 or -0.0 against every centroid
            x[3] = 0.0
            x[4] = -0.0
        _cache[key] = (x.contiguous(), c.contiguous())
    return _cache[key]


@pytest.mark.parametrize("D", [64, 128, 768])
@pytest.mark.parametrize("K", [1, 2, 17, 33, 257])
@pytest.mark.parametrize("N", [1, 31, 33, 1000])
def test_assign_equals_sim_topk_bit_for_bit(gpu, N, K, D):
    x, c = _random_case(N, K, D)
    dx, dc = x.to(gpu), c.to(gpu)
    s, i = ops.sim_topk(dx, dc, 1)
    prev = torch.zeros((N,), dtype=torch.int32, device=gpu)
    labels, best, changed = ops.kmeans_assign(dx, dc, None, prev)
    assert labels.dtype == torch.int32 and best.dtype == torch.float32 and changed.dtype == torch.int64
    assert torch.equal(labels.long(), i[:, 0]), (labels.long() != i[:, 0]).nonzero()[:4]
    assert torch.equal(best.view(torch.int32), s[:, 0].contiguous().view(torch.int32))
    assert int(changed.item()) == int((labels != prev).sum().item())
    if K >= 2 and N >= 31:
        assert int(labels[3].item()) == 0 and int(labels[4].item()) == 0  # every centroid ties at +-0.0
        assert not bool((labels == K - 1).any())  # the duplicate of centroid 0 never wins


def _int_case(N, K, D, seed):
    gen = torch.Generator().manual_seed(seed)
    x = torch.randint(-2, 3, (N, D), generator=gen).float()
    c = torch.randint(-2, 3, (K, D), generator=gen).float()
    bias = torch.randint(-8, 9, (K,), generator=gen).float() * 0.5
    return x, c, bias


@pytest.mark.parametrize("N,K,D", [(33, 17, 64), (1000, 33, 128), (257, 257, 768), (100, 65, 1024)])
def test_assign_with_bias_equals_the_fp32_reference_on_exact_data(gpu, N, K, D):
    x, c, bias = _int_case(N, K, D, N + K + D)
    wl, wb, _ = ops.kmeans_assign_ref(x, c, bias)
    labels, best, changed = ops.kmeans_assign(x.to(gpu), c.to(gpu), bias.to(gpu))
    assert torch.equal(labels.cpu(), wl) and torch.equal(best.cpu(), wb)
    assert int(changed.item()) == N  # no previous labels: every row counts
    # l2 form: the arg-max of x.c - 0.5 ||c||^2 is the nearest centroid (integers: exact distances)
    l2b = -0.5 * (c * c).sum(1)
    labels, best, _ = ops.kmeans_assign(x.to(gpu), c.to(gpu), l2b.to(gpu))
    d2 = torch.cdist(x.double(), c.double()) ** 2
    near = torch.where(d2 == d2.min(1, keepdim=True).values, torch.arange(K).expand(N, K), K).min(1).values
    assert torch.equal(labels.cpu().long(), near)


def test_assign_bits_do_not_depend_on_position_batch_or_launch_shape(gpu):
    N, K, D = 1000, 257, 768
    x, c = _random_case(N, K, D)
    bias = torch.linspace(-1, 1, K)
    dx, dc, db = x.to(gpu), c.to(gpu), bias.to(gpu)
    l0, b0, _ = ops.kmeans_assign(dx, dc, db)
    for wgs in (1, 3, 7):
        l, b, _ = ops.kmeans_assign(dx, dc, db, max_wgs=wgs)
        assert torch.equal(l, l0) and torch.equal(b.view(torch.int32), b0.view(torch.int32)), wgs
    perm = torch.randperm(N, generator=torch.Generator().manual_seed(1)).to(gpu)
    l, b, _ = ops.kmeans_assign(dx[perm].contiguous(), dc, db)
    assert torch.equal(l, l0[perm]) and torch.equal(b.view(torch.int32), b0[perm].contiguous().view(torch.int32))
    for lo, hi in ((0, 517), (517, N)):  # the batch cut in two
        l, b, _ = ops.kmeans_assign(dx[lo:hi].contiguous(), dc, db)
        assert torch.equal(l, l0[lo:hi]) and torch.equal(b.view(torch.int32), b0[lo:hi].contiguous().view(torch.int32))
    # few centroids take the 16-row kernel: the same bits as the 32-row kernel gives for those centroids
    l16, b16, _ = ops.kmeans_assign(dx, dc[:33].contiguous(), None)
    s, i = ops.sim_topk(dx, dc[:33].contiguous(), 1)
    assert torch.equal(l16.long(), i[:, 0]) and torch.equal(b16, s[:, 0])
    prev = l0.clone()
    prev[::3] = (prev[::3] + 1) % K
    _, _, ch = ops.kmeans_assign(dx, dc, db, prev)
    assert int(ch.item()) == int((l0 != prev).sum().item()) == len(range(0, N, 3))


def test_nothing_outside_the_tensors_is_read(gpu):
    N, K, D, pad = 33, 17, 128, 64
    x, c = _random_case(N, K, D)
    l0, b0, _ = ops.kmeans_assign(x.to(gpu), c.to(gpu), None)
    for poison in (1e30, float("nan")):
        bx = torch.full((N + 2 * pad, D), poison, device=gpu)
        bc = torch.full((K + 2 * pad, D), poison, device=gpu)
        bx[pad:pad + N] = x.to(gpu)
        bc[pad:pad + K] = c.to(gpu)
        l, b, _ = ops.kmeans_assign(bx[pad:pad + N], bc[pad:pad + K], None)
        assert torch.equal(l, l0) and torch.equal(b, b0)


def _update_case(N, K, D, seed):
    gen = torch.Generator().manual_seed(seed)
    x = 0.5 * torch.randn(N, D, generator=gen)  # |x| < 4 everywhere else
    x[0, 0] = 4.0  # absmax, an exact power of two
    x[N // 2, D - 1] = -4.0
    x[N - 1, 1] = 2.0 ** -30
    labels = torch.randint(0, K, (N,), generator=gen).to(torch.int32)
    return x.contiguous(), labels


@pytest.mark.parametrize("N,K,D", [(CHUNK - 1, 3, 64), (CHUNK + 1, 3, 768), (1000, 17, 128), (4 * CHUNK + 1, 1, 1024),
                                   (5000, 4096, 64)])
def test_update_equals_the_int64_twin(gpu, N, K, D):
    x, labels = _update_case(N, K, D, N + K)
    if K == 3:
        labels[:] = 1  # one cluster holds every row (one below / one above the chunk), the others none
    if K == 17:
        labels[labels == 5] = 6  # a cluster with no member
    s = ops.fixed_shift(N, float(x.abs().max()))
    assert s == 62 - (N - 1).bit_length() - 2
    ws, wc = ops.kmeans_update_ref(x, labels, K, s)
    sums, counts = ops.kmeans_update(x.to(gpu), labels.to(gpu), K, s)
    assert sums.dtype == counts.dtype == torch.int64
    assert torch.equal(counts.cpu(), wc) and int(wc.sum()) == N
    assert torch.equal(sums.cpu(), ws), (sums.cpu() != ws).nonzero()[:4]
    if K == 17:
        assert int(counts[5].item()) == 0 and not bool(sums[5].any())


def test_update_rounds_halves_to_even_and_fixed_sum_is_order_free(gpu):
    # at shift 1 the values k + 0.25 and -(k + 0.25) are exact halves after scaling: ties go to even
    D, K = 64, 2
    v = torch.tensor([0.25, 0.75, 1.25, -0.25, -0.75, -1.25, 2.0 ** -30, 0.0])
    x = torch.zeros((8, D))
    x[:, 0] = v
    x[:, 63] = -v
    labels = torch.tensor([0, 0, 0, 1, 1, 1, 0, 1], dtype=torch.int32)
    sums, counts = ops.kmeans_update(x.to(gpu), labels.to(gpu), K, 1)
    assert sums[:, 0].tolist() == [0 + 2 + 2 + 0, -0 - 2 - 2 + 0] and counts.tolist() == [4, 4]
    assert sums[:, 63].tolist() == [-4, 4]
    ws, _ = ops.kmeans_update_ref(x, labels, K, 1)
    assert torch.equal(sums.cpu(), ws)
    big = torch.randn(100003, generator=torch.Generator().manual_seed(3))
    s = ops.fixed_shift(big.numel(), float(big.abs().max()))
    want = ops.fixed_sum_ref(big, s)
    got = ops.fixed_sum(big.to(gpu), s)
    got_rev = ops.fixed_sum(big.flip(0).contiguous().to(gpu), s)
    assert torch.equal(got.cpu(), want) and torch.equal(got_rev.cpu(), want)
    assert abs(float(want) / 2.0 ** s - float(big.double().sum())) < 1e-6


@pytest.mark.parametrize("metric", ["cosine", "l2"])
def test_finalize_equals_the_fp64_twin(gpu, metric):
    N, K, D = 1000, 17, 768
    x, labels = _update_case(N, K, D, 11)
    labels[labels == 5] = 6  # cluster 5 is empty and keeps its old centroid
    s = ops.fixed_shift(N, float(x.abs().max()))
    sums, counts = ops.kmeans_update_ref(x, labels, K, s)
    old = torch.randn(K, D, generator=torch.Generator().manual_seed(2))
    wc, wb = ops.kmeans_finalize_ref(sums, counts, old, s, metric)
    c, b = ops.kmeans_finalize(sums.to(gpu), counts.to(gpu), old.to(gpu), s, metric)
    assert torch.equal(c.cpu().view(torch.int32), wc.view(torch.int32))
    assert torch.equal(c[5].cpu(), old[5])
    if metric == "l2":
        assert torch.equal(b.cpu().view(torch.int32), wb.view(torch.int32))
        mean = torch.stack([x[labels == k].double().mean(0) for k in range(K) if k != 5])
        assert (c.cpu()[[k for k in range(K) if k != 5]].double() - mean).abs().max() < 1e-6
    else:
        assert b is None and wb is None
        assert (c.cpu()[0].double().norm() - 1.0).abs() < 1e-6


def _blobs(N, K, D, seed):
    """Well-separated integer blobs: centre k is 40 on its own block of columns, the noise is in {-1, 0, 1}."""
    gen = torch.Generator().manual_seed(seed)
    centres = torch.zeros((K, D))
    w = D // K
    for k in range(K):
        centres[k, k * w:(k + 1) * w] = 40.0
    planted = torch.randint(0, K, (N,), generator=gen)
    x = centres[planted] + torch.randint(-1, 2, (N, D), generator=gen).float()
    return x.contiguous(), planted


@pytest.mark.parametrize("metric", ["cosine", "l2"])
@pytest.mark.parametrize("D", [64, 768])
def test_loop_equals_the_cpu_twin(gpu, D, metric):
    from agent_tpu_amd.runtime.search import normalize_rows

    N, K = 1000, 5
    x, planted = _blobs(N, K, D, D)
    xs = normalize_rows(x).contiguous() if metric == "cosine" else x
    init = torch.stack([xs[int((planted == k).nonzero()[0, 0])] for k in range(K)])  # one row of every blob
    want = rc.kmeans(xs, K, metric, max_iter=20, init=init)
    got = rc.kmeans(xs.to(gpu), K, metric, max_iter=20, init=init)
    assert want.converged and got.converged and got.iterations == want.iterations and got.changed_last == 0
    assert torch.equal(got.labels.cpu(), want.labels) and torch.equal(got.sizes.cpu(), want.sizes)
    assert torch.equal(got.centroids.cpu().view(torch.int32), want.centroids.view(torch.int32))
    assert torch.equal(want.labels.long(), planted)  # the planted partition, named by the initial rows
    if D == 64:  # the seeded start (rows 'sorted(randperm(N, seed)[:K])'): the same bits as well
        ws_, gs_ = rc.kmeans(xs, K, metric, seed=3, max_iter=20), rc.kmeans(xs.to(gpu), K, metric, seed=3, max_iter=20)
        assert gs_.iterations == ws_.iterations and torch.equal(gs_.labels.cpu(), ws_.labels)
        assert torch.equal(gs_.centroids.cpu().view(torch.int32), ws_.centroids.view(torch.int32))
        assert gs_.objective == pytest.approx(ws_.objective, rel=1e-5)
        assert sorted(ws_.sizes.tolist()) == sorted(want.sizes.tolist())
    # objective: a sum of N scores, each within the fp32 dot-product bound (D + 2) 2^-24 sum|x c| of the
    # search contract (the fixed-point rounding of the sum itself is below 2^-30 of it)
    cw = want.centroids.double()
    dots = (xs.double() * cw[want.labels.long()]).sum(1)
    tol = ((D + 2) * U * (xs.double().abs() * cw[want.labels.long()].abs()).sum(1))
    if metric == "cosine":
        exact, bound = dots.sum(), tol.sum()
    else:
        exact = ((xs.double() - cw[want.labels.long()]) ** 2).sum(1).sum()
        xsq, csq = (xs.double() ** 2).sum(1), (cw ** 2).sum(1)[want.labels.long()]
        bound = (2 * tol + (D + 2) * U * (xsq + csq)).sum()
    print(f"objective gpu {got.objective!r} cpu {want.objective!r} fp64 {float(exact)!r} bound {float(bound):.3e}")
    assert abs(got.objective - float(exact)) <= float(bound)
    assert abs(want.objective - float(exact)) <= float(bound)


def test_map_cluster_op_on_a_small_npy(gpu, tmp_path, monkeypatch):
    from ops.map_cluster import map_cluster

    monkeypatch.delenv("CLASSIFY_DEVICE", raising=False)
    N, K, D = 300, 4, 64
    x, planted = _blobs(N, K, D, 9)
    path = str(tmp_path / "vec.npy")
    np.save(path, x.numpy())
    out = str(tmp_path / "out.npy")
    for metric in ("cosine", "l2"):
        r = map_cluster({"vectors_uri": path, "k": K, "metric": metric, "seed": 2, "representatives": 3})
        assert r["ok"] and r["op"] == "map_cluster" and r["row_count"] == N and r["dim"] == D and r["k"] == K
        assert r["converged"] and r["changed_last"] == 0 and sum(r["sizes"]) == N and r["empty_clusters"] == 0
        assert len(set(zip(planted.tolist(), r["labels"]))) == K
        for k, rep in enumerate(r["representatives"]):
            assert len(rep["ids"]) == 3 and all(r["labels"][i] == k for i in rep["ids"])
            assert rep["scores"] == sorted(rep["scores"], reverse=True)
        monkeypatch.setenv("CLASSIFY_DEVICE", "cpu")
        h = map_cluster({"vectors_uri": path, "k": K, "metric": metric, "seed": 2, "representatives": 3})
        monkeypatch.delenv("CLASSIFY_DEVICE")
        for key in ("labels", "sizes", "centroids", "iterations"):
            assert r[key] == h[key], key
    # the index LRU (2 entries) still holds the GPU engine's unnormalised rows of the l2 job
    r = map_cluster({"vectors_uri": path, "k": K, "metric": "l2", "output": "npy", "output_uri": out})
    assert r["index_cached"] is True and "labels" not in r
    assert np.load(r["labels_uri"]).shape == (N,) and np.load(r["centroids_uri"]).shape == (K, D)
    with pytest.raises(ValueError, match="kmeans_assign: unsupported shape"):
        bad = str(tmp_path / "bad.npy")
        np.save(bad, np.ones((10, 96), dtype=np.float32))
        map_cluster({"vectors_uri": bad, "k": 2})
