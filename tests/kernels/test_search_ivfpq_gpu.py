"""IVF-PQ (csrc/kernels/pq_ivf.hip): the scan and the residual encoder against their PyTorch twins, bit for bit, and
against the float64 reference ``q . (centroid[label] + decode(codes))``; map_search on the GPU against the CPU engine.
The longest chain has ``D`` coarse terms, ``M`` table entries and one final add, so ``|score - ref| <= gamma_n sum_d
|q_d| (|c_d| + |r_d|)``, ``n = D + M + 1``, ``gamma_n = n u / (1 - n u)``, ``u = 2^-24``: the standard forward bound.
"""
import numpy as np
import pytest
import torch

from agent_tpu_amd import ops

pytestmark = pytest.mark.gpu

_cache = {}


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def _index(D, M, n, K, ties=False):
    """Hand-built: cluster 0 empty and cluster 1 of one row (where K and n allow), random codes, the builder's sort."""
    key = (D, M, n, K, ties)
    if key not in _cache:
        gen = torch.Generator().manual_seed(D + 3 * M + 5 * n + 7 * K)
        labels = torch.randint(0, K, (n,), generator=gen)
        if K > 2:
            labels[labels <= 1] = K - 1
            if n > 1:
                labels[n // 2] = 1
        codes = torch.randint(0, 256, (n, M), generator=gen).to(torch.uint8)
        cent = torch.randn(K, D, generator=gen)
        if ties:  # three distinct rows of codes and one centroid: equal scores in different clusters and lanes
            codes = codes[:3][torch.randint(0, 3, (n,), generator=gen)]
            cent[:] = cent[0]
        order = torch.sort(labels, stable=True).indices
        offsets = torch.zeros(K + 1, dtype=torch.int32)
        offsets[1:] = torch.cumsum(torch.bincount(labels, minlength=K), 0).to(torch.int32)
        _cache[key] = (torch.randn(33, D, generator=gen), 0.3 * torch.randn(M, 256, D // M, generator=gen),
                       codes[order].contiguous(), order.to(torch.int32), offsets, cent)
    return _cache[key]


def _check_fp64(q, books, codes, rid, off, cent, nprobe, s, i, cnt, D, M):
    n, K = codes.shape[0], cent.shape[0]
    cluster = torch.repeat_interleave(torch.arange(K), (off[1:] - off[:-1]).long())
    c, r = cent[cluster].double(), ops.pq_decode(codes, books).double()
    ref = torch.empty(q.shape[0], n, dtype=torch.float64)
    mag = torch.empty_like(ref)
    ref[:, rid.long()] = q.double() @ (c + r).T
    mag[:, rid.long()] = q.double().abs() @ (c.abs() + r.abs()).T
    nu = (D + M + 1) * 2.0 ** -24
    bound = nu / (1 - nu) * mag
    label = torch.empty(n, dtype=torch.int64)
    label[rid.long()] = cluster
    probes = ops.sim_topk_ref(q, cent, nprobe)[1]
    for a in range(q.shape[0]):
        m = int(cnt[a])
        ids = i[a, :m] - 1000
        probed = torch.isin(label, probes[a])
        assert m == min(s.shape[1], int(probed.sum())) and bool(probed[ids].all())
        assert bool(((s[a, :m].double() - ref[a, ids]).abs() <= bound[a, ids]).all()), a
        probed[ids] = False  # the probed rows left out
        if m and bool(probed.any()):
            assert bool((ref[a, probed] <= ref[a, ids[-1]] + bound[a, ids[-1]] + bound[a, probed]).all()), a


# dsub 16 / 4 / 4 at every n, and one case with the table at the LDS limit (k = 32 below)
SHAPES = [(D, M, n) for D, M in ((64, 4), (64, 16), (128, 32)) for n in (1, 63, 65, 257, 1000)] + [(512, 128, 257)]


@pytest.mark.parametrize("D,M,n", SHAPES)
def test_scan_equals_the_twin_and_the_fp64_reference(gpu, D, M, n):
    for K in (1, 3, 7, n // 64 + 9):
        q, books, codes, rid, off, cent = _index(D, M, n, K)
        q = q[:5].contiguous()
        dev = [t.to(gpu) for t in (q, books, codes, rid, off, cent)]
        dev[2] = ops.pq_interleave(dev[2])
        for k in ((32,) if M == 128 else (1, 8, 9, 32)):
            for nprobe in sorted({1, min(2, K), min(K, 32)}):
                ws, wi, wc = ops.sim_topk_ivfpq_ref(q, books, codes, rid, off, cent, k, nprobe, 1000)
                for splits in (1, 3, 200):  # 200: more than the query's blocks
                    s, i, c = ops.sim_topk_ivfpq(*dev, k, nprobe, 1000, splits=splits)
                    assert s.shape == (5, k) and torch.equal(c.cpu(), wc), (D, M, n, K, k, nprobe, splits)
                    assert torch.equal(i.cpu(), wi) and torch.equal(_bits(s), _bits(ws)), (D, M, n, K, k, nprobe, splits)
                _check_fp64(q, books, codes, rid, off, cent, nprobe, ws, wi, wc, D, M)


def test_equal_scores_come_back_in_ascending_original_id(gpu):
    q, books, codes, rid, off, cent = _index(64, 16, 1000, 7, ties=True)
    ws, wi, wc = ops.sim_topk_ivfpq_ref(q, books, codes, rid, off, cent, 32, 7, 5)
    same = ws[:, 1:] == ws[:, :-1]
    assert same.float().mean() > 0.8 and bool((wi[:, 1:] > wi[:, :-1])[same].all()) and wc.tolist() == [32] * 33
    dev = [t.to(gpu) for t in (q, books, codes, rid, off, cent)]
    for splits in (1, 3, None):
        s, i, c = ops.sim_topk_ivfpq(*dev, 32, 7, 5, splits=splits)
        assert torch.equal(i.cpu(), wi) and torch.equal(_bits(s), _bits(ws)), splits


def test_a_query_alone_equals_the_query_inside_a_batch_of_33(gpu):
    dev = [t.to(gpu) for t in _index(128, 32, 1000, 7)]
    s, i, c = ops.sim_topk_ivfpq(*dev, 9, 2)
    for a in (0, 16, 32):
        s1, i1, c1 = ops.sim_topk_ivfpq(dev[0][a:a + 1].contiguous(), *dev[1:], 9, 2)
        assert torch.equal(s1[0], s[a]) and torch.equal(i1[0], i[a]) and int(c1[0]) == int(c[a]), a


@pytest.mark.parametrize("D,M", [(64, 4), (64, 8), (64, 16)])
def test_encode_residual_equals_the_twin_of_the_subtracted_rows(gpu, D, M):
    gen = torch.Generator().manual_seed(D * M)
    books, cent = torch.randn(M, 256, D // M, generator=gen), torch.randn(7, D, generator=gen)
    books[:, 200] = books[:, 17]  # a duplicated codeword: the lower id wins
    bias = ops.pq_bias(books)
    for n in (1, 300, 1000):
        x = torch.randn(n, D, generator=gen)
        labels = torch.randint(0, 7, (n,), generator=gen).to(torch.int32)
        x[::3] = cent[labels[::3].long()] + books[:, 200].reshape(1, D)  # residual = codeword 200 = 17, up to rounding
        want = ops.pq_encode_ref((x - cent[labels.long()]).contiguous(), books, bias)
        got = ops.pq_encode_residual(x.to(gpu), labels.to(gpu), cent.to(gpu), books.to(gpu), bias.to(gpu))
        assert got.dtype == torch.uint8 and torch.equal(got.cpu(), want) and bool((want != 200).all()), (D, M, n)


def test_map_search_ivfpq_on_the_gpu_engine_equals_the_cpu_engine(gpu, tmp_path, monkeypatch):
    """600 rows of sixteen +-1 entries at D = 64: the normalisation (a division by 4) is exact on either device."""
    from agent_tpu_amd.runtime import ivfpq
    from agent_tpu_amd.runtime import search as rs
    from ops.map_search import map_search

    monkeypatch.delenv("SEARCH_INDEX_DTYPE", raising=False)
    rs.clear_cache()
    N, D, M, K = 600, 64, 16, 6
    gen = torch.Generator().manual_seed(6)
    c = torch.zeros(N, D)
    for r in range(N):
        c[r, torch.randperm(D, generator=gen)[:16]] = torch.randint(0, 2, (16,), generator=gen).float() * 2 - 1
    path = str(tmp_path / "corpus.npy")
    np.save(path, c.numpy())
    ix = {"type": "ivfpq", "subvectors": M, "clusters": K, "nprobe": 2, "train_rows": 512, "train_iterations": 4}
    job = {"query_vectors": torch.cat([c[3:4], c[500:507]]).tolist(), "corpus_uri": path, "top_k": 10, "index": ix}
    try:
        monkeypatch.setenv("CLASSIFY_DEVICE", "cpu")
        cpu = map_search(dict(job))
        monkeypatch.delenv("CLASSIFY_DEVICE")
        dev = map_search(dict(job))
        again = map_search(dict(job, index=dict(ix, nprobe=K)))
        assert dev["ids"] == cpu["ids"] and dev["scores"] == cpu["scores"] and dev["ids"][0][0] == 3
        assert dev["index"] == cpu["index"] == dict(ix, converged=dev["index"]["converged"], bytes_per_row=M + 4)
        assert dev["index_cached"] is False and again["index_cached"] is True
        a = ivfpq.load_index(path, 0, -1, torch.device("cpu"), K, M, 512, 4)
        b = ivfpq.load_index(path, 0, -1, gpu, K, M, 512, 4)
        assert a.cached and b.cached and b.codes.shape == (10, M // 4, 64, 4)
        assert torch.equal(ivfpq.row_major_codes(b).cpu(), a.codes) and torch.equal(b.row_ids.cpu(), a.row_ids)
    finally:
        rs.clear_cache()
