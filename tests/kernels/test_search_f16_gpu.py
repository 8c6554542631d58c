"""sim_topk over a float16 corpus (csrc/kernels/sim_topk_f16.hip) against its fp64 twin, with and
without ``row_scale``; its invariances and bounds; and map_search with ``corpus_dtype: "float16"``
on the GPU engine. The data recipes are those of test_search_gpu.py.

Exact data: integer-valued operands in [-2, 2] are exact in fp16, and every product and partial
sum is an integer below 2^24, so the kernel must return the fp64 twin's scores and ids bit for
bit, ties included. A power-of-two ``row_scale`` keeps every scaled score exact.

Random data: one (query, row) score is an fp32 fma chain of length D over the stored fp16 values
(exactly widened), then one fp32 multiply by the scale, itself one rounding of the true scale:
``(D + 2) * 2^-24 * scale * sum_k |q_k c_k|`` in fp64 (D roundings of the chain, the scale's one,
one spare for the second-order term). A returned score must lie within that of the fp64 score of
the returned id; a returned id's fp64 score may fall below the fp64 k-th best by at most the two
tolerances involved. Nothing is excluded.
"""
import numpy as np
import pytest
import torch

from agent_tpu_amd import ops

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
_cache = {}


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


def _pow2_scale(N):
    """{0.25, 0.5, 1, 2} per row in an aperiodic pattern."""
    n = torch.arange(N)
    return torch.tensor([0.25, 0.5, 1.0, 2.0])[(n * 3 + n // 7 + n // 3) % 4].contiguous()


EXACT = [  # (D, N, nq, k, id_base)
    (768, 1, 17, 8, 0), (768, 15, 16, 10, 0), (768, 16, 33, 16, 0), (768, 17, 32, 17, 12345),
    (768, 255, 70, 32, 0), (768, 4099, 1, 10, 0), (768, 4099, 33, 8, 0),
    (64, 17, 70, 10, 0), (64, 4099, 1, 16, 0),
    (192, 1000, 32, 17, 0), (960, 255, 33, 32, 0),  # odd multiples of 64: the tail step
    (1024, 4099, 16, 1, 0), (1024, 15, 1, 17, 12345),
]
# one per kernel form: nq <= 16; nq > 16 with k <= 8 and k <= 16; k > 16 (narrow and wide); the tail step
SCALED = [(768, 4099, 1, 10, 0), (768, 4099, 33, 8, 0), (768, 16, 33, 16, 0), (768, 255, 70, 32, 0),
          (1024, 15, 1, 17, 12345), (192, 1000, 32, 17, 0), (64, 4099, 1, 16, 0)]


@pytest.mark.parametrize("D,N,nq,k,id_base", EXACT)
def test_exact_integer_data_equals_the_fp64_twin(gpu, D, N, nq, k, id_base):
    q, c = _exact_case(D, N, nq)
    assert torch.equal(c.half().float(), c)
    ws, wi = ops.sim_topk_ref(q, c, k, id_base, dtype=torch.float64)
    s, i = ops.sim_topk(q.to(gpu), c.half().to(gpu), k, id_base)
    assert s.shape == i.shape == (nq, min(k, N)) and s.dtype == torch.float32 and i.dtype == torch.int64
    assert torch.equal(i.cpu(), wi), (i.cpu() != wi).nonzero()[:4]
    assert torch.equal(s.cpu().double(), ws)


@pytest.mark.parametrize("D,N,nq,k,id_base", SCALED)
def test_exact_with_a_power_of_two_row_scale(gpu, D, N, nq, k, id_base):
    q, c = _exact_case(D, N, nq)
    scale = _pow2_scale(N)
    ws, wi = ops.sim_topk_ref(q, c, k, id_base, dtype=torch.float64, row_scale=scale)
    s, i = ops.sim_topk(q.to(gpu), c.half().to(gpu), k, id_base, row_scale=scale.to(gpu))
    assert torch.equal(i.cpu(), wi), (i.cpu() != wi).nonzero()[:4]
    assert torch.equal(s.cpu().double(), ws)
    if N > 1:  # an ignored scale, or one applied after the ranking, fails here
        _, plain = ops.sim_topk(q.to(gpu), c.half().to(gpu), k, id_base)
        assert (plain != i).any(dim=1).any()


def _random_case(N, nq, D=768, dup=False, seed=1):
    """fp32 unit queries; fp16 corpus rows (normalised, then rounded) and the fp32 scale that
    renormalises them."""
    key = ("rand", N, nq, D, dup, seed)
    if key not in _cache:
        gen = torch.Generator().manual_seed(seed)
        c = torch.nn.functional.normalize(torch.randn(N, D, generator=gen), dim=1)
        if dup:
            c = c[torch.randint(0, N // 2, (N,), generator=gen)]
        q = torch.nn.functional.normalize(torch.randn(nq, D, generator=gen), dim=1)
        c = c.half().contiguous()
        scale = (1.0 / c.float().norm(dim=1)).contiguous()
        _cache[key] = (q.contiguous(), c, scale)
    return _cache[key]


def _check_within_bound(s, i, exact, tol, k, N):
    """test_random_data_within_the_fma_chain_bound's three assertions -> worst |d| / tol."""
    worst = 0.0
    for a in range(s.shape[0]):
        ids = i[a]
        assert len(set(ids.tolist())) == k and ids.min() >= 0 and ids.max() < N
        d = (s[a] - exact[a, ids]).abs()
        worst = max(worst, (d / tol[a, ids]).max().item())
        assert (d <= tol[a, ids]).all(), a
        kth_v, kth_i = torch.sort(exact[a], descending=True, stable=True)
        kth_v, kth_i = kth_v[k - 1], kth_i[k - 1]
        assert (exact[a, ids] >= kth_v - tol[a, ids] - tol[a, kth_i]).all(), a
        pairs = list(zip((-s[a]).tolist(), ids.tolist()))
        assert pairs == sorted(pairs), a
    return worst


def test_random_data_within_the_fma_chain_bound(gpu):
    D, N, nq, k = 768, 3000, 33, 10
    q, c, scale = _random_case(N, nq)
    s, i = ops.sim_topk(q.to(gpu), c.to(gpu), k, row_scale=scale.to(gpu))
    exact = (q.double() @ c.double().T) * scale.double()
    tol = (D + 2) * U * scale.double() * (q.double().abs() @ c.double().abs().T)  # [nq, N]
    worst = _check_within_bound(s.cpu().double(), i.cpu(), exact, tol, k, N)
    print(f"random fp16 data: worst |score - fp64| / tolerance {worst:.4f}")


def test_result_does_not_depend_on_splits_batch_or_run(gpu):
    N, k = 4099, 10
    q, c, scale = _random_case(N, 70, dup=True, seed=2)
    dq, dc, ds = q.to(gpu), c.to(gpu), scale.to(gpu)
    s0, i0 = ops.sim_topk(dq, dc, k, row_scale=ds)
    for splits in (1, 2, 7, 64):
        s, i = ops.sim_topk(dq, dc, k, splits=splits, row_scale=ds)
        assert torch.equal(s, s0) and torch.equal(i, i0), splits
    s, i = ops.sim_topk(dq, dc, k, row_scale=ds)
    assert torch.equal(s, s0) and torch.equal(i, i0)
    s17, i17 = ops.sim_topk(dq[:17].contiguous(), dc, k, row_scale=ds)
    assert torch.equal(s17, s0[:17]) and torch.equal(i17, i0[:17])
    for a in (0, 16, 40, 69):
        s1, i1 = ops.sim_topk(dq[a:a + 1].contiguous(), dc, k, row_scale=ds)
        assert torch.equal(s1[0], s0[a]) and torch.equal(i1[0], i0[a]), a
    for a in (5, 16):  # inside 17 at another position: queries 2 .. 18 and 13 .. 29
        lo = a - 3
        s2, i2 = ops.sim_topk(dq[lo:lo + 17].contiguous(), dc, k, row_scale=ds)
        assert torch.equal(s2[a - lo], s0[a]) and torch.equal(i2[a - lo], i0[a]), a
    # the duplicated rows tie (equal rows have equal scales): equal scores come back in ascending id
    sc, ic = s0.cpu(), i0.cpu()
    same = sc[:, 1:] == sc[:, :-1]
    assert same.any() and (ic[:, 1:][same] > ic[:, :-1][same]).all()


@pytest.mark.parametrize("N", [1, 15, 17, 4099])
def test_nothing_outside_the_corpus_is_read(gpu, N):
    D, pad, k = 768, 64, 10
    q, c, scale = _random_case(max(N, 2), 33, seed=3)
    c, scale = c[:N].contiguous(), scale[:N].contiguous()
    s0, i0 = ops.sim_topk(q.to(gpu), c.to(gpu), k, row_scale=scale.to(gpu))
    for poison in (65504.0, float("nan")):
        big = torch.full((N + 2 * pad, D), poison, dtype=torch.float16, device=gpu)
        big[pad:pad + N] = c.to(gpu)
        bigs = torch.full((N + 2 * pad,), poison, dtype=torch.float32, device=gpu)
        bigs[pad:pad + N] = scale.to(gpu)
        view, vs = big[pad:pad + N], bigs[pad:pad + N]
        assert view.is_contiguous() and vs.is_contiguous()
        s, i = ops.sim_topk(q.to(gpu), view, k, row_scale=vs)
        assert torch.isfinite(s).all() and torch.equal(s, s0) and torch.equal(i, i0)


def test_rejections_and_empty_query_batch(gpu):
    q = torch.zeros((2, 64), device=gpu)
    c = torch.zeros((40, 64), dtype=torch.float16, device=gpu)
    ok = torch.ones(40, device=gpu)
    bad = [
        lambda: ops.sim_topk(q.half(), c, 4),  # fp16 q
        lambda: ops.sim_topk(q, c.bfloat16(), 4),  # bf16 c
        lambda: ops.sim_topk(q, c.double(), 4),
        lambda: ops.sim_topk(q, c.float(), 4, row_scale=ok),  # a scale with an fp32 c
        lambda: ops.sim_topk(q, c, 4, row_scale=torch.ones(39, device=gpu)),
        lambda: ops.sim_topk(q, c, 4, row_scale=torch.ones((40, 1), device=gpu)),
        lambda: ops.sim_topk(q, c, 4, row_scale=ok.half()),
        lambda: ops.sim_topk(q, c, 4, row_scale=ok.cpu()),
        lambda: ops.sim_topk(q, c, 4, row_scale=torch.ones(80, device=gpu)[::2]),
        lambda: ops.sim_topk(torch.zeros((2, 96), device=gpu), torch.zeros((40, 96), dtype=torch.float16, device=gpu), 4),
        lambda: ops.sim_topk(q, c, 33),
        lambda: ops.sim_topk(q, c[:0], 4),
        lambda: ops.sim_topk(q, torch.zeros((40, 128), dtype=torch.float16, device=gpu)[:, ::2], 4),
    ]
    for f in bad:
        with pytest.raises(ValueError):
            f()
    s, i = ops.sim_topk(torch.zeros((0, 64), device=gpu), c, 4, row_scale=ok)
    assert s.shape == i.shape == (0, 4) and s.dtype == torch.float32 and i.dtype == torch.int64 and s.is_cuda


def test_map_search_op_with_a_float16_resident_corpus(gpu, tmp_path, monkeypatch):
    from agent_tpu_amd.runtime import search as rs
    from agent_tpu_amd.utils.synthetic import make_text_rows
    from ops.map_embed import map_embed
    from ops.map_search import map_search

    monkeypatch.delenv("CLASSIFY_DEVICE", raising=False)
    monkeypatch.delenv("SEARCH_INDEX_DTYPE", raising=False)
    rs.clear_cache()
    N, D, k = 60, 256, 8
    path = str(tmp_path / "corpus16.npy")
    assert map_embed({"texts": make_text_rows(N, 30, 11), "model_path": "bert-tiny?batch=32&seed=2", "output": "npy",
                      "output_uri": path, "dtype": "float16"})["ok"]
    c16 = np.load(path)
    assert c16.dtype == np.float16 and c16.shape == (N, D)
    c = torch.from_numpy(c16.astype(np.float64))
    # known numbers of norm exactly 1: 256 entries of +-1/16, or 64 of +-1/8 among zeros. Their sums of
    # squares are exact in fp32 in any order, so the op's cosine normalisation returns them unchanged
    gen = torch.Generator().manual_seed(5)
    sign = torch.randint(0, 2, (7, D), generator=gen).float() * 2 - 1
    q32 = sign / 16
    q32[4:] = (sign[4:] / 8) * (torch.arange(D) % 4 == 1)
    assert torch.equal((q32 * q32).sum(dim=1), torch.ones(7))
    qv = q32.tolist()
    for metric in ("cosine", "dot"):
        rs.clear_cache()
        job = {"query_vectors": qv, "corpus_uri": path, "top_k": k, "metric": metric, "corpus_dtype": "float16"}
        first, second = map_search(dict(job)), map_search(dict(job))
        assert first["ok"] and first["index_cached"] is False and second["index_cached"] is True
        assert first["ids"] == second["ids"] and first["scores"] == second["scores"]
        assert first["corpus_dtype"] == "float16" and first["corpus_rows"] == N and first["dim"] == D
        info = rs.cache_info()
        assert len(info["entries"]) == 1 and info["entries"][0].endswith("corpus16.npy")
        assert info["resident_bytes"] == N * D * 2 + (N * 4 if metric == "cosine" else 0)
        # fp64 on the host from the file and the query vectors (unit vectors as they are)
        q64 = q32.double()
        scale = 1.0 / c.norm(dim=1) if metric == "cosine" else torch.ones(N, dtype=torch.float64)
        exact = (q64 @ c.T) * scale
        tol = (D + 2) * U * scale * (q64.abs() @ c.abs().T)
        s = torch.tensor(first["scores"], dtype=torch.float64)
        i = torch.tensor(first["ids"], dtype=torch.int64)
        worst = _check_within_bound(s, i, exact, tol, k, N)
        print(f"map_search float16 {metric}: worst |score - fp64| / tolerance {worst:.4f}")
        plain = map_search({"query_vectors": qv, "corpus_uri": path, "top_k": k, "metric": metric})
        assert "corpus_dtype" not in plain and plain["index_cached"] is False
    rs.clear_cache()
