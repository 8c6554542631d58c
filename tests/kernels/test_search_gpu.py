"""sim_topk (csrc/kernels/sim_topk.hip) against its fp64 twin, its invariances and bounds, and the
map_search op on the GPU engine.

Exact data: integer-valued fp32 operands in [-2, 2]. Every product and every partial sum is an
integer of magnitude <= 4 * 1024 < 2^24, so fp32 holds it exactly in any summation order and the
kernel must return the fp64 twin's scores and ids bit for bit, ties (duplicated corpus rows)
included. The corpus is asymmetric: column j is a {-1, 0, 1} value times a per-column factor
from {1, 2, -1, -2} in an aperiodic pattern, so a transposed operand or a k permutation applied
to one operand only changes the scores.

Random data: the tolerance of one (query, row) score is the standard bound of an fp32 fma chain
of length D, ``D * 2^-24 * sum_k |q_k c_k|`` with the sum in fp64 (each of the D roundings is at
most half an ulp, ``2^-24`` relative, of a partial sum no larger than ``sum_k |q_k c_k|``). A
returned score must lie within that tolerance of the fp64 score of the returned id; a returned
id's fp64 score may fall below the fp64 k-th best score by at most the two tolerances involved
(its own and the k-th best row's: the kernel ranks by computed scores, each off by its tolerance).
Nothing is excluded.
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


EXACT = [  # (D, N, nq, k, id_base): D = 768 with every N; every nq and k at least once; k > N; id_base
    (768, 1, 17, 8, 0), (768, 15, 16, 10, 0), (768, 16, 33, 16, 0), (768, 17, 32, 17, 12345),
    (768, 255, 70, 32, 0), (768, 1000, 1, 10, 0), (768, 4099, 33, 8, 0), (768, 4099, 17, 32, 12345),
    (64, 17, 70, 10, 0), (64, 4099, 1, 16, 0), (64, 1000, 32, 17, 0),
    (1024, 255, 33, 32, 0), (1024, 4099, 16, 1, 0), (1024, 15, 1, 17, 12345),
]


@pytest.mark.parametrize("D,N,nq,k,id_base", EXACT)
def test_exact_integer_data_equals_the_fp64_twin(gpu, D, N, nq, k, id_base):
    q, c = _exact_case(D, N, nq)
    ws, wi = ops.sim_topk_ref(q, c, k, id_base, dtype=torch.float64)
    s, i = ops.sim_topk(q.to(gpu), c.to(gpu), k, id_base)
    assert s.shape == i.shape == (nq, min(k, N)) and s.dtype == torch.float32 and i.dtype == torch.int64
    assert torch.equal(i.cpu(), wi), (i.cpu() != wi).nonzero()[:4]
    assert torch.equal(s.cpu().double(), ws)


def _random_case(N, nq, D=768, dup=False, seed=1):
    key = ("rand", N, nq, D, dup, seed)
    if key not in _cache:
        gen = torch.Generator().manual_seed(seed)
        c = torch.nn.functional.normalize(torch.randn(N, D, generator=gen), dim=1)
        if dup:
            c = c[torch.randint(0, N // 2, (N,), generator=gen)]
        q = torch.nn.functional.normalize(torch.randn(nq, D, generator=gen), dim=1)
        _cache[key] = (q.contiguous(), c.contiguous())
    return _cache[key]


def test_random_data_within_the_fma_chain_bound(gpu):
    D, N, nq, k = 768, 3000, 33, 10
    q, c = _random_case(N, nq)
    s, i = ops.sim_topk(q.to(gpu), c.to(gpu), k)
    s, i = s.cpu().double(), i.cpu()
    exact = q.double() @ c.double().T
    tol = D * U * (q.double().abs() @ c.double().abs().T)  # [nq, N]
    worst = 0.0
    for a in range(nq):
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
    print(f"random data: worst |score - fp64| / tolerance {worst:.4f}")


def test_result_does_not_depend_on_splits_batch_or_run(gpu):
    N, k = 4099, 10
    q, c = _random_case(N, 70, dup=True, seed=2)
    dq, dc = q.to(gpu), c.to(gpu)
    s0, i0 = ops.sim_topk(dq, dc, k)
    for splits in (1, 2, 7, 64):
        s, i = ops.sim_topk(dq, dc, k, splits=splits)
        assert torch.equal(s, s0) and torch.equal(i, i0), splits
    s, i = ops.sim_topk(dq, dc, k)
    assert torch.equal(s, s0) and torch.equal(i, i0)
    s17, i17 = ops.sim_topk(dq[:17].contiguous(), dc, k)
    assert torch.equal(s17, s0[:17]) and torch.equal(i17, i0[:17])
    for a in (0, 16, 40, 69):
        s1, i1 = ops.sim_topk(dq[a:a + 1].contiguous(), dc, k)
        assert torch.equal(s1[0], s0[a]) and torch.equal(i1[0], i0[a]), a
    for a in (5, 16):  # inside 17 at another position: queries 3 .. 19
        lo = a - 3 if a >= 3 else 0
        s2, i2 = ops.sim_topk(dq[lo:lo + 17].contiguous(), dc, k)
        assert torch.equal(s2[a - lo], s0[a]) and torch.equal(i2[a - lo], i0[a]), a
    # the duplicated rows tie: equal scores come back in ascending id
    sc, ic = s0.cpu(), i0.cpu()
    same = sc[:, 1:] == sc[:, :-1]
    assert same.any() and (ic[:, 1:][same] > ic[:, :-1][same]).all()


@pytest.mark.parametrize("N", [1, 15, 17, 4099])
def test_nothing_outside_the_corpus_is_read(gpu, N):
    D, pad, k = 768, 64, 10
    q, c = _random_case(max(N, 2), 33, seed=3)
    c = c[:N].contiguous()
    for poison in (1e30, float("nan")):
        big = torch.full((N + 2 * pad, D), poison, dtype=torch.float32, device=gpu)
        big[pad:pad + N] = c.to(gpu)
        view = big[pad:pad + N]
        assert view.is_contiguous()
        s, i = ops.sim_topk(q.to(gpu), view, k)
        s0, i0 = ops.sim_topk(q.to(gpu), c.to(gpu), k)
        assert torch.isfinite(s).all() and torch.equal(s, s0) and torch.equal(i, i0)


def test_rejections_and_empty_query_batch(gpu):
    c = torch.zeros((40, 64), device=gpu)
    for D in (96, 1088):
        with pytest.raises(ValueError):
            ops.sim_topk(torch.zeros((2, D), device=gpu), torch.zeros((40, D), device=gpu), 4)
    for k in (0, 33):
        with pytest.raises(ValueError):
            ops.sim_topk(torch.zeros((2, 64), device=gpu), c, k)
    with pytest.raises(ValueError):
        ops.sim_topk(torch.zeros((2, 128), device=gpu)[:, ::2], c, 4)
    with pytest.raises(ValueError):
        ops.sim_topk(torch.zeros((2, 64), device=gpu), torch.zeros((40, 128), device=gpu)[:, ::2], 4)
    with pytest.raises(ValueError):
        ops.sim_topk(torch.zeros((2, 64), device=gpu), torch.zeros((0, 64), device=gpu), 4)
    s, i = ops.sim_topk(torch.zeros((0, 64), device=gpu), c, 4)
    assert s.shape == i.shape == (0, 4) and s.dtype == torch.float32 and i.dtype == torch.int64 and s.is_cuda


def test_map_search_op_on_the_gpu_engine_agrees_with_the_cpu_engine(gpu, tmp_path, monkeypatch):
    """The bf16 GPU encoder and the fp32 CPU encoder embed a text differently; their rankings must
    agree wherever the CPU run's margin between consecutive scores exceeds what that measured
    embedding difference can move a score by. With unit rows ``|q| = |c| = 1`` (up to rounding),
    ``|q'.c' - q.c| <= |dq| + |dc| + |dq| |dc|`` for embedding differences ``dq``, ``dc``; both
    neighbours of a margin may move, in opposite directions: twice that."""
    from agent_tpu_amd.utils.synthetic import make_text_rows
    from ops.map_embed import map_embed
    from ops.map_search import map_search

    model = "bert-tiny?batch=32&seed=2"
    corpus = make_text_rows(60, 30, 11)
    queries = corpus[:5] + make_text_rows(4, 20, 12)
    out = {}
    for dev in ("gpu", "cpu"):
        if dev == "cpu":
            monkeypatch.setenv("CLASSIFY_DEVICE", "cpu")
        else:
            monkeypatch.delenv("CLASSIFY_DEVICE", raising=False)
        path = str(tmp_path / f"corpus_{dev}.npy")
        assert map_embed({"texts": corpus, "model_path": model, "output": "npy", "output_uri": path})["ok"]
        job = {"queries": queries, "corpus_uri": path, "model_path": model, "top_k": 8}
        first, second = map_search(dict(job)), map_search(dict(job))
        assert first["ok"] and first["index_cached"] is False and second["index_cached"] is True
        assert first["ids"] == second["ids"] and first["scores"] == second["scores"]
        assert first["corpus_rows"] == 60 and first["dim"] == 256 and first["query_count"] == 9
        qemb = map_embed({"texts": queries, "model_path": model})["embeddings"]
        out[dev] = (first, np.load(path).astype(np.float64), np.asarray(qemb, dtype=np.float64))
    (g, gc, gq), (h, hc, hq) = out["gpu"], out["cpu"]
    dc = np.linalg.norm(gc - hc, axis=1).max()
    dq = np.linalg.norm(gq - hq, axis=1).max()
    move = 2 * (dq + dc + dq * dc)
    print(f"embedding difference GPU vs CPU engine: corpus {dc:.3e} queries {dq:.3e}; score margin needed {move:.3e}")
    checked = 0
    for a in range(len(queries)):
        hs, hi, gi = h["scores"][a], h["ids"][a], g["ids"][a]
        for j in range(8):
            above = hs[j - 1] - hs[j] if j > 0 else float("inf")
            below = hs[j] - hs[j + 1] if j + 1 < 8 else 0.0  # the 9th score is unknown: no claim on the last
            if above > move and below > move:
                assert gi[j] == hi[j], (a, j)
                checked += 1
    assert checked > 0
    for a in range(5):  # a corpus text used as a query finds its own row first
        assert g["ids"][a][0] == a and abs(g["scores"][a][0] - 1.0) < 1e-5
