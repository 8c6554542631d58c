"""sim_topk_wide (csrc/kernels/sim_topk_wide.hip): deep lists against the fp64 twin bit for bit on exact data,
the arrival orders that stress its threshold-and-buffer selection, its score bits against sim_topk's, its
invariances and bounds, and map_search ``depth`` on the GPU engine.

Exact data is test_search_gpu.py's: integer-valued operands in [-2, 2] with a per-column factor and duplicated
corpus rows. Every partial sum is an integer below 2^24, so fp32 holds it in any order; the few distinct scores tie
across the k-th place, where only the full (score, id) order selects the right rows.
"""
import numpy as np
import pytest
import torch

from agent_tpu_amd import ops

pytestmark = pytest.mark.gpu

_cache = {}


def _case(kind, D, N, nq):
    key = (kind, D, N, nq)
    if key not in _cache:
        gen = torch.Generator().manual_seed(D + 3 * N + 5 * nq)
        if kind == "exact":
            col = torch.tensor([1.0, 2.0, -1.0, -2.0])[(torch.arange(D) * 7 + torch.arange(D) // 5) % 4]
            base = torch.randint(-1, 2, (max(1, (N + 2) // 3), D), generator=gen).float() * col
            c = base[torch.randint(0, base.shape[0], (N,), generator=gen)]  # duplicated rows: ties
            q = torch.randint(-2, 3, (nq, D), generator=gen).float()
        else:  # random unit rows, half of them duplicates
            c = torch.nn.functional.normalize(torch.randn(N, D, generator=gen), dim=1)
            c = c[torch.randint(0, max(1, N // 2), (N,), generator=gen)]
            q = torch.nn.functional.normalize(torch.randn(nq, D, generator=gen), dim=1)
        _cache[key] = (q.contiguous(), c.contiguous())
    return _cache[key]


EXACT = [  # (D, N, nq, k, id_base): N < k, N = k, N = k + 1, one and many splits, every k, nq and D
    (768, 20, 17, 33, 0), (64, 64, 1, 64, 0), (64, 101, 16, 100, 12345), (64, 1025, 33, 1024, 0),
    (1024, 1024, 17, 1024, 0), (768, 4099, 33, 100, 0), (1024, 4099, 16, 1024, 0), (768, 4099, 1, 64, 0),
    (64, 20011, 17, 1024, 0), (768, 20011, 16, 33, 0),
    (64, 40, 2740, 1024, 0),  # past ops.search.WIDE_WS_BYTES at one split: two query chunks
]


@pytest.mark.parametrize("D,N,nq,k,id_base", EXACT)
def test_exact_integer_data_equals_the_fp64_twin(gpu, D, N, nq, k, id_base):
    q, c = _case("exact", D, N, nq)
    ws, wi = ops.sim_topk_ref(q, c, k, id_base, dtype=torch.float64)
    s, i = ops.sim_topk_wide(q.to(gpu), c.to(gpu), k, id_base)
    assert s.shape == i.shape == (nq, min(k, N)) and s.dtype == torch.float32 and i.dtype == torch.int64
    assert torch.equal(i.cpu(), wi), (i.cpu() != wi).nonzero()[:4]
    assert torch.equal(s.cpu().double(), ws)


@pytest.mark.parametrize("splits", [1, 7])
@pytest.mark.parametrize("k", [33, 1024])
def test_worst_case_arrival_orders(gpu, k, splits):
    """c[j] = j e_0. The query +e_0 sees ascending scores (every row passes the threshold: the most appends and
    prunes the design allows), -e_0 descending ones (nothing passes after the first k), 0 an N-way tie."""
    N, D = 4099, 64
    c = torch.zeros(N, D)
    c[:, 0] = torch.arange(N).float()
    q = torch.zeros(3, D)
    q[0, 0], q[1, 0] = 1.0, -1.0
    ws, wi = ops.sim_topk_ref(q, c, k, dtype=torch.float64)
    assert wi[2].tolist() == list(range(k))
    s, i = ops.sim_topk_wide(q.to(gpu), c.to(gpu), k, splits=splits)
    assert torch.equal(i.cpu(), wi) and torch.equal(s.cpu().double(), ws)


@pytest.mark.parametrize("half", [False, True])
@pytest.mark.parametrize("k", [1, 10, 32, 100, 1024])
def test_same_bits_as_sim_topk(gpu, k, half):
    q, c = _case("random", 768, 4099, 33)
    q, c, scale = q.to(gpu), c.to(gpu), None
    if half:
        c = c.half()
        scale = (0.5 + torch.rand(4099, generator=torch.Generator().manual_seed(9))).to(gpu)
    s0, i0 = ops.sim_topk(q, c, min(k, 32), row_scale=scale)
    s, i = ops.sim_topk_wide(q, c, k, row_scale=scale)
    assert s.shape == (33, k)
    assert torch.equal(s[:, :32], s0) and torch.equal(i[:, :32], i0)


def test_result_does_not_depend_on_splits_batch_or_run(gpu):
    k = 100
    q, c = _case("random", 768, 4099, 33)
    dq, dc = q.to(gpu), c.to(gpu)
    s0, i0 = ops.sim_topk_wide(dq, dc, k)
    for splits in (1, 2, 7, 64, None):  # None: a second run
        s, i = ops.sim_topk_wide(dq, dc, k, splits=splits)
        assert torch.equal(s, s0) and torch.equal(i, i0), splits
    s17, i17 = ops.sim_topk_wide(dq[:17].contiguous(), dc, k)
    assert torch.equal(s17, s0[:17]) and torch.equal(i17, i0[:17])
    for a in (0, 16, 32):
        s1, i1 = ops.sim_topk_wide(dq[a:a + 1].contiguous(), dc, k)
        assert torch.equal(s1[0], s0[a]) and torch.equal(i1[0], i0[a]), a
    tied = s0[:, 1:] == s0[:, :-1]
    assert tied.any() and (s0[:, 1:] <= s0[:, :-1]).all() and (i0[:, 1:] > i0[:, :-1])[tied].all()


@pytest.mark.parametrize("N", [1, 33, 4099])
def test_nothing_outside_the_operands_is_read(gpu, N):
    D, pad, k, nq = 768, 64, 64, 17
    q, c = _case("random", D, max(N, 2), nq)
    q, c = q.to(gpu), c[:N].to(gpu)
    s0, i0 = ops.sim_topk_wide(q.contiguous(), c.contiguous(), k)
    bigc = torch.full((N + 2 * pad, D), float("nan"), device=gpu)
    bigq = torch.full((nq + 2 * pad, D), float("nan"), device=gpu)
    bigc[pad:pad + N], bigq[pad:pad + nq] = c, q
    s, i = ops.sim_topk_wide(bigq[pad:pad + nq], bigc[pad:pad + N], k)
    assert not torch.isnan(s).any() and torch.equal(s, s0) and torch.equal(i, i0)
    s0, i0 = ops.sim_topk_wide(q.contiguous(), c.half(), k)  # the fp16 kernel
    s, i = ops.sim_topk_wide(bigq[pad:pad + nq], bigc.half()[pad:pad + N], k)
    assert not torch.isnan(s).any() and torch.equal(s, s0) and torch.equal(i, i0)


@pytest.mark.parametrize("corpus_dtype", ["float32", "float16"])
def test_map_search_depth_on_the_gpu_engine(gpu, tmp_path, monkeypatch, corpus_dtype):
    from agent_tpu_amd.runtime import search as rs
    from ops.map_search import map_search

    monkeypatch.delenv("CLASSIFY_DEVICE", raising=False)
    monkeypatch.delenv("SEARCH_INDEX_DTYPE", raising=False)
    rs.clear_cache()
    q, c = _case("exact", 64, 150, 5)  # small integers: exact in fp16 too
    for rows in (150, 60):
        path = str(tmp_path / f"corpus{rows}.npy")
        np.save(path, c[:rows].numpy())
        got = map_search({"query_vectors": q.tolist(), "corpus_uri": path, "depth": 100, "metric": "dot",
                          "corpus_dtype": corpus_dtype})
        resident = c[:rows].to(gpu).to(getattr(torch, corpus_dtype)).contiguous()
        s, i = ops.sim_topk_wide(q.to(gpu), resident, 100)
        assert got["ok"] and got["depth"] == 100 and got["corpus_rows"] == rows
        assert all(len(row) == min(100, rows) for row in got["ids"]) and len(got["ids"]) == 5
        assert got["ids"] == i.tolist() and got["scores"] == s.tolist()
    rs.clear_cache()
