"""refine_topk (csrc/kernels/sim_refine.hip) against its PyTorch twin: ids and score bits, exactly.

Exact data (test_search_f16_gpu.py's recipe): integer-valued operands in [-2, 2] are exact in fp16, every product
and partial sum is an integer below 2^24, and a power-of-two row scale keeps the scaled score exact, so whatever
order the twin sums in, the kernel must return its scores bit for bit, ties included. "cosine" is a power-of-two
scale per row: ``row_scale`` beside an fp16 store, multiplied into the rows of an fp32 store (exact), as the
runtime keeps the two. Where the shortlist holds every row, random data is compared to ``ops.sim_topk`` over the
same store as well: there an equal result means the same accumulation order, not only the same value.
"""
import pytest
import torch

from agent_tpu_amd import ops
from agent_tpu_amd.ops.search import PAD_ID

pytestmark = pytest.mark.gpu

N = 300
NO_ROW = 0x7fffffff
_cache = {}


def _store(D, dtype, metric, random=False):
    """(q [17, D], store [N, D] of dtype, row_scale or None) on the CPU; rows are duplicated, so scores tie."""
    key = (D, dtype, metric, random)
    if key not in _cache:
        gen = torch.Generator().manual_seed(D + (7 if random else 0))
        if random:
            base, q = torch.randn(N // 3, D, generator=gen), torch.randn(17, D, generator=gen)
        else:
            col = torch.tensor([1.0, 2.0, -1.0, -2.0])[(torch.arange(D) * 7 + torch.arange(D) // 5) % 4]
            base = torch.randint(-1, 2, (N // 3, D), generator=gen).float() * col
            q = torch.randint(-2, 3, (17, D), generator=gen).float()
        c = base[torch.randint(0, base.shape[0], (N,), generator=gen)].contiguous()
        n = torch.arange(N)
        scale = torch.tensor([0.25, 0.5, 1.0, 2.0])[(n * 3 + n // 7 + n // 3) % 4].contiguous()
        if metric == "dot":
            scale = None
        elif dtype == torch.float32:
            c, scale = c * scale[:, None], None
        _cache[key] = (q, c.to(dtype).contiguous(), scale)
    return _cache[key]


def _lists(nq, R, k):
    """name -> (cand int32 [nq, R], chunks): (a) distinct random rows and a tail of empty slots that ends inside a
    16-row group, in one workgroup per 32 candidates; (b) fewer live candidates than k; (d) every row, ids past N
    among them, streamed by one workgroup."""
    gen = torch.Generator().manual_seed(nq + R + k)
    a = torch.stack([torch.randperm(N, generator=gen)[:R] for _ in range(nq)]).to(torch.int32)
    a[:, R - 9:] = NO_ROW
    a[:, 3] = -1
    b = torch.full((nq, R), NO_ROW, dtype=torch.int32)
    b[:, 5:5 + (k + 1) // 2] = a[:, :(k + 1) // 2]
    d = torch.arange(320, dtype=torch.int32).flip(0).repeat(nq, 1).contiguous()
    return {"a": (a, R // 32), "b": (b, None), "d": (d, 1)}


def _run(q, c, scale, cand, k, chunks, gpu, host=False):
    store = c.pin_memory() if host else c.to(gpu)
    return ops.refine_topk(q.to(gpu), store, cand.to(gpu), k, id_base=1000, chunks=chunks,
                           row_scale=None if scale is None else scale.to(gpu))


@pytest.mark.parametrize("nq,R,k", [(1, 32, 1), (17, 96, 10), (3, 64, 32)])
@pytest.mark.parametrize("metric", ["dot", "cosine"])
@pytest.mark.parametrize("dtype", [torch.float16, torch.float32], ids=["fp16", "fp32"])
@pytest.mark.parametrize("D", [64, 768])
def test_refine_topk_equals_its_twin(gpu, D, dtype, metric, nq, R, k):
    q, c, scale = _store(D, dtype, metric)
    q = q[:nq].contiguous()
    for name, (cand, chunks) in _lists(nq, R, k).items():
        ws, wi = ops.refine_topk_ref(q, c, cand, k, 1000, scale, dtype=torch.float64)
        s, i = _run(q, c, scale, cand, k, chunks, gpu)
        assert s.shape == i.shape == (nq, k) and s.dtype == torch.float32 and i.dtype == torch.int64
        assert torch.equal(i.cpu(), wi), (name, (i.cpu() != wi).nonzero()[:4])
        assert torch.equal(s.cpu().double(), ws), name
        live = int(((cand >= 0) & (cand < N)).sum(1).min())
        assert (wi[:, min(live, k):] == PAD_ID).all() and (wi[:, :min(live, k)] < 1000 + N).all(), name
        tie = (ws[:, 1:] == ws[:, :-1]) & (wi[:, 1:] != PAD_ID)  # (c) duplicated rows: equal scores, ascending ids
        assert (wi[:, 1:][tie] > wi[:, :-1][tie]).all() and (name != "d" or k < 3 or tie.any()), name
    # (d) every row shortlisted: the exact search over the same store, on random data too
    cand, chunks = _lists(nq, R, k)["d"]
    for random in (False, True):
        q, c, scale = _store(D, dtype, metric, random)
        q = q[:nq].contiguous()
        s, i = _run(q, c, scale, cand, k, chunks, gpu)
        es, ei = ops.sim_topk(q.to(gpu), c.to(gpu), k, id_base=1000, row_scale=None if scale is None else scale.to(gpu))
        assert torch.equal(i, ei) and torch.equal(s, es), random


def test_store_in_pinned_host_memory(gpu):
    q, c, scale = _store(768, torch.float16, "cosine")
    cand, chunks = _lists(17, 96, 10)["a"]
    ws, wi = ops.refine_topk_ref(q, c, cand, 10, 1000, scale, dtype=torch.float64)
    s, i = _run(q, c, scale, cand, 10, chunks, gpu, host=True)
    assert torch.equal(i.cpu(), wi) and torch.equal(s.cpu().double(), ws)
