"""Product quantization (csrc/kernels/pq.hip): ``pq_encode``, ``pq_lut`` and the ADC scan with the top-k in its
epilogue, bit for bit against their PyTorch twins on the CPU, and map_search with ``compression`` on the GPU engine
against the CPU engine.

The twins do the kernels' operations one column at a time (every product and every add a PyTorch op of its own, so
one rounding each, no FMA), and the order is fixed: a sub-space dot product is ``p_0, + p_1, ...`` in ascending
column, a row's score ``lut[0][code_0], + lut[1][code_1], ...`` in ascending sub-space. A value has one right bit
pattern, so every comparison below is on the int32 view of the floats or on integers; no tolerance is involved.
References are computed once per shape on the CPU and never changed.
"""
import numpy as np
import pytest
import torch

from agent_tpu_amd import ops

pytestmark = pytest.mark.gpu

SHAPES = [(64, 4), (64, 8), (64, 16), (128, 16)]  # (D, M): dsub 16, 8, 4, 8
_cache = {}


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def _books(D, M, ints=False):
    key = ("books", D, M, ints)
    if key not in _cache:
        gen = torch.Generator().manual_seed(31 * D + M + (7 if ints else 0))
        if ints:
            b = torch.randint(-1, 2, (M, 256, D // M), generator=gen).float()
        else:
            b = torch.randn(M, 256, D // M, generator=gen)
            b[:, 200] = b[:, 17]  # duplicated codewords: the lower id wins
            b[:, 255] = b[:, 0]
        _cache[key] = b.contiguous()
    return _cache[key]


def _rows(D, M, n):
    """Random rows; from row 5 on every fourth row is made of codewords (17 or 200, 0 or 255, and others)."""
    key = ("rows", D, M, n)
    if key not in _cache:
        gen = torch.Generator().manual_seed(D + 3 * M + 5 * n)
        b = _books(D, M)
        x = torch.randn(n, D, generator=gen)
        pick = torch.randint(0, 256, (n, M), generator=gen)
        pick[:, 0], pick[:, M - 1] = 200, 255
        made = b[torch.arange(M)[None, :], pick].reshape(n, D)
        x[5::4] = made[5::4]
        _cache[key] = (x.contiguous(), pick)
    return _cache[key]


# ------------------------------------------------------------------------------------------ pq_encode
@pytest.mark.parametrize("D,M", SHAPES)
def test_encode_equals_the_twin(gpu, D, M):
    b = _books(D, M)
    bias = ops.pq_bias(b)
    assert torch.equal(ops.pq_bias(b.to(gpu)).cpu(), bias)
    for n in (1, 63, 65, 1000):
        x, pick = _rows(D, M, n)
        want = ops.pq_encode_ref(x, b, bias)
        got = ops.pq_encode(x.to(gpu), b.to(gpu), bias.to(gpu))
        assert got.dtype == torch.uint8 and got.shape == (n, M) and torch.equal(got.cpu(), want), (D, M, n)
        # a row made of codewords gets them back, a duplicated codeword under its lower id
        made = want[5::4].long()
        exp = pick[5::4].clone()
        exp[exp == 200] = 17
        exp[exp == 255] = 0
        assert torch.equal(made, exp)
        assert torch.equal(ops.pq_decode(got, b.to(gpu))[5::4].cpu(), x[5::4])


@pytest.mark.parametrize("D,M", SHAPES)
def test_encode_ties_go_to_the_lower_codeword_and_signed_zeros_tie(gpu, D, M):
    """Small integers: a score is exact and many codewords tie; products of 0 and -1 are -0.0, and the bias holds
    both zeros."""
    b = _books(D, M, ints=True)
    gen = torch.Generator().manual_seed(D * M)
    bias = torch.zeros(M, 256)
    bias[:, ::3] = -0.0
    x = torch.randint(-1, 2, (300, D), generator=gen).float()
    x[::7] = 0.0  # every score +-0.0: codeword 0
    x[3::7] = -0.0
    want = ops.pq_encode_ref(x, b, bias)
    assert (want[::7] == 0).all() and (want[3::7] == 0).all()
    got = ops.pq_encode(x.to(gpu), b.to(gpu), bias.to(gpu))
    assert torch.equal(got.cpu(), want)


# --------------------------------------------------------------------------------------------- pq_lut
@pytest.mark.parametrize("D,M", SHAPES)
def test_lut_equals_the_twin(gpu, D, M):
    b = _books(D, M)
    for nq in (1, 3, 33):
        q = _rows(D, M, 65)[0][:nq].contiguous()
        want = ops.pq_lut_ref(q, b)
        got = ops.pq_lut(q.to(gpu), b.to(gpu))
        assert got.shape == (nq, M, 256) and got.dtype == torch.float32
        assert torch.equal(_bits(got), _bits(want)), (D, M, nq)
    z = ops.pq_lut(torch.zeros(1, D, device=gpu), _books(D, M, ints=True).to(gpu))  # 0 * -1 = -0.0 survives
    assert torch.equal(_bits(z), _bits(ops.pq_lut_ref(torch.zeros(1, D), _books(D, M, ints=True))))
    if D // M == 4:  # an all -1 codeword of four columns occurs among the 256 x M
        assert (_bits(z) != 0).any()


# ----------------------------------------------------------------------------------------------- scan
def _scan_case(M, N, ints=False):
    """(lut [33, M, 256], codes [N, M], the twin's (scores, ids) at k = 32)."""
    key = ("scan", M, N, ints)
    if key not in _cache:
        gen = torch.Generator().manual_seed(1000 * M + N + (1 if ints else 0))
        codes = torch.randint(0, 256, (N, M), generator=gen).to(torch.uint8)
        if ints:
            lut = torch.randint(-1, 1, (33, M, 256), generator=gen).float()  # -1 and +0.0
            lut[:, :, 0] = -0.0
            codes = codes % 6  # few distinct entries: many equal scores
            codes[::5] = 0  # rows whose score is -0.0: they tie with the rows that score +0.0
        else:
            lut = torch.randn(33, M, 256, generator=gen)
        _cache[key] = (lut.contiguous(), codes.contiguous(), ops.pq_scan_topk_ref(lut, codes, 32, 7))
    return _cache[key]


def _check_scan(gpu, M, N, ints=False):
    lut, codes, (ws, wi) = _scan_case(M, N, ints)
    lg, cg = lut.to(gpu), codes.to(gpu)
    pc = ops.pq_interleave(cg)
    assert torch.equal(ops.pq_deinterleave(pc), cg)
    for nq in (1, 3, 33):
        for k in (1, 10, 32):
            kk = min(k, N)
            s, i = ops.pq_scan_topk(lg[:nq].contiguous(), pc, k, 7)
            assert s.shape == i.shape == (nq, kk) and s.dtype == torch.float32 and i.dtype == torch.int64
            assert torch.equal(i.cpu(), wi[:nq, :kk]) and torch.equal(_bits(s), _bits(ws[:nq, :kk])), (M, N, nq, k)
    # splits give equal bits, row-major codes are accepted, and a query alone equals the query in the batch
    for splits in (1, 2, 7):
        s, i = ops.pq_scan_topk(lg, cg, 10, 7, splits=splits)
        assert torch.equal(i.cpu(), wi[:, :10]) and torch.equal(_bits(s), _bits(ws[:, :10])), (M, N, splits)
    for a in (0, 2, 32):
        s, i = ops.pq_scan_topk(lg[a:a + 1].contiguous(), pc, 32, 7)
        assert torch.equal(i.cpu(), wi[a:a + 1]) and torch.equal(_bits(s), _bits(ws[a:a + 1])), (M, N, a)


@pytest.mark.parametrize("M", [4, 16])
@pytest.mark.parametrize("N", [1, 31, 33, 257, 1000])
def test_scan_equals_the_twin(gpu, M, N):
    _check_scan(gpu, M, N)


def test_scan_at_the_lds_limit(gpu):
    _check_scan(gpu, 128, 300)  # D = 1024 at dsub 8: a 128 KiB table


@pytest.mark.parametrize("M,N", [(4, 1000), (16, 257), (16, 1000)])
def test_scan_orders_equal_scores_by_id_across_lanes_waves_and_splits(gpu, M, N):
    lut, codes, (ws, wi) = _scan_case(M, N, ints=True)
    assert (ws[:, 1:] == ws[:, :-1]).float().mean() > 0.5  # ties dominate
    assert (ws[:, 0] == 0).all() and (_bits(ws[:, 0]) != 0).all() and wi[:, 0].tolist() == [7] * 33  # row 0: -0.0
    assert (wi[:, 1:] > wi[:, :-1])[ws[:, 1:] == ws[:, :-1]].all()  # equal scores (+0.0 == -0.0): ascending id
    _check_scan(gpu, M, N, ints=True)


def test_sim_topk_pq_is_the_lut_then_the_scan(gpu):
    D, M = 64, 16
    b = _books(D, M)
    x, _ = _rows(D, M, 1000)
    q = x[:9].contiguous()
    codes = ops.pq_encode_ref(x, b, ops.pq_bias(b))
    ws, wi = ops.sim_topk_pq_ref(q, b, codes, 10, 100)
    s, i = ops.sim_topk_pq(q.to(gpu), b.to(gpu), codes.to(gpu), 10, 100)
    assert torch.equal(i.cpu(), wi) and torch.equal(_bits(s), _bits(ws))
    assert i[5, 0] == 105  # a row made of codewords reconstructs itself


# --------------------------------------------------------------------------------------------- the op
def _blobs(N, D, seed):
    gen = torch.Generator().manual_seed(seed)
    cent = torch.randn(24, D, generator=gen) * 2
    return (cent[torch.randint(0, 24, (N,), generator=gen)] + 0.5 * torch.randn(N, D, generator=gen)).contiguous()


def _signs(N, D, seed):
    gen = torch.Generator().manual_seed(seed)
    c = torch.zeros(N, D)
    for r in range(N):
        c[r, torch.randperm(D, generator=gen)[:16]] = torch.randint(0, 2, (16,), generator=gen).float() * 2 - 1
    return c


@pytest.mark.parametrize("metric", ["dot", "cosine"])
def test_map_search_with_compression_on_the_gpu_engine_equals_the_cpu_engine(gpu, tmp_path, monkeypatch, metric):
    """A 1000-row, D = 64 file. ``dot``: Gaussian blobs as they are. ``cosine``: rows of sixteen +-1 entries, whose
    normalisation (a division by 4) is exact on either device. Training, encoding and the scan then give the same
    codebooks, codes, ids and score bits on both engines."""
    from agent_tpu_amd.runtime import pq
    from agent_tpu_amd.runtime import search as rs
    from ops.map_search import map_search

    monkeypatch.delenv("SEARCH_INDEX_DTYPE", raising=False)
    rs.clear_cache()
    N, D, M = 1000, 64, 16
    c = _blobs(N, D, 5) if metric == "dot" else _signs(N, D, 6)
    q = torch.cat([c[3:4], c[500:507]])
    path = str(tmp_path / "corpus.npy")
    np.save(path, c.numpy())
    job = {"query_vectors": q.tolist(), "corpus_uri": path, "top_k": 10, "metric": metric,
           "compression": {"type": "pq", "subvectors": M, "train_rows": 512, "train_iterations": 4}}
    try:
        monkeypatch.setenv("CLASSIFY_DEVICE", "cpu")
        cpu = map_search(dict(job))
        monkeypatch.delenv("CLASSIFY_DEVICE")
        dev = map_search(dict(job))
        again = map_search(dict(job, top_k=3))
        assert dev["ids"] == cpu["ids"] and dev["scores"] == cpu["scores"]
        assert dev["compression"] == cpu["compression"] == {"type": "pq", "subvectors": M, "train_rows": 512,
                                                            "train_iterations": 4, "bytes_per_row": M}
        assert dev["index_cached"] is False and again["index_cached"] is True
        assert again["ids"] == [r[:3] for r in dev["ids"]]
        a = pq.load_index(path, 0, -1, torch.device("cpu"), M, 512, 4, metric == "cosine")
        b = pq.load_index(path, 0, -1, gpu, M, 512, 4, metric == "cosine")
        assert a.cached and b.cached and b.codes.is_cuda and b.codes.shape == (16, M // 4, 64, 4)
        assert torch.equal(_bits(a.codebooks), _bits(b.codebooks))
        assert torch.equal(pq.row_major_codes(b).cpu(), a.codes)
    finally:
        rs.clear_cache()
