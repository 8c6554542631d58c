"""binary_pack and hamming_scan (csrc/kernels/sim_binary.hip) against a plain float64 reference: equality everywhere.

The reference does not use the PyTorch twins: the bits are unpacked to +-1 in float64, the scores are the matrix
product (exact integers), and the total order is the stable descending sort by score of rows in ascending id. Rows
are drawn from a pool of N / 3 distinct rows, so whole rows duplicate (integer scores tie heavily anyway); some
entries equal the threshold exactly and some are -0.0 (both pack to 0 against a zero threshold).
"""
import numpy as np
import pytest
import torch

from agent_tpu_amd import ops

pytestmark = pytest.mark.gpu

NO_ROW = 0x7fffffff
BIG = 9000  # 141 blocks: a part spans several wave steps, several splits, a last block of 40 rows
_cache = {}


def _data(D, N, kind="zero"):
    """(x [N, D], thr [D], q [33, D], row bits, query bits as int32 words [., D / 32]) on the CPU."""
    key = (D, N, kind)
    if key not in _cache:
        gen = torch.Generator().manual_seed(D + N)
        pool = torch.randn(max(N // 3, 1), D, generator=gen)
        x = pool[torch.randint(0, pool.shape[0], (N,), generator=gen)].contiguous()
        thr = torch.zeros(D) if kind == "zero" else 0.1 * torch.randn(D, generator=gen)
        x[::5, ::7] = thr[::7]  # equal to the threshold: not above it
        x[1::5, 3::11] = -0.0
        q = (x[torch.randint(0, N, (33,), generator=gen)] + 0.5 * torch.randn(33, D, generator=gen)).contiguous()
        _cache[key] = (x, thr, q, _words(x, thr), _words(q, thr))
    return _cache[key]


def _words(x, thr):
    bits = (x.double() > thr.double()[None, :]).numpy()
    return torch.from_numpy(np.packbits(bits, axis=1, bitorder="little").view("<i4").copy())


def _scores(qw, cw):
    """float64 [nq, N]: the +-1 dot products of the unpacked words."""
    pm = lambda w: torch.from_numpy(  # noqa: E731
        np.unpackbits(w.numpy().view(np.uint8), axis=1, bitorder="little").astype(np.float64)) * 2 - 1
    return pm(qw) @ pm(cw).T


def _topk(s, k):
    order = torch.sort(s, dim=1, descending=True, stable=True).indices[:, :k]  # ids ascend: ties keep the lower id
    return torch.gather(s, 1, order), order


@pytest.mark.parametrize("n", [1, 64, 300])
@pytest.mark.parametrize("D", [64, 768, 1024])
def test_pack_words_and_padding(gpu, D, n):
    for kind in ("zero", "random"):
        x, thr, _, want, _ = _data(D, 300, kind)
        x, want = x[:n].contiguous(), want[:n]
        got = ops.binary_pack(x.to(gpu), thr.to(gpu))
        assert got.dtype == torch.int32 and torch.equal(got.cpu(), want), kind
        bc = ops.binary_pack(x.to(gpu), thr.to(gpu), interleave=True)
        nb = -(-n // 64)
        full = torch.cat([want, torch.zeros(nb * 64 - n, D // 32, dtype=torch.int32)])  # the padding rows are zero
        assert bc.rows == n and bc.D == D and bc.data.shape == (nb, D // 32, 64)
        assert torch.equal(bc.data.cpu(), full.view(nb, 64, D // 32).permute(0, 2, 1)), kind
        assert kind != "zero" or (want != 0).any()


@pytest.mark.parametrize("k", [1, 10, 32])
@pytest.mark.parametrize("nq", [1, 33])
@pytest.mark.parametrize("N", [300, BIG])
@pytest.mark.parametrize("D", [64, 768, 1024])
def test_scan_topk_is_exact_for_every_split(gpu, D, N, nq, k):
    _, _, _, cw, qw = _data(D, N)
    qw = qw[:nq].contiguous()
    ws, wi = _topk(_scores(qw, cw), k)
    codes = ops.binary_interleave(cw.to(gpu))
    for splits in (1, 3, None):
        s, i = ops.hamming_scan_topk(qw.to(gpu), codes, D, k, id_base=1000, splits=splits)
        assert s.shape == i.shape == (nq, k) and s.dtype == torch.float32 and i.dtype == torch.int64
        assert torch.equal(i.cpu(), wi + 1000), (splits, (i.cpu() != wi + 1000).nonzero()[:4])
        assert torch.equal(s.cpu().double(), ws), splits
    assert k < 10 or (ws[:, 1:] == ws[:, :-1]).any()  # the data does tie


def test_fewer_rows_than_k(gpu):
    _, _, _, cw, qw = _data(768, 300)
    cw = cw[:20].contiguous()
    ws, wi = _topk(_scores(qw, cw), 32)
    s, i = ops.hamming_scan_topk(qw.to(gpu), cw.to(gpu), 768, 32, id_base=1000)  # row-major codes: interleaved inside
    assert s.shape == (33, 20) and torch.equal(i.cpu(), wi + 1000) and torch.equal(s.cpu().double(), ws)


@pytest.mark.parametrize("G", [1, 3, 8])
@pytest.mark.parametrize("N", [280, 300, BIG])  # 280: at G = 8 the last segment has 24 rows
def test_segments_equal_the_per_segment_reference(gpu, N, G):
    D = 768
    x, _, q, cw, qw = _data(D, N)
    s = _scores(qw, cw)
    seg = ops.segment_rows(N, G)
    P = -(-N // seg)
    want = torch.full((33, P, 32), NO_ROW, dtype=torch.int64)
    for p in range(P):
        order = _topk(s[:, p * seg:min(N, (p + 1) * seg)], 32)[1]
        want[:, p, :order.shape[1]] = order + p * seg
    want = want.view(33, P * 32)
    if (N, G) == (280, 8):
        assert (want[:, -8:] == NO_ROW).all() and (want[:, -9] != NO_ROW).all()
    codes = ops.binary_interleave(cw.to(gpu))
    for parts in (1, 2, 5, None):
        cand = ops.hamming_scan_segments(qw.to(gpu), codes, D, G, parts=parts)
        assert cand.dtype == torch.int32 and cand.shape == (33, P * 32) and cand.stride(1) == 2
        assert torch.equal(cand.cpu().long(), want), (parts, (cand.cpu() != want).nonzero()[:4])
    live = [row[row != NO_ROW] for row in want]
    assert all(len(set(r.tolist())) == len(r) for r in live)  # no duplicates
    if (N, G) == (BIG, 8):  # the list as it lies (stride 2) into the exact re-scoring; integer data: exact in any order
        xi, qi = (x * 2).round().clamp(-2, 2), (q * 2).round().clamp(-2, 2)
        got = ops.refine_topk(qi.to(gpu), xi.to(gpu), cand, 10)
        ref = ops.refine_topk_ref(qi, xi, cand.cpu().contiguous(), 10, dtype=torch.float64)
        assert torch.equal(got[1].cpu(), ref[1]) and torch.equal(got[0].cpu().double(), ref[0])
