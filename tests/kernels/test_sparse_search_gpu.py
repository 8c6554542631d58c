"""sparse_index_build and sparse_scan_topk (csrc/kernels/sparse_index.hip) against plain int64 math: equality everywhere.

The scan's reference does not use the index: per query, c = rint(double(wq) * double(fp16(wd)) * 2^32) of every CSR
entry whose token the query has, summed per row in int64; score = float(acc) * 2^-32 and the total order is the stable
descending sort of rows in ascending id. Corpus (per N, V): every 7th row empty (N < 8192 or rows past the first
block), row 1 with 1024 terms, token V - 1 with a kept weight in every row of the first block at N >= 8192 (a segment
of exactly 32 full chunks; in the rows with terms below that),
tokens V - 2 and V - 3 never used, tokens 2..4 with weight 1.0 wherever they occur (ties), every 11th weight 1e-9 (fp16
zero: dropped) and every 13th 1e-7 (an fp16 denormal); the rest random fp32, so fp16-inexact.
"""
import pytest
import torch

from agent_tpu_amd import ops

pytestmark = pytest.mark.gpu

R = 8192
SIZES = [1, R - 1, R + 1, 3 * R + 5]
VOCABS = [1, 70, 30522]
_cache = {}


def _csr(keys, w, n, V):
    keys = torch.unique(keys)  # sorted: by row, then token
    row, tok = keys // V, (keys % V).to(torch.int32)
    indptr = torch.zeros(n + 1, dtype=torch.int64)
    indptr[1:] = torch.cumsum(torch.bincount(row, minlength=n), 0)
    return indptr, tok.contiguous(), w[:tok.numel()].contiguous()


def _corpus(N, V):
    gen = torch.Generator().manual_seed(1000 * N + V)
    free = max(V - 3, 1)  # tokens the random draws use
    lens = torch.randint(0, 41, (N,), generator=gen)
    r = torch.arange(N)
    lens[(r % 7 == 3) & ((N < R) | (r >= R))] = 0
    row = torch.repeat_interleave(r, lens)
    tok = (free * torch.rand(row.numel(), generator=gen) ** 3).long().clamp_(max=free - 1)  # skewed to low ids
    keys = [row * V + tok, (r[:R] if N >= R else r[lens > 0]) * V + (V - 1)]
    if V >= 1024 and N > 1:
        keys = [k[k // V != 1] for k in keys] + [V + torch.randperm(free, generator=gen)[:1023], torch.tensor([2 * V - 1])]
    keys = torch.cat(keys)
    w = 3 * torch.rand(keys.numel(), generator=gen) + 1e-3
    w[::11], w[5::13] = 1e-9, 1e-7
    indptr, tok, w = _csr(keys, w, N, V)
    w[(tok >= 2) & (tok <= 4)] = 1.0
    w[tok == V - 1] = 0.75  # kept: at N >= 8192 its segment in the first block is 8192 postings, 32 full chunks
    return indptr, tok, w


def _queries(V, gen):
    """One batch as CSR: the module docstring's cases; for V = 1 the only token, twice, and a query without terms."""
    if V == 1:
        terms = [([0], [0.7]), ([0], [1.0]), ([], [])]
    else:
        free = V - 3
        many = torch.randperm(V, generator=gen)[:1024].tolist()
        some = torch.randperm(free, generator=gen)[:50].tolist()
        rnd = lambda n: (4 * torch.rand(n, generator=gen) + 1e-4).tolist()  # noqa: E731
        terms = [([7], rnd(1)), (many, rnd(len(many))), ([V - 1], [0.37]), ([V - 2, 5], rnd(2)),
                 ([V - 2, V - 3], rnd(2)), ([2, 3, 4], [1.0, 1.0, 2.0]), (some, rnd(50)), ([], [])]
    q_ptr = torch.tensor([0] + [len(t) for t, _ in terms], dtype=torch.int64).cumsum(0)
    return (q_ptr, torch.tensor([x for t, _ in terms for x in t], dtype=torch.int32),
            torch.tensor([x for _, w in terms for x in w], dtype=torch.float32))


def _acc(indptr, tok, w, q_ptr, q_tok, q_w, V):
    """int64 [nq, N]: the integer sums, from the CSR rows."""
    N, nq = indptr.numel() - 1, q_ptr.numel() - 1
    row = torch.repeat_interleave(torch.arange(N), indptr[1:] - indptr[:-1])
    wd = w.to(torch.float16).to(torch.float64)
    acc = torch.zeros(nq, N, dtype=torch.int64)
    for i in range(nq):
        a, b = int(q_ptr[i]), int(q_ptr[i + 1])
        wq = torch.zeros(V, dtype=torch.float64)
        wq[q_tok[a:b].long()] = q_w[a:b].double()
        acc[i].index_add_(0, row, torch.round(wq[tok.long()] * wd * 2.0 ** 32).to(torch.int64))
    return acc


def _case(N, V, gpu):
    if (N, V) not in _cache:
        indptr, tok, w = _corpus(N, V)
        q = _queries(V, torch.Generator().manual_seed(N + V))
        acc = _acc(indptr, tok, w, *q, V)
        s = torch.where(acc > 0, acc.to(torch.float32) * 2.0 ** -32, torch.tensor(float("-inf")))
        order = torch.sort(s, dim=1, descending=True, stable=True).indices  # ids ascend: ties keep the lower id
        index = ops.sparse_index_build(indptr.to(gpu), tok.to(gpu), w.to(gpu), V)
        _cache[(N, V)] = ((indptr, tok, w), q, torch.gather(s, 1, order), order, index)
    return _cache[(N, V)]


def _segments(index):
    """The words sorted inside every (block, token) segment."""
    seg = (index.offsets[:, 1:] - index.offsets[:, :-1]).reshape(-1).long()
    sid = torch.repeat_interleave(torch.arange(seg.numel()), seg)
    return torch.sort(sid * 2 ** 32 + (index.postings.long() & 0xffffffff)).values


@pytest.mark.parametrize("V", VOCABS)
@pytest.mark.parametrize("N", SIZES)
def test_build_equals_the_twin(gpu, N, V):
    (indptr, tok, w), _, _, _, got = _case(N, V, gpu)
    want = ops.sparse_index_build_ref(indptr, tok, w, V)
    got = ops.SparseIndex(got.postings.cpu(), got.offsets.cpu(), got.block_start.cpu(), got.rows, got.V)
    assert (got.rows, got.V) == (N, V) and got.offsets.shape == (-(-N // R), V + 1)
    assert torch.equal(got.offsets, want.offsets) and torch.equal(got.block_start, want.block_start)
    assert torch.equal(_segments(got), _segments(want))
    kept = w.to(torch.float16) != 0
    assert got.nnz == int(kept.sum()) and (V == 1 or not kept.all())  # the fp16 zeros are dropped (V = 1: the kept token alone)
    assert N < R or int(got.offsets[0, V] - got.offsets[0, V - 1]) == R  # the full segment: 32 whole chunks
    lens = indptr[1:] - indptr[:-1]
    assert int(lens.max()) == 1024 or V < 1024 or N == 1
    assert int((lens == 0).sum()) > 0 or N in (1, R + 1)


@pytest.mark.parametrize("k", [1, 8, 32])
@pytest.mark.parametrize("V", VOCABS)
@pytest.mark.parametrize("N", SIZES)
def test_scan_equals_the_int64_reference(gpu, N, V, k):
    _, q, ws, wi, index = _case(N, V, gpu)
    nq = q[0].numel() - 1
    hits = (ws > float("-inf")).sum(1)
    want_n = hits.clamp(max=k)
    live = torch.arange(k)[None, :] < want_n[:, None]
    kk = min(k, N)
    want_s = torch.full((nq, k), float("-inf"))
    want_i = torch.full((nq, k), ops.search.PAD_ID)
    want_s[:, :kk] = torch.where(live[:, :kk], ws[:, :kk], want_s[:, :kk])
    want_i[:, :kk] = torch.where(live[:, :kk], wi[:, :kk] + 1000, want_i[:, :kk])
    qd = [t.to(gpu) for t in q]
    for splits in (1, 3, None):
        s, i, n = ops.sparse_scan_topk(index, *qd, k, id_base=1000, splits=splits)
        assert s.shape == i.shape == (nq, k) and s.dtype == torch.float32 and i.dtype == torch.int64
        assert torch.equal(n.cpu(), want_n), splits
        assert torch.equal(i.cpu(), want_i), (splits, (i.cpu() != want_i).nonzero()[:4])
        assert torch.equal(s.cpu(), want_s), splits
    assert int(want_n[-1]) == 0 and (V == 1 or int(want_n[4]) == 0)  # the queries without a hit: padding only
    if V > 1 and N > 1 and k > 1:
        assert (want_s[5, 1:] == want_s[5, :-1]).any()  # the integer weights tie
        a, b = int(q[0][1]), int(q[0][2])  # the 1024-term query alone: the same bits as in the batch
        s1, i1, n1 = ops.sparse_scan_topk(index, torch.tensor([0, b - a], device=gpu), qd[1][a:b].contiguous(),
                                          qd[2][a:b].contiguous(), k, id_base=1000)
        assert torch.equal(s1[0], s[1]) and torch.equal(i1[0], i[1]) and int(n1[0]) == int(n[1])


def test_text_search_end_to_end(gpu, tmp_path):
    """The ops on the GPU: map_sparse_embed writes 40 texts as the npz (min_weight applied, tokens sorted), then
    map_sparse_search's text form equals the int64 reference computed from the file and the engine's own tok / w of
    the queries, and every text retrieves itself."""
    import numpy as np

    from agent_tpu_amd.runtime import search as rs
    from agent_tpu_amd.utils.synthetic import make_text_rows
    from ops import get_op
    from ops._gpu_runtime import get_gpu_handle

    model = "bert-tiny?mlm=1&batch=8&seq=40&seed=3"
    h = get_gpu_handle(model, gpu)
    texts, path = make_text_rows(40, words_per_row=9, seed=5), str(tmp_path / "rows.npz")
    wrote = get_op("map_sparse_embed")({"texts": texts, "model_path": model, "max_terms": 64, "min_weight": 0.25,
                                        "output": "npz", "output_uri": path})
    rs.clear_cache()
    out = get_op("map_sparse_search")({"corpus_uri": path, "queries": texts, "model_path": model, "top_k": 8,
                                       "max_query_terms": 48})
    rs.clear_cache()
    with np.load(path, allow_pickle=False) as z:
        indptr, indices, data = (torch.from_numpy(z[n]) for n in ("indptr", "indices", "data"))
    V = int(h.cfg.vocab_size)
    assert wrote["shape"] == [40, V] and wrote["stored"] == data.numel() and float(data.min()) >= 0.25
    assert (out["corpus_rows"], out["vocab_size"], out["nnz"], out["row_count"]) == (40, V, data.numel(), 40)
    tok, _, w, _ = (t.cpu() for t in h.engine.sparse_rows(texts, 48))
    live = tok >= 0
    q_ptr = torch.zeros(41, dtype=torch.int64)
    q_ptr[1:] = torch.cumsum(live.sum(1), 0)
    acc = _acc(indptr, indices, data, q_ptr, tok[live], w[live], V)
    ref = torch.where(acc > 0, acc.to(torch.float32) * 2.0 ** -32, torch.tensor(float("-inf")))
    order = torch.sort(ref, dim=1, descending=True, stable=True).indices[:, :8]
    for i, r in enumerate(out["results"]):
        n = int((ref[i, order[i]] > float("-inf")).sum())
        assert (r["hits"], r["ids"], r["scores"]) == (n, order[i, :n].tolist(), ref[i, order[i, :n]].tolist()), i
        assert i in r["ids"]
