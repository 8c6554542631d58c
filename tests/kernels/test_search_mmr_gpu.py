"""mmr_select and rows_gather (csrc/kernels/sim_mmr.hip) against a plain fp64 loop, and map_search's ``diversify``.

Exact data: test_search_gpu.py's integer operands with duplicated rows, power-of-two row scales and lambda in
{0.25, 0.5, 0.75}: the Gram matrix and ``rel * lam - mu * pen`` are exact in fp32, so picks and values must equal the
fp64 loop's bit for bit, ties included. Random data: with test_search_gpu.py's fma-chain bound
``tol = D * 2^-24 * sum_k |a_k b_k|`` of one dot product, a candidate's ``v`` inherits ``lam * tol(rel) + mu * tol(G)``
(the max over the picks moves by at most the largest tolerance among them); replayed along the kernel's own picks in
fp64, every pick's ``v`` is within the two candidates' tolerances of the fp64 best and the reported value within its
own. Nothing is excluded."""
import numpy as np
import pytest
import torch

from agent_tpu_amd import ops
from agent_tpu_amd.ops.search import PAD_ID

from test_search_gpu import U, _exact_case, _random_case

pytestmark = pytest.mark.gpu

NO_ROW = 0x7fffffff
F32, F16, F16S = "float32", "float16", "float16+scale"


def _store(c, form, gpu):
    # (store, row_scale) on the device, and the fp64 scale the reference uses
    if form == F32:
        return c.to(gpu), None, torch.ones(c.shape[0], dtype=torch.float64)
    if form == F16:
        return c.half().to(gpu), None, torch.ones(c.shape[0], dtype=torch.float64)
    scale = 2.0 ** ((torch.arange(c.shape[0]) * 5) % 7 - 3).float()
    return c.half().to(gpu), scale.to(gpu), scale.double()


def _candidates(q, store, scale, R, gpu):
    # sim_topk's top-R as mmr_select takes it: (rel, cand int32) padded to R columns with (0, no row)
    s, i = ops.sim_topk(q.to(gpu), store, R, row_scale=scale)
    pad = R - s.shape[1]
    return (torch.nn.functional.pad(s, (0, pad)).contiguous(),
            torch.nn.functional.pad(i.to(torch.int32), (0, pad), value=NO_ROW).contiguous())


def _fp64_picks(rel, rows, c, scale, lam, k):
    """One query, a dozen plain lines: fp64 Gram, then greedy arg-max with (v desc, id asc)."""
    C = c.double()[rows] * 1.0
    G = (C @ C.T) * (scale[rows][:, None] * scale[rows][None, :])
    picked, out = [], []
    for _ in range(min(k, len(rows))):
        pen = [max(G[j][p].item() for p in picked) if picked else 0.0 for j in range(len(rows))]
        v = [lam * rel[j] - (1.0 - lam) * pen[j] if picked else lam * rel[j] for j in range(len(rows))]
        best = min((j for j in range(len(rows)) if j not in picked), key=lambda j: (-v[j], rows[j]))
        picked.append(best)
        out.append((rows[best], v[best]))
    return out


EXACT = [  # (D, R, k, form, nq, N, id_base)
    (64, 2, 1, F32, 1, 40, 0), (64, 2, 2, F16, 3, 40, 0), (64, 17, 9, F16S, 3, 40, 0),
    (768, 16, 1, F32, 3, 100, 0), (768, 16, 7, F16S, 1, 100, 0), (768, 16, 16, F16, 3, 100, 12345),
    (768, 17, 17, F32, 3, 100, 0), (768, 17, 5, F16, 1, 100, 0),
    (768, 32, 32, F32, 3, 100, 12345), (768, 32, 10, F16S, 3, 100, 0), (768, 32, 32, F32, 3, 5, 0),
    (192, 32, 32, F16, 1, 100, 0),  # fp16 with a two-chunk tail step after a full one
    (1024, 32, 1, F16, 1, 100, 0), (1024, 32, 32, F16S, 3, 100, 0), (1024, 17, 8, F32, 1, 100, 0),
]


@pytest.mark.parametrize("D,R,k,form,nq,N,id_base", EXACT)
def test_exact_integer_data_equals_the_fp64_loop(gpu, D, R, k, form, nq, N, id_base):
    q, c = _exact_case(D, N, nq)
    store, scale, s64 = _store(c, form, gpu)
    rel, cand = _candidates(q, store, scale, R, gpu)
    lam = (0.25, 0.5, 0.75)[(D // 64 + R + k) % 3]
    ids, scores, mmr = ops.mmr_select(rel, cand, store, k, lam, id_base=id_base, row_scale=scale)
    assert ids.shape == scores.shape == mmr.shape == (nq, k) and ids.dtype == torch.int64
    later = 0
    for a in range(nq):
        rows = [r for r in cand[a].tolist() if r != NO_ROW]
        assert len(rows) == min(R, N)
        want = _fp64_picks(rel[a].double().tolist(), rows, c, s64, lam, k)
        live = len(want)
        assert ids[a, :live].tolist() == [id_base + r for r, _ in want], a
        assert mmr[a, :live].double().tolist() == [v for _, v in want], a
        assert scores[a, :live].tolist() == [rel[a, rows.index(r)].item() for r, _ in want], a
        assert (ids[a, live:] == PAD_ID).all() and (scores[a, live:] == float("-inf")).all() \
            and (mmr[a, live:] == float("-inf")).all()
        if k == R and N > R and scale is None:  # a copy of the first pick comes later than the plain order has it
            first = rows[0]
            twins = [r for r in rows[1:] if torch.equal(c[r], c[first])]
            picks = [r for r, _ in want]
            later += sum(picks.index(r) > rows.index(r) for r in twins)
            assert all(picks.index(r) >= rows.index(r) for r in twins)
    assert later > 0 or not (k == R == 32 and N > R and nq == 3 and scale is None)


def test_identities(gpu):
    q, c = _random_case(400, 3, dup=True, seed=4)
    dc = c.to(gpu)
    rel, cand = _candidates(q, dc, None, 32, gpu)
    ids, scores, mmr = ops.mmr_select(rel, cand, dc, 32, 1.0)  # lambda = 1: sim_topk's list
    assert torch.equal(ids, cand.to(torch.int64)) and torch.equal(scores, rel) and torch.equal(mmr, rel)
    full = ops.mmr_select(rel, cand, dc, 32, 0.5)
    assert not torch.equal(full[0], ids)
    for k in (1, 10, 31):  # the prefix property
        part = ops.mmr_select(rel, cand, dc, k, 0.5)
        assert all(torch.equal(p, f[:, :k]) for p, f in zip(part, full)), k
    for a in range(3):  # alone and inside the batch
        one = ops.mmr_select(rel[a:a + 1].contiguous(), cand[a:a + 1].contiguous(), dc, 32, 0.5)
        assert all(torch.equal(o[0], f[a]) for o, f in zip(one, full)), a
    # lambda = 0: the second pick's value is -G[pick][first], and G has sim_topk's bits (refine_topk's, for a pair)
    i0, _, m0 = ops.mmr_select(rel, cand, dc, 2, 0.0)
    for a in range(3):
        pair = torch.full((1, 32), NO_ROW, dtype=torch.int32, device=gpu)
        pair[0, 0] = i0[a, 1]
        g = ops.refine_topk(dc[i0[a, 0]][None].contiguous(), dc, pair, 1)[0]
        assert i0[a, 0] == cand[a].min() and m0[a, 0] == 0 and torch.equal(m0[a, 1:2], -g[0]), a
    empty = ops.mmr_select(rel[:0].contiguous(), cand[:0].contiguous(), dc, 4, 0.5)
    assert [t.shape for t in empty] == [(0, 4)] * 3 and empty[0].is_cuda
    for k, lam in ((33, 0.5), (0, 0.5), (4, 1.5)):
        with pytest.raises(ValueError):
            ops.mmr_select(rel, cand, dc, k, lam)


@pytest.mark.parametrize("form", [F32, F16])
def test_random_data_within_the_fma_chain_bound(gpu, form):
    D, R, k, lam = 768, 32, 10, 0.5
    q, c = _random_case(400, 3, dup=True, seed=5)
    store, _, _ = _store(c, form, gpu)
    rel, cand = _candidates(q, store, None, R, gpu)
    ids, _, mmr = ops.mmr_select(rel, cand, store, k, lam)
    cs, qd = store.cpu().double(), q.double()
    worst = 0.0
    for a in range(3):
        rows = cand[a].tolist()
        C = cs[rows]
        rel64, rel_tol = C @ qd[a], D * U * (C.abs() @ qd[a].abs())
        G, G_tol = C @ C.T, D * U * (C.abs() @ C.abs().T)
        picked = []
        for t in range(k):
            if picked:
                pen, at = G[:, picked].max(1)
                v = lam * rel64 - (1 - lam) * pen
                tol = lam * rel_tol + (1 - lam) * G_tol[:, picked].max(1).values
            else:
                v, tol = lam * rel64, lam * rel_tol
            j = rows.index(ids[a, t].item())
            assert j not in picked
            left = [x for x in range(R) if x not in picked]
            b = max(left, key=lambda x: v[x].item())
            assert v[j] >= v[b] - tol[j] - tol[b], (a, t)
            err = abs(mmr[a, t].item() - v[j].item())
            worst = max(worst, err / tol[j].item())
            assert err <= tol[j], (a, t)
            picked.append(j)
    print(f"random data ({form}): worst |mmr - fp64| / tolerance {worst:.4f}")


@pytest.mark.parametrize("form", [F32, F16S])
def test_rows_gather(gpu, form):
    _, c = _exact_case(192, 100, 1)
    store, scale, _ = _store(c, form, gpu)
    ids = torch.tensor([1007, 1000, 1099, 999, 1100, 1050, PAD_ID, 1007, 0], dtype=torch.int64, device=gpu)
    out, sc = ops.rows_gather(ids, store, id_base=1000, row_scale=scale)
    rows = (ids - 1000).cpu()
    ok = (rows >= 0) & (rows < 100)
    want = torch.where(ok[:, None], store.cpu()[rows.clamp(0, 99)], torch.zeros((), dtype=store.dtype))
    assert out.dtype == store.dtype and torch.equal(out.cpu(), want) and (~ok).sum() == 4
    if scale is None:
        assert sc is None
    else:
        assert torch.equal(sc.cpu(), torch.where(ok, scale.cpu()[rows.clamp(0, 99)], torch.ones(())))


@pytest.mark.parametrize("corpus_dtype", ["float32", "float16"])
def test_map_search_diversify_on_the_gpu_engine_equals_the_cpu_engine(gpu, tmp_path, monkeypatch, corpus_dtype):
    from agent_tpu_amd.runtime import search as rs
    from ops.map_search import map_search

    q, c = _exact_case(768, 100, 3)
    path = str(tmp_path / "exact.npy")
    np.save(path, c.numpy())
    job = {"query_vectors": q.tolist(), "corpus_uri": path, "top_k": 10, "metric": "dot", "corpus_dtype": corpus_dtype,
           "diversify": {"lambda": 0.25, "candidates": 24}}
    out = {}
    for dev in ("gpu", "cpu"):
        if dev == "cpu":
            monkeypatch.setenv("CLASSIFY_DEVICE", "cpu")
        else:
            monkeypatch.delenv("CLASSIFY_DEVICE", raising=False)
        rs.clear_cache()
        out[dev] = map_search(dict(job))
    rs.clear_cache()
    for key in ("ids", "scores", "mmr_scores", "diversify"):
        assert out["gpu"][key] == out["cpu"][key], key
    assert out["gpu"]["ids"] != map_search(dict(job, diversify={"lambda": 1}))["ids"]
