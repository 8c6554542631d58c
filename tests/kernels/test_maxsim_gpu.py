"""``maxsim`` and ``token_unit`` (csrc/kernels/maxsim.hip) on the GPU: bit-equal to the twin on exactly
representable inputs, blind to what padding rows hold, clamped indices, the same bits wherever a pair sits
in a launch, random unit vectors within the derived bound, and the engine's late-interaction scores end to
end on ``bert-tiny?late=64``.

Shapes: S = 20 leaves a tail in both token dimensions (two 16-token query tiles, one 32-token passage
step with 12 dead rows); P = 64 is one load step, P = 192 three (an odd count for the two-buffer prefetch);
lengths from {1, 2, 15, 16, 17, 20}; ``qidx`` not monotone.

Bounds. ``maxsim`` against its fp32 twin or an fp64 loop on unit vectors: a dot product errs by at most
about ``P * 2^-24``, the sum of ``len_q`` terms of magnitude at most 1 adds ``len_q * 2^-24`` each, so
``|err| <= len_q * (P + len_q) * 2^-23``. ``token_unit``: ``(P + 8) * 2^-24`` per element."""
import functools

import numpy as np
import pytest
import torch

from agent_tpu_amd import ops
from agent_tpu_amd.ops.maxsim import maxsim_ref, token_unit_ref

pytestmark = pytest.mark.gpu

S, QN, DN = 20, 3, 5
LENS = (1, 2, 15, 16, 17, 20)
QIDX = [2, 0, 1, 1, 2, 0, 0, 2, 1]  # not monotone
DIDX = [0, 4, 2, 3, 1, 1, 4, 3, 0]


def _bound(lens_q, qidx, P, S=S):
    lq = lens_q.long().clamp(1, S)[qidx.long().clamp(0, lens_q.numel() - 1)].double()
    return lq * (P + lq) * 2.0 ** -23


@functools.lru_cache(maxsize=None)
def _case(P, kind):
    """``(qv, lens_q, dv, lens_d)`` on the host, built once and never changed: ``kind`` "dyadic" (entries on
    the grid {-2..2}/4: every product, partial sum and final sum is exact in fp32, whatever the order) or
    "unit" (random unit rows)."""
    g = torch.Generator().manual_seed(P + (0 if kind == "dyadic" else 1))
    if kind == "dyadic":
        qv = torch.randint(-2, 3, (QN, S, P), generator=g).float() / 4
        dv = torch.randint(-2, 3, (DN, S, P), generator=g).float() / 4
    else:
        qv = torch.nn.functional.normalize(torch.randn(QN, S, P, generator=g), dim=-1)
        dv = torch.nn.functional.normalize(torch.randn(DN, S, P, generator=g), dim=-1)
    lens_q = torch.tensor([16, 20, 1], dtype=torch.int32)
    lens_d = torch.tensor([17, 2, 20, 15, 16], dtype=torch.int32)
    assert set(lens_q.tolist()) | set(lens_d.tolist()) == set(LENS)
    return qv, lens_q, dv, lens_d


def _loop64(qv, lens_q, dv, lens_d, qidx, didx):
    """The naive double loop in fp64."""
    q64, d64 = qv.double().numpy(), dv.double().numpy()
    out = []
    for a, b in zip(qidx.tolist(), didx.tolist()):
        total = 0.0
        for i in range(int(lens_q[a])):
            total += max(float(np.dot(q64[a, i], d64[b, j])) for j in range(int(lens_d[b])))
        out.append(total)
    return torch.tensor(out, dtype=torch.float64)


def _idx(n):
    return torch.tensor(QIDX[:n], dtype=torch.int32), torch.tensor(DIDX[:n], dtype=torch.int32)


def _run(gpu, qv, lens_q, dv, lens_d, qidx, didx, **kw):
    out = ops.maxsim(*(t.to(gpu) for t in (qv, lens_q, dv, lens_d, qidx, didx)), **kw)
    torch.cuda.synchronize()
    return out.cpu()


def _bits(t):
    return t.view(torch.int32)


@pytest.mark.parametrize("P", [64, 192])
@pytest.mark.parametrize("n", [1, 5, 9])
def test_exact_inputs_are_bit_equal_to_the_twin(gpu, P, n):
    case = _case(P, "dyadic")
    qidx, didx = _idx(n)
    ref = maxsim_ref(*case, qidx, didx)
    assert torch.equal(ref.double(), _loop64(*case, qidx, didx))  # the twin is exact on these inputs
    got = _run(gpu, *case, qidx, didx)
    assert got.dtype == torch.float32 and got.shape == (n,)
    assert torch.equal(_bits(got), _bits(ref)), (got, ref)
    buf = torch.full((n,), -7.0, device=gpu)  # the out= form writes the given tensor
    _run(gpu, *case, qidx, didx, out=buf)
    assert torch.equal(_bits(buf.cpu()), _bits(ref))


@pytest.mark.parametrize("P", [64, 192])
@pytest.mark.parametrize("poison", [float("nan"), 1e30])
def test_padding_rows_never_reach_a_score(gpu, P, poison):
    qv, lens_q, dv, lens_d = _case(P, "dyadic")
    qidx, didx = _idx(9)
    clean = _run(gpu, qv, lens_q, dv, lens_d, qidx, didx)
    pq, pd = qv.clone(), dv.clone()
    pq[torch.arange(S).view(1, S) >= lens_q.view(-1, 1)] = poison
    pd[torch.arange(S).view(1, S) >= lens_d.view(-1, 1)] = poison
    assert not torch.equal(pq, qv) and not torch.equal(pd, dv)
    got = _run(gpu, pq, lens_q, pd, lens_d, qidx, didx)
    assert torch.equal(_bits(got), _bits(clean)), (got, clean)


@pytest.mark.parametrize("P", [64, 192])
def test_indices_and_lens_are_clamped(gpu, P):
    qv, lens_q, dv, lens_d = _case(P, "dyadic")
    qidx = torch.tensor([-1, QN + 5, 1, 0], dtype=torch.int32)
    didx = torch.tensor([DN + 5, -1, -1, DN + 5], dtype=torch.int32)
    got = _run(gpu, qv, lens_q, dv, lens_d, qidx, didx)
    want = _run(gpu, qv, lens_q, dv, lens_d, qidx.clamp(0, QN - 1), didx.clamp(0, DN - 1))
    assert torch.equal(_bits(got), _bits(want))
    assert torch.equal(_bits(got), _bits(maxsim_ref(qv, lens_q, dv, lens_d, qidx, didx)))
    # lens out of [1, S]: clamped
    wild_q = torch.tensor([-3, S + 9, 0], dtype=torch.int32)
    wild_d = torch.tensor([0, S + 1, -1, 2**30, 5], dtype=torch.int32)
    a, b = _idx(9)
    got = _run(gpu, qv, wild_q, dv, wild_d, a, b)
    want = _run(gpu, qv, wild_q.clamp(1, S), dv, wild_d.clamp(1, S), a, b)
    assert torch.equal(_bits(got), _bits(want))


@pytest.mark.parametrize("P", [64, 192])
def test_a_pair_has_the_same_bits_wherever_it_sits(gpu, P):
    qv, lens_q, dv, lens_d = _case(P, "unit")
    one = torch.tensor([1], dtype=torch.int32), torch.tensor([2], dtype=torch.int32)  # lens 20 x 20
    alone = _run(gpu, qv, lens_q, dv, lens_d, *one)
    for pos in (0, 4, 8):  # first, in the middle and last of n = 9
        qidx, didx = _idx(9)
        qidx[pos], didx[pos] = 1, 2
        got = _run(gpu, qv, lens_q, dv, lens_d, qidx, didx)
        assert torch.equal(_bits(got[pos:pos + 1]), _bits(alone)), pos
    # Qn / Dn enlarged: more rows after the pair's own
    g = torch.Generator().manual_seed(7)
    qv2 = torch.cat([qv, torch.randn(4, S, P, generator=g)])
    dv2 = torch.cat([dv, torch.randn(6, S, P, generator=g)])
    lq2 = torch.cat([lens_q, torch.full((4,), 3, dtype=torch.int32)])
    ld2 = torch.cat([lens_d, torch.full((6,), 9, dtype=torch.int32)])
    assert torch.equal(_bits(_run(gpu, qv2, lq2, dv2, ld2, *one)), _bits(alone))


@pytest.mark.parametrize("P", [64, 192])
@pytest.mark.parametrize("n", [1, 5, 9])
def test_random_unit_vectors_within_the_bound(gpu, P, n):
    case = _case(P, "unit")
    qidx, didx = _idx(n)
    got = _run(gpu, *case, qidx, didx)
    ref = maxsim_ref(*case, qidx, didx)  # on the copied tensors
    err = (got.double() - ref.double()).abs()
    bound = _bound(case[1], qidx, P)
    err64 = (got.double() - _loop64(*case, qidx, didx)).abs()
    print(f"P={P} n={n}: max |gpu - twin| {err.max().item():.3e}, |gpu - fp64| {err64.max().item():.3e}, "
          f"min bound {bound.min().item():.3e}")
    assert (err <= bound).all() and (err64 <= bound).all()
    assert torch.equal(_bits(got), _bits(_run(gpu, *case, qidx, didx)))  # run to run


def test_shapes_the_wrapper_refuses(gpu):
    lens = torch.ones(1, dtype=torch.int32, device=gpu)
    idx = torch.zeros(1, dtype=torch.int32, device=gpu)
    for P in (96, 1088):  # not a multiple of 64; above 1024
        v = torch.zeros((1, 4, P), device=gpu)
        with pytest.raises(ValueError):
            ops.maxsim(v, lens, v, lens, idx, idx)
        with pytest.raises(ValueError):
            ops.token_unit(torch.zeros((4, P), device=gpu))
    v = torch.zeros((1, 4, 64), device=gpu)
    out = ops.maxsim(v, lens, v, lens, idx[:0], idx[:0])  # n == 0: no launch
    assert out.shape == (0,)
    assert ops.token_unit(torch.zeros((0, 64), device=gpu)).shape == (0, 64)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("M", [1, 37])
@pytest.mark.parametrize("P", [64, 192])
def test_token_unit_against_the_twin(gpu, dtype, M, P):
    g = torch.Generator().manual_seed(M * P)
    x = (torch.randn(M, P, generator=g) * 3).to(dtype)
    if M > 1:
        x[5] = 0  # a zero row stays zero: 0 / max(0, 1e-12)
    got = ops.token_unit(x.to(gpu))
    torch.cuda.synchronize()
    got = got.cpu()
    assert got.dtype == torch.float32 and got.shape == (M, P)
    bound = (P + 8) * 2.0 ** -24
    err = (got.double() - token_unit_ref(x).double()).abs().max().item()
    err64 = (got.double() - token_unit_ref(x, dtype=torch.float64)).abs().max().item()
    print(f"{dtype} M={M} P={P}: max |gpu - twin| {err:.3e}, |gpu - fp64| {err64:.3e}, bound {bound:.3e}")
    assert err <= bound and err64 <= bound
    if M > 1:
        assert got[5].eq(0).all()
    buf = torch.full((M, P), -7.0, device=gpu)
    assert ops.token_unit(x.to(gpu), out=buf) is buf and torch.equal(buf.cpu(), got)


# ------------------------------------------------------------------ end to end
MODEL = "bert-tiny?late=64&batch=8&seq=32"
QUERIES = ["how do gpus multiply matrices", "Weather tomorrow?", "kalo mira ten"]
POOL = ["matrix cores multiply tiles", "", "gpus have many compute units", "rain, then sun", "kalo " * 40,
        "it's (not) here", "x"] + [f"passage number {i} about topic {i % 5}" for i in range(13)]  # 20 passages


@pytest.fixture(scope="module")
def handle(gpu):
    from ops._gpu_runtime import get_gpu_handle

    return get_gpu_handle(MODEL, gpu)


def _token_rows(eng, texts):
    """``(ids, lens)`` on the device of ``texts``, by the engine's own tokenizer."""
    from agent_tpu_amd.tokenizer import pack_rows

    text, offs = pack_rows(eng._encode_rows(texts))
    return eng._tokenize(torch.from_numpy(text).to(eng.device), torch.from_numpy(offs).to(eng.device))


def test_engine_token_vectors_against_the_cpu_oracle(gpu, handle):
    """The tolerance of test_embed_gpu.py for embedding vectors against the fp32 CPU oracle is relative: the
    error of the path under test is at most 1.5x that of the plain path on the same rows. Here the plain
    path is the GPU encoder's rows (``encode``) finished on the host by the twins. The bound that
    test_bert_gpu.py and test_rerank_gpu.py apply against the oracle, 0.05 * max|ref|, is checked too."""
    from agent_tpu_amd.models.bert import BertClassifier, init_random

    eng = handle.engine
    P = eng.late_dim
    assert P == 64 and handle.cfg.late_dim == 64
    texts = QUERIES + POOL[:5]
    ids, lens = _token_rows(eng, texts)
    tv = eng.model.token_vectors(ids, lens)
    h = eng.model.encode(ids, lens, cls_only_last=False)
    torch.cuda.synchronize()
    assert tv.shape == (8 * 32, P) and tv.dtype == torch.float32
    pack = init_random(handle.cfg, seed=handle.spec.seed)  # the same bits on every device
    assert torch.equal(pack["late_w"], eng.pack["late_w"].cpu())
    ref = BertClassifier(handle.cfg, pack, fp32=True).token_vectors(ids.cpu(), lens.cpu())
    plain = token_unit_ref(h.cpu().float() @ pack["late_w"].float().T)
    live = (torch.arange(32).view(1, 32) < lens.cpu().view(-1, 1)).reshape(-1)
    err = (tv.cpu() - ref)[live].abs().max().item()
    err_plain = (plain - ref)[live].abs().max().item()
    print(f"token vectors vs fp32 oracle: engine {err:.3e}, plain path {err_plain:.3e}, ratio {err / err_plain:.3f}")
    assert err <= 1.5 * err_plain
    assert err < 0.05 * ref[live].abs().max().item()
    torch.testing.assert_close(tv.cpu()[live].norm(dim=1), torch.ones(int(live.sum())), atol=1e-5, rtol=0)


def test_engine_scores_are_maxsim_of_its_own_token_vectors(gpu, handle):
    eng = handle.engine
    groups = [POOL[:3], [], POOL[3:8]]
    flat = [p for g in groups for p in g]
    goff = [0, 3, 3, 8]
    scores = eng.maxsim_scores(QUERIES, flat, goff).cpu()
    lens_q = eng.maxsim_lens_q.cpu()
    ids_q, lq = _token_rows(eng, QUERIES)
    ids_d, ld = _token_rows(eng, flat)
    qv = eng.model.token_vectors(ids_q, lq).view(-1, 32, 64).cpu()
    dv = eng.model.token_vectors(ids_d, ld).view(-1, 32, 64).cpu()
    assert torch.equal(lens_q, lq.cpu())
    qidx = torch.tensor([0, 0, 0, 2, 2, 2, 2, 2], dtype=torch.int32)
    ref = maxsim_ref(qv, lq.cpu(), dv, ld.cpu(), qidx, torch.arange(8, dtype=torch.int32))
    err = (scores.double() - ref.double()).abs()
    bound = _bound(lq.cpu(), qidx, 64, S=32)
    print(f"engine scores vs the twin on its own vectors: max err {err.max().item():.3e}, min bound {bound.min().item():.3e}")
    assert (err <= bound).all()  # real token vectors are not dyadic: the derived bound
    res = eng.maxsim_rank(QUERIES, flat, goff, top_k=4)
    want_i, want_v = ops.group_topk_ref(scores, torch.tensor(goff, dtype=torch.int32), 4)
    assert torch.equal(res.scores, scores) and torch.equal(res.idx, want_i) and torch.equal(res.score, want_v)


def test_pair_form_shared_form_and_chunks_agree_bit_for_bit(gpu, handle):
    eng = handle.engine
    assert eng.B == 8 and len(POOL) == 20  # 20 passages: chunks of 8, 8 and 4
    shared = eng.maxsim_scores(QUERIES, POOL).cpu()
    assert shared.shape == (3, 20) and torch.isfinite(shared).all()
    pairs = eng.maxsim_scores(QUERIES, POOL * 3, [0, 20, 40, 60]).cpu()  # 60 pairs: eight chunks
    assert torch.equal(_bits(pairs.view(3, 20)), _bits(shared))
    for q in range(3):  # one query alone, a single chunk of its first five passages
        alone = eng.maxsim_scores([QUERIES[q]], POOL[:5], [0, 5]).cpu()
        assert torch.equal(_bits(alone), _bits(shared[q, :5])), q
    again = eng.maxsim_scores(QUERIES, POOL).cpu()  # the second call replays the captured graphs
    assert torch.equal(_bits(again), _bits(shared))
    assert eng.maxsim_scores(QUERIES, []).shape == (3, 0) and eng.maxsim_scores([], [], [0]).shape == (0,)
