"""``maxsim_index`` (csrc/kernels/maxsim_index.hip) on the GPU: bit-equal to the twin on exactly representable
inputs in both storage dtypes and both forms, an fp32 index bit-equal to ``ops.maxsim`` on the padded tensors,
an fp16 index within the derived bound, blind to what the neighbouring passages' rows and the query's padding
rows hold, the same bits wherever a pair sits in a launch, clamped device data, and the engine's index path
end to end on ``bert-tiny?late=64``.

Shapes: N = 7 packed passages of 17, 1, 33, 16, 70, 2 and 31 tokens (tails in the 16-row tile, one to five row
tiles per passage), two more of 15 and 32 where N is enlarged; queries S = 20 with ``lens_q`` = (16, 20, 1).
P = 64 and 192 keep every passage in one on-chip tile. P = 1024 is the case of a passage longer than the
on-chip tile at the kernel's own capacity: the fp32 tile holds 16 rows (66 KB), so the 70-token passage is walked
in five tiles and every passage above 16 tokens in more than one; the fp16 tile holds 32 rows, three tiles.

Bounds. Against the fp32 twin on the same stored values or an fp64 loop, on unit vectors:
``|err| <= len_q * (P + len_q) * 2^-23`` (test_maxsim_gpu.py's derivation)."""
import functools

import numpy as np
import pytest
import torch

from agent_tpu_amd import ops
from agent_tpu_amd.ops.maxsim import maxsim_index_ref

pytestmark = pytest.mark.gpu

S, QN = 20, 3
LENS = (17, 1, 33, 16, 70, 2, 31)
MORE = (15, 32)
LENS_Q = (16, 20, 1)
PIDX = [4, 0, 6, 0, 2, 5]  # not monotone, with a repeat
QOFF = [0, 2, 2, 3, 6, 7, 9]  # item 1 is empty
QSEL = [2, 0, 1, 1, 2, 0, 1, 0, 2]  # not monotone
DTYPES = [torch.float16, torch.float32]


def _i32(v):
    return torch.tensor(v, dtype=torch.int32)


@functools.lru_cache(maxsize=None)
def _case(P, kind, lens=LENS):
    """``(qv, lens_q, tok fp32, off)`` on the host, built once and never changed: "dyadic" (the grid {-2..2}/4,
    exact in fp16 and in any summation order) or "unit" (random unit rows)."""
    g = torch.Generator().manual_seed(P + (0 if kind == "dyadic" else 1))
    T = sum(lens)
    if kind == "dyadic":
        qv = torch.randint(-2, 3, (QN, S, P), generator=g).float() / 4
        tok = torch.randint(-2, 3, (T, P), generator=g).float() / 4
    else:
        qv = torch.nn.functional.normalize(torch.randn(QN, S, P, generator=g), dim=-1)
        tok = torch.nn.functional.normalize(torch.randn(T, P, generator=g), dim=-1)
    off = torch.tensor([0] + np.cumsum(lens).tolist(), dtype=torch.int64)
    return qv, _i32(list(LENS_Q)), tok, off


@functools.lru_cache(maxsize=None)
def _twin(P, kind, dtype):
    """The twin's all-form scores ``[QN, N]`` of the case with ``tok`` stored as ``dtype``."""
    qv, lens_q, tok, off = _case(P, kind)
    return maxsim_index_ref(qv, lens_q, tok.to(dtype), off)


@functools.lru_cache(maxsize=None)
def _loop64(P, kind, dtype):
    qv, lens_q, tok, off = _case(P, kind)
    q64, t64 = qv.double().numpy(), tok.to(dtype).double().numpy()
    out = np.zeros((QN, len(LENS)))
    for a in range(QN):
        for p in range(len(LENS)):
            out[a, p] = sum(max(float(np.dot(q64[a, i], t64[j])) for j in range(int(off[p]), int(off[p + 1])))
                            for i in range(LENS_Q[a]))
    return torch.from_numpy(out)


def _run(gpu, qv, lens_q, tok, off, pidx=None, qoff=None, qsel=None, **kw):
    dev = lambda t: None if t is None else t.to(gpu)  # noqa: E731
    out = ops.maxsim_index(dev(qv), dev(lens_q), dev(tok), dev(off), dev(pidx), dev(qoff), dev(qsel), **kw)
    torch.cuda.synchronize()
    return out.cpu()


def _bits(t):
    return t.contiguous().view(torch.int32)


def _item_of_entry():
    return [m for m in range(len(PIDX)) for _ in range(QOFF[m + 1] - QOFF[m])]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("P", [64, 192, 1024])
def test_dyadic_inputs_are_bit_equal_to_the_twin(gpu, P, dtype):
    qv, lens_q, tok, off = _case(P, "dyadic")
    want = _twin(P, "dyadic", dtype)
    t = tok.to(dtype)
    assert torch.equal(_bits(_run(gpu, qv, lens_q, t, off)), _bits(want))
    sub = _run(gpu, qv, lens_q, t, off, _i32(PIDX))
    assert torch.equal(_bits(sub), _bits(want[:, PIDX]))
    lst = _run(gpu, qv, lens_q, t, off, _i32(PIDX), _i32(QOFF), _i32(QSEL))
    ref = torch.stack([want[q, PIDX[m]] for q, m in zip(QSEL, _item_of_entry())])
    assert torch.equal(_bits(lst), _bits(ref))
    assert torch.equal(_bits(lst), _bits(maxsim_index_ref(qv, lens_q, t, off, _i32(PIDX), _i32(QOFF), _i32(QSEL))))


@pytest.mark.parametrize("kind", ["dyadic", "unit"])
@pytest.mark.parametrize("P", [64, 192, 1024])
def test_fp32_index_has_the_bits_of_maxsim_on_the_padded_tensors(gpu, P, kind):
    qv, lens_q, tok, off = _case(P, kind)
    N, Sp = len(LENS), max(LENS)
    dv = torch.zeros(N, Sp, P)
    for p in range(N):
        dv[p, :LENS[p]] = tok[int(off[p]):int(off[p + 1])]
    qp = torch.zeros(QN, Sp, P)
    qp[:, :S] = qv
    qidx = torch.arange(QN, dtype=torch.int32).repeat_interleave(N)
    didx = torch.arange(N, dtype=torch.int32).repeat(QN)
    pair = ops.maxsim(qp.to(gpu), lens_q.to(gpu), dv.to(gpu), _i32(list(LENS)).to(gpu), qidx.to(gpu), didx.to(gpu))
    got = _run(gpu, qv, lens_q, tok, off)
    assert torch.equal(_bits(got.reshape(-1)), _bits(pair.cpu()))


@pytest.mark.parametrize("P", [64, 192, 1024])
def test_fp16_index_on_unit_rows(gpu, P):
    qv, lens_q, tok, off = _case(P, "unit")
    t = tok.half()
    got = _run(gpu, qv, lens_q, t, off)
    lq = lens_q.double().view(-1, 1)
    bound = lq * (P + lq) * 2.0 ** -23
    err = (got.double() - _twin(P, "unit", torch.float16).double()).abs()
    err64 = (got.double() - _loop64(P, "unit", torch.float16)).abs()
    print(f"fp16 P={P}: max |gpu - twin| {err.max():.3e}, |gpu - fp64| {err64.max():.3e}, bound {bound.min():.3e}..{bound.max():.3e}")
    assert (err <= bound).all() and (err64 <= bound).all()
    assert torch.equal(_bits(_run(gpu, qv, lens_q, t, off)), _bits(got))  # the same bits run to run
    # and the fp32 index against its own twin and the fp64 loop
    got32 = _run(gpu, qv, lens_q, tok, off)
    assert ((got32.double() - _twin(P, "unit", torch.float32).double()).abs() <= bound).all()
    assert ((got32.double() - _loop64(P, "unit", torch.float32)).abs() <= bound).all()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("P", [64, 1024])
def test_neighbours_and_query_padding_reach_no_score(gpu, P, dtype):
    qv, lens_q, tok, off = _case(P, "unit")
    t = tok.to(dtype)
    want = _run(gpu, qv, lens_q, t, off)
    for poison in (float("nan"), 1e30 if dtype == torch.float32 else 6e4):
        for p in range(len(LENS)):  # everything but passage p: a tile's clamped reads land on neighbours
            bad = torch.full_like(t, poison)
            bad[int(off[p]):int(off[p + 1])] = t[int(off[p]):int(off[p + 1])]
            got = _run(gpu, qv, lens_q, bad, off, _i32([p]))
            assert torch.equal(_bits(got[:, 0]), _bits(want[:, p])), (poison, p)
        pq = qv.clone()
        pq[torch.arange(S).view(1, S) >= lens_q.view(-1, 1)] = poison if poison != 6e4 else 1e30
        assert torch.equal(_bits(_run(gpu, pq, lens_q, t, off)), _bits(want))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("P", [192, 1024])
def test_a_pair_has_the_same_bits_wherever_it_sits(gpu, P, dtype):
    qv, lens_q, tok, off = _case(P, "unit")
    t = tok.to(dtype)
    want = _run(gpu, qv, lens_q, t, off)  # all form
    N = len(LENS)
    for q, p in ((1, 4), (0, 2), (2, 1)):
        w = _bits(want[q, p])
        alone = _run(gpu, qv[q:q + 1].contiguous(), lens_q[q:q + 1], t, off, _i32([p]))
        assert torch.equal(_bits(alone[0, 0]), w)
        first = _run(gpu, qv, lens_q, t, off, _i32([p, 0, 3, 5]))
        last = _run(gpu, qv, lens_q, t, off, _i32([0, 3, 5, 6, 1, p]))
        assert torch.equal(_bits(first[q, 0]), w) and torch.equal(_bits(last[q, 5]), w)
        # list form: alone in its item, and with other queries sharing the item
        one = _run(gpu, qv, lens_q, t, off, _i32([3, p]), _i32([0, 0, 1]), _i32([q]))
        assert torch.equal(_bits(one[0]), w)
        shared = _run(gpu, qv, lens_q, t, off, _i32([p, 3]), _i32([0, 5, 6]), _i32([0, 2, q, 1, 0, 2]))
        assert torch.equal(_bits(shared[2]), w)
    # Qn and N enlarged: 35 queries (two query chunks of the all form) and two more passages
    qv2 = torch.cat([qv] * 11 + [qv[:2]])
    lens_q2 = torch.cat([lens_q] * 11 + [lens_q[:2]])
    g = torch.Generator().manual_seed(7)
    more = torch.nn.functional.normalize(torch.randn(sum(MORE), P, generator=g), dim=-1).to(dtype)
    tok2 = torch.cat([t, more])
    off2 = torch.cat([off, off[-1] + torch.tensor(np.cumsum(MORE).tolist(), dtype=torch.int64)])
    big = _run(gpu, qv2, lens_q2, tok2, off2)
    assert big.shape == (35, N + 2)
    for rep in (0, 5, 10):
        assert torch.equal(_bits(big[3 * rep:3 * rep + 3, :N]), _bits(want))
    assert torch.equal(_bits(big[33:35, :N]), _bits(want[:2]))
    small = _run(gpu, qv, lens_q, more, off2[N:] - off2[N])  # the two new passages as an index of their own
    assert torch.equal(_bits(big[:3, N:]), _bits(small))


@pytest.mark.parametrize("dtype", DTYPES)
def test_wild_device_data_equals_its_clamped_form(gpu, dtype):
    P = 64
    qv, lens_q, tok, off = _case(P, "unit")
    t = tok.to(dtype)
    N, T = len(LENS), sum(LENS)
    wild = _run(gpu, qv, _i32([16, 99, -3]), t, off, _i32([-1, N + 5, 2 ** 31 - 1]), _i32([-4, 1, 99, 99]),
                _i32([QN + 5, -1, -(2 ** 31)]))
    want = _run(gpu, qv, _i32([16, 20, 1]), t, off, _i32([0, N - 1, N - 1]), _i32([0, 1, 3, 3]), _i32([QN - 1, 0, 0]))
    assert torch.equal(_bits(wild), _bits(want))
    full = _run(gpu, qv, lens_q, t, off)
    bad = off.clone()
    bad[2] = bad[1]  # passage 1: length 0 -> 1
    bad[-1] = T + 50  # the last passage runs past T -> T - start
    got = _run(gpu, qv, lens_q, t, bad)
    a = int(off[1])
    ref = _run(gpu, qv, lens_q, t, torch.tensor([0, a, a + 1], dtype=torch.int64))
    assert torch.equal(_bits(got[:, 1]), _bits(ref[:, 1])) and torch.equal(_bits(got[:, N - 1]), _bits(full[:, N - 1]))
    neg = off.clone()
    neg[0] = -9  # start -> 0, length 17 + 9 = 26: the first 26 rows
    got = _run(gpu, qv, lens_q, t, neg)
    ref = _run(gpu, qv, lens_q, t, torch.tensor([0, 26, T], dtype=torch.int64))
    assert torch.equal(_bits(got[:, 0]), _bits(ref[:, 0]))
    assert torch.equal(_bits(maxsim_index_ref(qv, lens_q, t, neg)[:, 0]), _bits(maxsim_index_ref(qv, lens_q, t, off.new_tensor([0, 26, T]))[:, 0]))


def test_refusals_empty_launches_and_out(gpu):
    qv, lens_q, tok, off = _case(64, "unit")
    d = lambda t: t.to(gpu)  # noqa: E731
    for bad in (lambda: ops.maxsim_index(d(qv[..., :48].contiguous()), d(lens_q), d(tok[:, :48].contiguous()), d(off)),
                lambda: ops.maxsim_index(d(qv), d(lens_q), d(tok[:, :32].contiguous()), d(off)),
                lambda: ops.maxsim_index(d(qv), d(lens_q), d(tok.bfloat16()), d(off)),
                lambda: ops.maxsim_index(d(qv), d(lens_q), d(tok.double()), d(off)),
                lambda: ops.maxsim_index(d(qv.half()), d(lens_q), d(tok), d(off)),
                lambda: ops.maxsim_index(d(qv), d(lens_q), d(tok), d(off.int())),
                lambda: ops.maxsim_index(d(qv), d(lens_q), d(tok), d(off), d(_i32(PIDX)), d(_i32(QOFF))),
                lambda: ops.maxsim_index(d(qv), d(lens_q), d(tok), off)):
        with pytest.raises(ValueError):
            bad()
    assert _run(gpu, qv, lens_q, tok, off, _i32([])).shape == (QN, 0)  # M == 0: nothing is launched
    assert _run(gpu, qv, lens_q, tok, off, _i32(PIDX), _i32([0] * 7), _i32([])).shape == (0,)
    want = _run(gpu, qv, lens_q, tok, off, _i32(PIDX))
    buf = torch.full((QN, len(PIDX)), -7.0, device=gpu)
    got = ops.maxsim_index(d(qv), d(lens_q), d(tok), d(off), d(_i32(PIDX)), out=buf)
    assert got is buf and torch.equal(_bits(buf.cpu()), _bits(want))
    lbuf = torch.full((len(QSEL),), -7.0, device=gpu)
    ops.maxsim_index(d(qv), d(lens_q), d(tok), d(off), d(_i32(PIDX)), d(_i32(QOFF)), d(_i32(QSEL)), out=lbuf)
    assert torch.equal(_bits(lbuf.cpu()), _bits(_run(gpu, qv, lens_q, tok, off, _i32(PIDX), _i32(QOFF), _i32(QSEL))))


# ------------------------------------------------------------------ end to end
MODEL = "bert-tiny?late=64&batch=8&seq=32"
QUERIES = ["how do gpus multiply matrices", "Weather tomorrow?", "kalo mira ten"]
POOL = ["matrix cores multiply tiles", "", "gpus have many compute units", "rain, then sun", "kalo " * 40,
        "it's (not) here", "x"] + [f"passage number {i} about topic {i % 5}" for i in range(13)]  # 20 passages


@pytest.fixture(scope="module")
def handle(gpu):
    from ops._gpu_runtime import get_gpu_handle

    return get_gpu_handle(MODEL, gpu)


def _resident(eng, tok, lens, dtype):
    from agent_tpu_amd.runtime.maxsim_index import TokenIndex

    off = torch.zeros(lens.numel() + 1, dtype=torch.int64, device=tok.device)
    off[1:] = torch.cumsum(lens.to(torch.int64), 0)
    return TokenIndex(tok.to(dtype).contiguous(), off, 0, int(lens.numel()), str(dtype).split(".")[1], False)


def test_engine_index_equals_the_on_the_fly_path(gpu, handle):
    eng = handle.engine
    want = eng.maxsim_scores(QUERIES, POOL).cpu()  # [3, 20]
    tok, lens = eng.maxsim_build(POOL)
    assert tok.dtype == torch.float32 and tok.shape == (int(lens.sum()), 64) and lens.numel() == 20
    index = _resident(eng, tok, lens, torch.float32)
    assert torch.equal(_bits(eng.maxsim_index_scores(QUERIES, index).cpu()), _bits(want))
    cand = [[19, 0, 4, 7], [], [4, 1, 18]]
    got = eng.maxsim_index_scores(QUERIES, index, cand).cpu()
    assert got.shape == (3, 4)
    for q, c in enumerate(cand):
        assert torch.equal(_bits(got[q, :len(c)]), _bits(want[q, c])) and got[q, len(c):].eq(float("-inf")).all()
    # a slice (a DP rank's share): candidates outside it are -inf
    from agent_tpu_amd.runtime.maxsim_index import TokenIndex

    a, b = 5, 12
    r0, r1 = int(index.offsets[a]), int(index.offsets[b])
    part = TokenIndex(tok[r0:r1].contiguous(), (index.offsets[a:b + 1] - r0).contiguous(), a, 20, "float32", False)
    assert torch.equal(_bits(eng.maxsim_index_scores(QUERIES, part).cpu()), _bits(want[:, a:b]))
    sl = eng.maxsim_index_scores(QUERIES, part, cand).cpu()
    assert torch.equal(_bits(sl[0, 3]), _bits(want[0, 7])) and sl[0, :3].eq(float("-inf")).all() and sl[2].eq(float("-inf")).all()
    # fp16: within the bound of the fp32 scores
    h = eng.maxsim_index_scores(QUERIES, _resident(eng, tok, lens, torch.float16)).cpu()
    lq = eng.maxsim_lens_q.cpu().double().view(-1, 1)
    bound = lq * (2.0 ** -11 + 64 * 2.0 ** -24) + lq * (64 + lq) * 2.0 ** -23
    print(f"fp16 index: max |fp16 - fp32| {(h.double() - want.double()).abs().max():.3e}, bound {bound.min():.3e}")
    assert ((h.double() - want.double()).abs() <= bound).all()
    # rank: group_topk of its own scores
    res = eng.maxsim_index_rank(QUERIES, index, None, top_k=5)
    wi, wv = ops.group_topk_ref(want.reshape(-1), _i32([0, 20, 40, 60]), 5)
    assert torch.equal(res.idx, wi) and torch.equal(_bits(res.score), _bits(wv)) and torch.equal(_bits(res.scores.view(3, 20)), _bits(want))
    rc = eng.maxsim_index_rank(QUERIES, index, cand, top_k=3)
    flat = torch.cat([want[q, c] for q, c in enumerate(cand)])
    wi, wv = ops.group_topk_ref(flat, _i32([0, 4, 4, 7]), 3)
    assert torch.equal(rc.idx, wi) and torch.equal(_bits(rc.score), _bits(wv))
