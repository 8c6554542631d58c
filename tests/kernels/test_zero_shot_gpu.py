"""Zero-shot classification on the GPU: ``premise_assemble`` bit-equal to its twin on edge rows, ``nli_rank``
bit-equal in order to its reference and within the ``__expf`` tolerance in score (exact where the
arithmetic is), and ``ClassifyEngine.zero_shot`` against ``BertClassifier.nli_logits`` on the twin's rows,
the fp32 CPU oracle, its own eager form, and itself across chunkings and batch compositions."""
import numpy as np
import pytest
import torch

from agent_tpu_amd import ops
from agent_tpu_amd import tokenizer as T
from agent_tpu_amd.models.bert import BertClassifier, config_for, init_random
from agent_tpu_amd.runtime.classify import ClassifyEngine
from agent_tpu_amd.utils.synthetic import make_text_rows, make_wordpiece_vocab

pytestmark = pytest.mark.gpu


# --------------------------------------------------------- premise_assemble
def _rows(S, toks, base=1000):
    """Single-segment rows as a tokenizer emits them, token values base + 100 * row + position."""
    ids = np.zeros((len(toks), S), dtype=np.int32)
    lens = np.zeros(len(toks), dtype=np.int32)
    for r, n in enumerate(toks):
        ids[r, 0] = 101
        ids[r, 1:1 + n] = base + 100 * r + np.arange(n)
        ids[r, 1 + n] = 102
        lens[r] = n + 2
    return ids, lens


def _assemble(gpu, ids_t, lens_t, ids_h, lens_h, tidx, hidx, mh, rows=None, extra=3):
    """The kernel on ``rows`` (default: all) of the pairs into sentinel-filled outputs ``extra`` rows longer,
    against the twin; returns the kernel's rows."""
    P = len(tidx) if rows is None else rows
    S = ids_t.shape[1]
    want = T.premise_rows(ids_t, lens_t, ids_h, lens_h, tidx[:P], hidx[:P], mh, 7, 8, 3)
    dev = [torch.from_numpy(np.ascontiguousarray(a)).to(gpu) for a in (ids_t, lens_t, ids_h, lens_h, tidx, hidx)]
    out = [torch.full((P + extra, S), -7, dtype=torch.int32, device=gpu),
           torch.full((P + extra, S), -7, dtype=torch.int32, device=gpu),
           torch.full((P + extra,), -7, dtype=torch.int32, device=gpu)]
    ops.premise_assemble(*dev, mh, 7, 8, 3, ids=out[0], type_ids=out[1], lens=out[2], rows=P)
    for got, ref in zip(out, want):
        got = got.cpu().numpy()
        assert np.array_equal(got[:P], ref), (S, P, mh)
        assert (got[P:] == -7).all(), (S, P, mh)  # rows past `rows` are not touched
    return [o[:P].cpu().numpy() for o in out]


def test_premise_assemble_edge_rows(gpu):
    """The S = 8 rows of tests/contract/test_zero_shot_cpu.py, whose expected ids are written out there."""
    S = 8
    ids_t, lens_t = _rows(S, [3, 0, 6])
    ids_h, lens_h = _rows(S, [2, 0, 6, 1], 2000)
    i32 = lambda *v: np.asarray(v, np.int32)  # noqa: E731
    ids, types, lens = _assemble(gpu, ids_t, lens_t, ids_h, lens_h, i32(2, 1, 0, 0), i32(0, 0, 1, 2), 2)
    assert ids[0].tolist() == [7, 1200, 1201, 1202, 8, 2000, 2001, 8] and lens.tolist() == [8, 5, 6, 8]  # text cut
    assert ids[1].tolist() == [7, 8, 2000, 2001, 8, 3, 3, 3] and types[1].tolist() == [0, 0, 1, 1, 1, 0, 0, 0]  # no text
    assert ids[2].tolist() == [7, 1000, 1001, 1002, 8, 8, 3, 3]                                 # no hypothesis
    assert ids[3].tolist() == [7, 1000, 1001, 1002, 8, 2200, 2201, 8]                           # hypothesis past mh
    ids, types, lens = _assemble(gpu, ids_t, lens_t, ids_h, lens_h, i32(0, 2), i32(0, 2), 0)          # mh = 0
    assert ids[1].tolist() == [7, 1200, 1201, 1202, 1203, 1204, 8, 8] and types[1].tolist() == [0] * 7 + [1]
    ids, types, lens = _assemble(gpu, ids_t, lens_t, ids_h, lens_h, i32(0, 1), i32(2, 3), S + 5)      # mh >= S
    assert ids[0].tolist() == [7, 8, 2200, 2201, 2202, 2203, 2204, 8] and types[0].tolist() == [0, 0, 1, 1, 1, 1, 1, 1]
    # out-of-range tidx, hidx and lens: clamped
    _, _, lens = _assemble(gpu, ids_t, i32(-4, 1, 99), ids_h, i32(99, -1, 0, 3), i32(-1, 7, 0, 2), i32(9, -2, 3, 1), 3)
    assert lens.tolist() == [4, 8, 4, 8]


@pytest.mark.parametrize("S", [8, 128, 512])  # 128 and 512: positions past lane 63
def test_premise_assemble_kernel_equals_twin(gpu, S):
    rng = np.random.default_rng(S)
    for P in (1, 4, 5, 9):  # four rows per workgroup, with a ragged tail
        for Tn, Hn in ((1, 1), (3, 5)):
            ids_t = rng.integers(1000, 4096, (Tn, S), dtype=np.int32)
            ids_h = rng.integers(1000, 4096, (Hn, S), dtype=np.int32)
            lens_t = rng.integers(2, S + 1, Tn, dtype=np.int32)
            lens_h = rng.integers(2, min(S, 12) + 1, Hn, dtype=np.int32)
            lens_t[0] = S                       # a full-length text, shared by many rows
            lens_h[0] = 2                       # an empty hypothesis
            if Tn > 1:
                lens_t[1], lens_t[2] = 2, S + 9  # an empty text, and one out of range
                lens_h[1], lens_h[2] = S, -3     # a full-length hypothesis, and one out of range
            tidx = rng.integers(0, Tn, P + 3, dtype=np.int32)
            hidx = rng.integers(0, Hn, P + 3, dtype=np.int32)
            tidx[: (P + 1) // 2] = 0            # one text shared by many rows
            hidx[0], tidx[P - 1] = -1, Tn
            for mh in (0, 4, S):
                _assemble(gpu, ids_t, lens_t, ids_h, lens_h, tidx, hidx, mh, rows=P)
    dev = [torch.from_numpy(a).to(gpu) for a in (ids_t, lens_t, ids_h, lens_h, tidx[:P], hidx[:P])]
    got = ops.premise_assemble(*dev, 4)  # the allocating form, default special ids
    want = T.premise_rows(ids_t, lens_t, ids_h, lens_h, tidx[:P], hidx[:P], 4)
    assert all(np.array_equal(a.cpu().numpy(), b) for a, b in zip(got, want))


# ----------------------------------------------------------------- nli_rank
LENS = [0, 1, 2, 63, 64, 65, 256, 1000, 0, 7]
ATOL, RTOL = 2e-4, 1e-3  # the project's tolerance for __expf probabilities (classify_head_topk, test_tag_gpu.py)


def _goff(lens):
    return torch.tensor(np.concatenate([[0], np.cumsum(lens)]), dtype=torch.int32)


@pytest.fixture(scope="module")
def logits():
    """The two sets of pair logits every nli_rank test reads: heavy ties with signed zeros, and randn."""
    g = torch.Generator().manual_seed(17)
    P = sum(LENS)
    values = torch.tensor([-1.0, -0.0, 0.0, 2.5])
    return values[torch.randint(0, 4, (P, 2), generator=g)], torch.randn(P, 2, generator=g) * 2


@pytest.mark.parametrize("multi", [False, True])
def test_nli_rank_kernel_equals_ref(gpu, logits, multi):
    goff = _goff(LENS)
    for pair in logits:
        want_o, want_s = ops.nli_rank_ref(pair, goff, multi)
        order, score = ops.nli_rank(pair.to(gpu), goff.to(gpu), multi)
        assert order.dtype == torch.int32 and score.dtype == torch.float32
        order, score = order.cpu(), score.cpu()
        assert torch.equal(order, want_o)  # every label of every group, in the total order
        err = (score - want_s).abs()
        print(f"nli_rank multi={multi}: max |score - fp64| = {err.max().item():.3e}")
        torch.testing.assert_close(score, want_s, atol=ATOL, rtol=RTOL)
    # offsets out of [0, P] are clamped, a decreasing pair is an empty group; NaN and inf logits
    nan, inf = float("nan"), float("inf")
    pair = torch.tensor([[1.0, 0.0], [nan, 0.0], [2.0, nan], [-inf, 0.0], [inf, 0.0], [inf, inf], [0.0, inf]])
    bad = torch.tensor([-4, 3, 99, 5], dtype=torch.int32)
    want_o, want_s = ops.nli_rank_ref(pair, bad, multi)
    order, score = ops.nli_rank(pair.to(gpu), bad.to(gpu), multi)
    order, score = order.cpu(), score.cpu()
    assert torch.equal(order, want_o)
    torch.testing.assert_close(score, want_s, atol=ATOL, rtol=RTOL)
    exact = (want_s == 0) | (want_s == 0.5) | (want_s == 1)  # all but sigmoid(1)
    assert torch.equal(score[exact], want_s[exact]) and int(exact.sum()) >= 6
    assert want_o.tolist() == ([0, 1, 2, 1, 2, 3, 0] if not multi else [0, 1, 2, 1, 0, 2, 3])
    assert want_s.tolist() == ([1.0, 0.0, 0.0, 0.5, 0.5, 0.0, 0.0] if not multi else
                               [want_s[0].item(), 0.0, 0.0, 1.0, 0.0, 0.0, 0.0])
    # a group whose best key is -inf scores 0 throughout; positions outside every group hold (-1, 0)
    pair = torch.tensor([[nan, 0.0], [-inf, 1.0], [3.0, nan], [1.0, 1.0]])
    order, score = ops.nli_rank(pair.to(gpu), torch.tensor([0, 3], dtype=torch.int32, device=gpu), multi)
    assert order.tolist() == [0, 1, 2, -1] and score.eq(0).all()
    order, score = ops.nli_rank(torch.empty((0, 2), device=gpu), torch.zeros(3, dtype=torch.int32, device=gpu), multi)
    assert order.shape == score.shape == (0,)


def test_nli_rank_exact_scores(gpu):
    bits = lambda t: t.cpu().view(torch.int32)  # noqa: E731
    # mode 0, 2^n equal logits: exp(0) = 1 each, the sum 2^n, the score exactly 2^-n
    lens = [2 ** n for n in range(1, 11)]
    pair = torch.cat([torch.tensor([[1.7 * (-1) ** n, float(n)]]).expand(m, 2) for n, m in enumerate(lens)]).contiguous()
    order, score = ops.nli_rank(pair.to(gpu), _goff(lens).to(gpu), False)
    want = torch.cat([torch.full((m,), 1.0 / m) for m in lens])
    assert torch.equal(bits(score), bits(want))
    assert torch.equal(order.cpu(), torch.cat([torch.arange(m, dtype=torch.int32) for m in lens]))  # ties: by index
    # mode 1, e == c: exactly 0.5, also in a group of one of mode 0; signed zeros and infinities aside
    pair = torch.tensor([[3.3, 3.3], [-0.0, 0.0], [-7.5, -7.5], [1e30, 1e30], [0.25, 0.25]])
    _, score = ops.nli_rank(pair.to(gpu), torch.tensor([0, 4, 5], dtype=torch.int32, device=gpu), True)
    assert torch.equal(bits(score), bits(torch.full((5,), 0.5)))
    _, one = ops.nli_rank(pair[4:].to(gpu), torch.tensor([0, 1], dtype=torch.int32, device=gpu), False)
    assert torch.equal(bits(one), bits(torch.tensor([0.5])))
    # a -inf key: exactly 0, in both modes
    ninf, nan = float("-inf"), float("nan")
    pair = torch.tensor([[0.5, 0.1], [ninf, 0.0], [nan, 0.0], [0.0, float("inf")], [1.5, nan], [0.25, 0.0]])
    for multi in (False, True):
        order, score = ops.nli_rank(pair.to(gpu), torch.tensor([0, 6], dtype=torch.int32, device=gpu), multi)
        by_label = torch.zeros(6)
        by_label[order.cpu().long()] = score.cpu()
        zero = [1, 2, 4] + ([3] if multi else [])
        assert torch.equal(bits(by_label[zero]), torch.zeros(len(zero), dtype=torch.int32)), multi
        assert (by_label[[0, 5]] > 0).all()


@pytest.mark.parametrize("multi", [False, True])
def test_nli_rank_is_invariant_to_what_shares_the_launch(gpu, logits, multi):
    """A group's (order, score) has the same bits alone, among other groups, and at another offset."""
    goff = _goff(LENS)
    for pair in logits:
        order, score = (t.cpu() for t in ops.nli_rank(pair.to(gpu), goff.to(gpu), multi))
        for t in (2, 3, 5, 7, 9):  # 2, 63, 65, 1000 and 7 labels
            a, b = int(goff[t]), int(goff[t + 1])
            alone = ops.nli_rank(pair[a:b].contiguous().to(gpu), torch.tensor([0, b - a], dtype=torch.int32, device=gpu), multi)
            assert torch.equal(alone[0].cpu(), order[a:b]), t
            assert torch.equal(alone[1].cpu().view(torch.int32), score[a:b].view(torch.int32)), t
            moved = torch.cat([pair[:3], pair[a:b], pair[:5]]).contiguous()  # the same group at offset 3
            off = torch.tensor([0, 3, 3 + b - a, 8 + b - a], dtype=torch.int32, device=gpu)
            got = ops.nli_rank(moved.to(gpu), off, multi)
            assert torch.equal(got[0].cpu()[3:3 + b - a], order[a:b]), t
            assert torch.equal(got[1].cpu()[3:3 + b - a].view(torch.int32), score[a:b].view(torch.int32)), t


# ------------------------------------------------------------------ engine
TEXTS = ["how do gpus multiply matrices", "Weather tomorrow?", "", "kalo mira ten " * 30, "it's (not) here"]
LABELS = ["kalo", "mira ten", "weather", "x", "simal lora vo"]
HYPS = ["This example is %s." % name for name in LABELS]
RANGES = [(0, 5), (1, 4), (0, 5), (2, 2), (0, 3)]  # 16 pairs; text 3 has no labels


def _twin_logits(model, eng, texts, hyps, ranges, dev):
    """``nli_logits`` of ``model`` on the premise rows of the Python twins, (ent, con) = (2, 0), in chunks of
    the engine's ``batch_rows`` as the engine runs them (a chunk's size selects the GEMM kernels)."""
    enc = lambda rows: [r.encode() for r in rows]  # noqa: E731
    ids_t, lens_t = eng.vocab.tokenize_rows(enc(texts), eng.S)
    ids_h, lens_h = eng.vocab.tokenize_rows(enc(hyps), eng.S)
    tidx = np.concatenate([np.full(b - a, t, np.int32) for t, (a, b) in enumerate(ranges)])
    hidx = np.concatenate([np.arange(a, b, dtype=np.int32) for a, b in ranges])
    ids, types, lens = T.premise_rows(ids_t, lens_t, ids_h, lens_h, tidx, hidx, T.default_max_query_tokens(eng.S),
                                      *eng._special_ids())
    assert types.any() and (lens == eng.S).any() and (lens < eng.S).any()
    assert len(tidx) % eng.B == 0  # whole chunks: no padding rows to reproduce
    rows = [torch.from_numpy(a).to(dev) for a in (ids, lens, types)]
    return torch.cat([model.nli_logits(*(r[c:c + eng.B] for r in rows), 2, 0).cpu() for c in range(0, len(tidx), eng.B)])


def _oracle_checks(res, ref, multi):
    """Logits within the bound of test_bert_gpu.py (the idiom of test_rerank_gpu.py); the ranking equals the
    oracle's wherever the oracle's key gap to both neighbours exceeds twice that bound."""
    bound = 0.05 * ref.abs().max().item()
    err = (res.logits - ref).abs().max().item()
    print(f"zero_shot multi={multi}: max |logit - oracle| = {err:.3e}, bound {bound:.3e}")
    assert err < bound
    goff = torch.tensor(res.goff, dtype=torch.int32)
    want_o, _ = ops.nli_rank_ref(ref, goff, multi)
    for t in range(res.texts):
        a, b = res.goff[t], res.goff[t + 1]
        if b == a:
            continue
        key = ops.zeroshot.nli_keys(ref[a:b], multi or b - a == 1)[want_o[a:b].long()]
        gap = (key[:-1] - key[1:]) > 2 * bound * (2 if multi else 1)  # e - c carries both logits' errors
        clear = torch.cat([torch.tensor([True]), gap]) & torch.cat([gap, torch.tensor([True])])
        assert torch.equal(res.order[a:b][clear], want_o[a:b][clear]), t


@pytest.fixture(scope="module")
def tiny(tmp_path_factory):
    path = tmp_path_factory.mktemp("wp") / "vocab.txt"
    with open(path, "wb") as f:
        f.write("\n".join(make_wordpiece_vocab(300, seed=1)).encode("utf-8") + b"\n")
    cfg = config_for("bert-tiny", num_labels=3)
    return cfg, init_random(cfg, seed=2, bias_std=0.02), T.WordPieceVocab.load(str(path))


@pytest.mark.parametrize("multi", [False, True])
def test_zero_shot_tiny(gpu, tiny, multi):
    cfg, pack, vocab = tiny
    kw = dict(batch_rows=4, seq_len=32, topk=1, vocab=vocab)
    eng_g = ClassifyEngine(cfg, pack, gpu, use_graph=True, **kw)
    eng_e = ClassifyEngine(cfg, pack, gpu, use_graph=False, **kw)
    res = eng_g.zero_shot(TEXTS, HYPS, RANGES, multi, ent=2, con=0)  # 16 pairs: four chunks of four
    again = eng_g.zero_shot(TEXTS, HYPS, RANGES, multi, ent=2, con=0)  # the second call replays the captured graphs
    eager = eng_e.zero_shot(TEXTS, HYPS, RANGES, multi, ent=2, con=0)
    assert res.logits.shape == (16, 2) and res.goff == [0, 5, 8, 13, 13, 16] and torch.isfinite(res.logits).all()
    assert len([k for k in eng_g._bgraphs if k[0] == "zeroshot"]) == 1
    for other in (again, eager):  # graph replay == eager, bit for bit
        assert torch.equal(res.logits, other.logits) and torch.equal(res.order, other.order)
        assert torch.equal(res.score, other.score)
    # the engine's logits are BertClassifier.nli_logits on the twin's rows; its ranking is nli_rank's
    direct = _twin_logits(eng_g.model, eng_g, TEXTS, HYPS, RANGES, gpu)
    torch.testing.assert_close(res.logits, direct, atol=0, rtol=0)
    want_o, want_s = ops.nli_rank_ref(res.logits, torch.tensor(res.goff, dtype=torch.int32), multi)
    assert torch.equal(res.order, want_o)
    torch.testing.assert_close(res.score, want_s, atol=ATOL, rtol=RTOL)
    assert res.ranked(3) == ([], []) and sorted(res.ranked(1)[0]) == [0, 1, 2]
    # the fp32 CPU oracle
    ref = _twin_logits(BertClassifier(cfg, pack, fp32=True), eng_g, TEXTS, HYPS, RANGES, "cpu")
    _oracle_checks(res, ref, multi)
    # a job spanning several chunks against every text on its own (texts 1 and 4: one chunk each)
    for t, (a, b) in enumerate(RANGES):
        one = eng_g.zero_shot([TEXTS[t]], HYPS, [(a, b)], multi, ent=2, con=0)
        assert torch.equal(one.logits, res.logits[res.goff[t]:res.goff[t + 1]]), t
        assert one.ranked(0) == res.ranked(t), t


@pytest.fixture
def invariant():
    prev = ops.set_batch_invariant(True)
    yield
    ops.set_batch_invariant(prev)


def test_zero_shot_is_batch_invariant(gpu, invariant):
    """A text's logits, order and scores have the same bits alone, among 40 pairs, and across a chunk
    boundary (``batch_rows`` 32: 40 pairs are a chunk of 32 and one of 8, padded to the 16-row bucket)."""
    cfg = config_for("bert-base", num_labels=3)  # an engine of its own: its graphs are captured in this mode
    eng = ClassifyEngine(cfg, init_random(cfg, seed=0, device=gpu), gpu, batch_rows=32, seq_len=128, topk=1)
    texts = make_text_rows(4, words_per_row=40, seed=12) + make_text_rows(1, words_per_row=150, seed=13)
    hyps = ["This example is %s." % w for w in make_text_rows(1, words_per_row=10, seed=14)[0].split()]
    ranges = [(0, 10), (0, 10), (0, 10), (2, 8), (6, 10)]  # text 3 owns pairs 30..35: both chunks
    many = eng.zero_shot(texts, hyps, ranges, False)
    assert many.logits.shape == (40, 2) and many.goff == [0, 10, 20, 30, 36, 40]
    for t in (0, 3, 4):
        one = eng.zero_shot([texts[t]], hyps, [ranges[t]], False)
        a, b = many.goff[t], many.goff[t + 1]
        assert torch.equal(one.logits, many.logits[a:b]), t
        assert torch.equal(one.order, many.order[a:b]) and torch.equal(one.score, many.score[a:b]), t
    half = eng.zero_shot(texts[3:], hyps, ranges[3:], False)
    assert torch.equal(half.logits, many.logits[30:]) and torch.equal(half.score, many.score[30:])
