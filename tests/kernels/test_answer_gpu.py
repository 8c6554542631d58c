"""The reader on the GPU: ``span_topk`` logits against the fp64 evaluation of its formula within the
fp32 summation bound, its selection bit-equal to ``span_select_ref`` on the kernel's own logits on tie,
NaN and edge rows, and ``ClassifyEngine.answer_pairs`` against ``BertClassifier.spans`` on the twin's
rows, the fp32 CPU oracle, its own eager form, the unfused form, and itself across batch compositions."""
import numpy as np
import pytest
import torch

from agent_tpu_amd import ops
from agent_tpu_amd import tokenizer as T
from agent_tpu_amd.models.bert import BertClassifier, config_for, init_random
from agent_tpu_amd.runtime.classify import ClassifyEngine
from agent_tpu_amd.utils.synthetic import make_text_rows, make_wordpiece_vocab

pytestmark = pytest.mark.gpu

NINF = float("-inf")


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def _types_lens(B, S, g):
    """Pair-row shaped ``type_ids`` / ``lens``: ``q`` question tokens, mixed lengths, one full row."""
    q = (S - 4) // 3
    lens = torch.randint(q + 3, S + 1, (B,), generator=g, dtype=torch.int32)
    lens[0] = S
    types = torch.zeros((B, S), dtype=torch.int32)
    for b in range(B):
        types[b, q + 2:int(lens[b])] = 1
    return types, lens


def _select_equals_ref(out, logits, types, lens, max_len, n, tag):
    span, score, null = out
    want = ops.span_select_ref(logits.cpu(), types.cpu(), lens.cpu(), max_len, n)
    assert torch.equal(span.cpu(), want[0]), tag
    assert torch.equal(_bits(score), _bits(want[1])), tag  # the stored bits, zeros' signs too
    assert torch.equal(_bits(null), _bits(want[2])), tag


# ------------------------------------------------------------------- logits
@pytest.mark.parametrize("S", [4, 7, 128, 512])
def test_span_logits_within_fp32_summation_bound(gpu, S):
    for H in (64, 768, 1024):
        for B in (1, 5):  # 5: odd rows per launch
            for use_fin in (True, False):
                g = torch.Generator().manual_seed(S * 7 + H + B)
                x = torch.randn(B * S, H, generator=g).bfloat16()
                u = torch.randn(2, H, generator=g) * 0.05
                su = u.double().sum(1).float()
                c = torch.randn(2, generator=g)
                rstd = torch.rand(B * S, generator=g) * 1.5 + 0.5
                mu = torch.randn(B * S, generator=g) * 0.1
                fin = torch.stack([rstd, rstd * mu], 1).contiguous() if use_fin else None
                types, lens = _types_lens(B, S, g)
                live = (torch.arange(S).view(1, S) < lens.view(B, 1)).view(B * S)
                # the fp64 evaluation of the same formula on the same bf16 / fp32 inputs, and its bound
                xd, ud = x.double(), u.double()
                dot, mag = xd @ ud.t(), xd.abs() @ ud.abs().t()
                if use_fin:
                    fd = fin.double()
                    ref = fd[:, :1] * dot - fd[:, 1:] * su.double() + c.double()
                    bound = 2 * H * 2.0 ** -24 * (fd[:, :1].abs() * mag + (fd[:, 1:] * su.double()).abs() + c.double().abs())
                else:
                    ref = dot + c.double()
                    bound = 2 * H * 2.0 ** -24 * (mag + c.double().abs())
                xp, fp = x.clone(), None if fin is None else fin.clone()
                xp[~live] = float("nan")  # poisoned padding rows change nothing
                if fp is not None:
                    fp[~live] = float("nan")
                outs = []
                for xx, ff in ((x, fin), (xp, fp)):
                    logits = torch.full((B, S, 2), 7.0, device=gpu)
                    out = ops.span_topk(xx.to(gpu), lens.to(gpu), types.to(gpu), B, u.to(gpu), su.to(gpu), c.to(gpu),
                                        min(30, S), 3, fin=None if ff is None else ff.to(gpu), logits_out=logits)
                    outs.append((logits.cpu(),) + tuple(o.cpu() for o in out))
                tag = (S, H, B, use_fin)
                lg = outs[0][0].view(B * S, 2)
                err = (lg.double() - ref).abs()
                assert (err[live] <= bound[live]).all(), (tag, (err[live] / bound[live]).max().item())
                assert (lg[~live] == NINF).all(), tag  # positions >= len
                for a, b in zip(outs[0], outs[1]):
                    assert torch.equal(_bits(a), _bits(b)), tag
                _select_equals_ref(outs[0][1:], outs[0][0], types, lens, min(30, S), 3, tag)


# ---------------------------------------------------------------- selection
def _tie_rows(S, gpu, seed=0):
    """Rows whose logits the kernel computes exactly (H = 64, unit head vectors, fin = (+-1, 0), c = -0.0):
    values from {+-1, +-2.5, +-0.0} (heavy ties, signed zeros), a NaN and infinities, an empty passage,
    lens out of range, no type-1 position at all, type 1 from position 0."""
    g = torch.Generator().manual_seed(seed + S)
    B, H = 8, 64
    values = torch.tensor([-1.0, 0.0, 0.0, 2.5])
    x = torch.zeros(B, S, H)
    x[:, :, 0] = values[torch.randint(0, 4, (B, S), generator=g)]
    x[:, :, 1] = values[torch.randint(0, 4, (B, S), generator=g)]
    x[7, :, :2] = torch.randn(S, 2, generator=g)
    x[1, 2, 0], x[1, S - 2, 1] = float("nan"), float("nan")
    x[1, 1, 1] = float("inf")
    x[1, S - 3 if S > 4 else 1, 0] = float("-inf")
    u = torch.zeros(2, H)
    u[0, 0] = u[1, 1] = 1.0
    rstd = torch.where(torch.rand(B * S, generator=g) < 0.5, -1.0, 1.0)
    fin = torch.stack([rstd, torch.zeros(B * S)], 1).contiguous()
    q = (S - 4) // 3
    types = torch.zeros((B, S), dtype=torch.int32)
    types[:, q + 2:] = 1
    lens = torch.full((B,), S, dtype=torch.int32)
    lens[2] = q + 3                     # an empty passage: lo = q + 2 > hi = q + 1
    types[2, q + 3:] = 0
    lens[3], lens[4] = -5, S + 100      # out of range: clamped into [2, S]
    types[5] = 0                        # no type-1 position at all
    types[6] = 1                        # type 1 from position 0
    lens[6] = max(4, S - 1)
    lens[7] = max(4, (3 * S) // 4)
    types[7, int(lens[7]):] = 0
    dev = [t.to(gpu) for t in (x.view(B * S, H).bfloat16(), lens, types, u, torch.zeros(2), torch.tensor([-0.0, -0.0]),
                               fin)]
    return B, dev


@pytest.mark.parametrize("S", [4, 7, 128, 512])
def test_span_selection_equals_ref_on_own_logits(gpu, S):
    B, (x, lens, types, u, su, c, fin) = _tie_rows(S, gpu)
    saw_negzero = False
    for n in (1, 3, 32):
        for max_len in sorted({1, min(30, S), S}):
            logits = torch.zeros((B, S, 2), device=gpu)
            out = ops.span_topk(x, lens, types, B, u, su, c, max_len, n, fin=fin, logits_out=logits)
            _select_equals_ref(out, logits, types, lens, max_len, n, (S, n, max_len))
            span, score, _ = (o.cpu() for o in out)
            assert span[2].eq(-1).all() and (score[2] == NINF).all()  # the empty passage
            assert span[3].eq(-1).all() and span[5].eq(-1).all()      # len clamped to 2; no passage segment
            lg = logits.cpu()
            saw_negzero |= bool(((lg == 0) & (_bits(lg) != 0)).any())
            if S >= 7:
                assert torch.isnan(lg[1]).any() and (score[1] == score[1]).all()  # a NaN ranks as -inf
    assert saw_negzero  # signed zeros do reach the selection


def test_span_rows_alone_and_in_a_batch_and_bounds(gpu):
    S, H, B = 128, 768, 5
    g = torch.Generator().manual_seed(5)
    x = torch.randn(B * S, H, generator=g).bfloat16().to(gpu)
    u = (torch.randn(2, H, generator=g) * 0.05).to(gpu)
    su, c = u.double().sum(1).float(), torch.randn(2, generator=g).to(gpu)
    fin = torch.stack([torch.rand(B * S, generator=g) + 0.5, torch.randn(B * S, generator=g) * 0.1], 1).to(gpu)
    types, lens = (t.to(gpu) for t in _types_lens(B, S, g))
    span = torch.full((B + 2, 4, 2), -7, dtype=torch.int32, device=gpu)
    score = torch.full((B + 2, 4), -7.0, device=gpu)
    null = torch.full((B + 2,), -7.0, device=gpu)
    logits = torch.full((B + 2, S, 2), -7.0, device=gpu)
    ops.span_topk(x, lens, types, B, u, su, c, 30, 4, fin=fin, span=span, score=score, null=null, logits_out=logits)
    for t in (span, score, null, logits):  # buffers past B are untouched
        assert t[B:].eq(-7).all() and not t[:B].eq(-7).all()
    for b in range(B):  # a row's outputs have the same bits alone and inside the batch
        lg1 = torch.zeros((1, S, 2), device=gpu)
        one = ops.span_topk(x[b * S:(b + 1) * S], lens[b:b + 1], types[b:b + 1], 1, u, su, c, 30, 4,
                            fin=fin[b * S:(b + 1) * S], logits_out=lg1)
        for a, w in zip(one + (lg1,), (span[b:b + 1], score[b:b + 1], null[b:b + 1], logits[b:b + 1])):
            assert torch.equal(_bits(a), _bits(w)), b
    empty = ops.span_topk(x[:0], lens, types, 0, u, su, c, 30, 4)  # B == 0: no launch
    assert empty[0].shape == (0, 4, 2)
    for kw in (dict(n=0), dict(n=33), dict(max_len=0), dict(max_len=S + 1)):  # unsupported shapes raise
        args = dict(max_len=30, n=4)
        args.update(kw)
        with pytest.raises(ValueError):
            ops.span_topk(x, lens, types, B, u, su, c, args["max_len"], args["n"], fin=fin)
    with pytest.raises(ValueError):  # H = 96 is not a multiple of 64
        ops.span_topk(x[:, :96].contiguous(), lens, types, B, u[:, :96].contiguous(), su, c, 30, 4)
    with pytest.raises(ValueError):  # S = 640 > 512
        ops.span_topk(x, lens[:1], torch.zeros((1, 640), dtype=torch.int32, device=gpu), 1, u, su, c, 30, 4)
    with pytest.raises(ValueError):  # fp32 rows on the device
        ops.span_topk(x.float(), lens, types, B, u, su, c, 30, 4)


# ------------------------------------------------------------------ engine
QUESTIONS = ["how do gpus multiply matrices", "Weather tomorrow?", "kalo mira ten"]
GROUPS = [[], ["a recipe for bread"],
          ["matrix cores multiply tiles", "", "gpus have many compute units", "rain, then sun",
           "kalo " * 90, "it's (not) here", "x"]]


def _flat(groups):
    goff = [0]
    for g in groups:
        goff.append(goff[-1] + len(g))
    return [p for g in groups for p in g], goff


def _twin_rows(eng, questions, flat, goff, bucket):
    """The pair rows of an engine call by the Python twins, padded to ``bucket`` rows as the engine pads
    them (an empty passage of question 0)."""
    enc = lambda rows: [r.encode() for r in rows]  # noqa: E731
    if eng.vocab is not None:
        tok = lambda rows: eng.vocab.tokenize_rows(enc(rows), eng.S)  # noqa: E731
    else:
        tok = lambda rows: T.tokenize_rows(enc(rows), eng.S, eng.cfg.vocab_size)  # noqa: E731
    used = [q for q in range(len(questions)) if goff[q + 1] > goff[q]]
    qidx = np.repeat(np.arange(len(used)), [goff[q + 1] - goff[q] for q in used]).astype(np.int32)
    pad = bucket - len(flat)
    ids_q, lens_q = tok([questions[q] for q in used])
    ids_p, lens_p = tok(list(flat) + [""] * pad)
    return T.pair_rows(ids_q, lens_q, ids_p, lens_p, np.concatenate([qidx, np.zeros(pad, np.int32)]),
                       T.default_max_query_tokens(eng.S), *eng._special_ids())


def oracle_top(logits, types, lens, goff, max_len):
    """Per question: the oracle's best span ``(pair in group, i, j)`` over all its pairs, its lead over the
    runner-up, from fp32 ``logits [P, S, 2]``."""
    span, score, _ = ops.span_select_ref(logits, types, lens, max_len, 2)
    out = []
    for q in range(len(goff) - 1):
        a, b = goff[q], goff[q + 1]
        flat = score[a:b].reshape(-1)
        if flat.numel() == 0 or flat.max() == NINF:
            out.append(None)
            continue
        order = torch.sort(flat, descending=True, stable=True).indices
        f = int(order[0])
        lead = float(flat[order[0]] - flat[order[1]]) if flat.numel() > 1 else float("inf")
        out.append((f // 2, tuple(span[a + f // 2, f % 2].tolist()), lead))
    return out


def _oracle_checks(res, logits_g, logits_ref, types, lens, goff, max_len):
    """Logits within the bound of test_rerank_gpu.py; a question's top-1 span equals the oracle's wherever
    the oracle's top-1 leads its runner-up by more than twice that bound. Returns how many qualified."""
    live = torch.isfinite(logits_ref)
    bound = 0.05 * logits_ref[live].abs().max().item()
    assert torch.equal(torch.isfinite(logits_g), live)
    assert (logits_g[live] - logits_ref[live]).abs().max().item() < bound
    qualified = 0
    for q, top in enumerate(oracle_top(logits_ref, types, lens, goff, max_len)):
        if top is None:
            assert res.answers[q] == []
            continue
        pair, tokens, lead = top
        if lead > 2 * bound:
            qualified += 1
            assert (res.answers[q][0]["passage"], tuple(res.answers[q][0]["tokens"])) == (pair, tokens), q
    return qualified


@pytest.fixture(scope="module")
def tiny(tmp_path_factory):
    path = tmp_path_factory.mktemp("wp") / "vocab.txt"
    with open(path, "wb") as f:
        f.write("\n".join(make_wordpiece_vocab(300, seed=1)).encode("utf-8") + b"\n")
    cfg = config_for("bert-tiny", num_labels=1, qa_head=True)
    # The seed is one at which the fp32 CPU ORACLE alone, for both tokenizers, has a question whose best
    # span leads its runner-up by more than twice the logit bound 0.05 * max|logit| (checked on the CPU
    # with oracle_top: TINY_SEED was picked from that, never from what the GPU returns).
    return cfg, init_random(cfg, seed=TINY_SEED, bias_std=0.02), T.WordPieceVocab.load(str(path))


TINY_SEED = 2  # the oracle's lead of question 1 is 2.0x (wordpiece) and 2.3x (hash) the required 2 * bound


@pytest.mark.parametrize("tokenizer", ["wordpiece", "hash"])
def test_answer_pairs_tiny(gpu, tiny, tokenizer):
    cfg, pack, vocab = tiny
    vocab = vocab if tokenizer == "wordpiece" else None
    kw = dict(batch_rows=16, seq_len=128, topk=1, vocab=vocab)
    eng_g = ClassifyEngine(cfg, pack, gpu, use_graph=True, **kw)
    eng_e = ClassifyEngine(cfg, pack, gpu, use_graph=False, **kw)
    flat, goff = _flat(GROUPS)
    res = eng_g.answer_pairs(QUESTIONS, flat, goff, top_k=5, max_answer_tokens=30)
    again = eng_g.answer_pairs(QUESTIONS, flat, goff, top_k=5, max_answer_tokens=30)  # replays the captured graph
    eager = eng_e.answer_pairs(QUESTIONS, flat, goff, top_k=5, max_answer_tokens=30)
    assert res.span.shape == (8, 5, 2) and res.score.shape == (8, 5) and torch.isfinite(res.null).all()
    for other in (again, eager):  # graph replay == eager == second call, bit for bit
        assert torch.equal(res.span, other.span) and torch.equal(_bits(res.score), _bits(other.score))
        assert torch.equal(_bits(res.null), _bits(other.null)) and res.answers == other.answers
    # the engine's rows are BertClassifier.spans on the twin's rows, bit for bit
    bucket = eng_g._bucket(len(flat))
    ids, types, lens = (torch.from_numpy(a) for a in _twin_rows(eng_g, QUESTIONS, flat, goff, bucket))
    assert types.any() and (lens[:8] > 3).any()
    logits_g = torch.zeros((bucket, 128, 2), device=gpu)
    direct = eng_g.model.spans(ids.to(gpu), lens.to(gpu), types.to(gpu), 30, 5, logits_out=logits_g)
    for got, want in zip((res.span, res.score, res.null), direct):
        assert torch.equal(_bits(got), _bits(want[:8]))
    # the answers are the group top-k of those rows, mapped to the passage's characters
    want_i, want_v = ops.group_topk_ref(res.score.reshape(-1), torch.tensor([5 * g for g in goff], dtype=torch.int32), 5)
    for q, row in enumerate(res.answers):
        keep = [(f, v) for f, v in zip(want_i[q].tolist(), want_v[q].tolist()) if f >= 0 and v > NINF]
        assert len(row) == len(keep)
        for e, (f, v) in zip(row, keep):  # f: the index within the question's flattened [pairs * 5] scores
            pair, slot = goff[q] + f // 5, f % 5
            assert e["passage"] == f // 5 and e["score"] == v and e["null_score"] == res.null[pair].item()
            assert tuple(e["tokens"]) == tuple(res.span[pair, slot].tolist())
            assert flat[pair][e["start"]:e["end"]] == e["text"] and e["text"]
    assert res.answers[0] == [] and len(res.answers[2]) == 5
    oracle = BertClassifier(cfg, pack, fp32=True)
    logits_ref = torch.zeros((8, 128, 2))
    oracle.spans(ids[:8], lens[:8], types[:8], 30, 5, logits_out=logits_ref)
    assert _oracle_checks(res, logits_g[:8].cpu(), logits_ref, types[:8], lens[:8], goff, 30) >= 1
    assert eng_g.memory_bytes() > eng_e.pack.nbytes


@pytest.fixture(scope="module")
def base():
    cfg = config_for("bert-base", num_labels=1, qa_head=True)
    return cfg, init_random(cfg, seed=1, bias_std=0.02)


def test_answer_bert_base_folded_path_and_unfused(gpu, base, monkeypatch):
    """16 pairs x 128 tokens: M = 2048 reaches the LayerNorm-folded fused encoder; the fused span head
    equals the ATPU_ANSWER_FUSED=0 form and the fp32 oracle within the logit bound."""
    cfg, pack = base
    eng = ClassifyEngine(cfg, pack, gpu, batch_rows=32, seq_len=128, topk=1)
    assert eng.model.can_fold(16, 128) and eng.model.answer_fused
    questions = make_text_rows(2, words_per_row=6, seed=1)
    groups = [make_text_rows(9, words_per_row=60, seed=2), make_text_rows(7, words_per_row=150, seed=3)]
    flat, goff = _flat(groups)
    res = eng.answer_pairs(questions, flat, goff, top_k=4, max_answer_tokens=30)
    ids, types, lens = (torch.from_numpy(a) for a in _twin_rows(eng, questions, flat, goff, 16))
    assert lens.max() == 128 and types.sum() > 500
    dev = [t.to(gpu) for t in (ids, lens, types)]
    logits_f = torch.zeros((16, 128, 2), device=gpu)
    fused = eng.model.spans(*dev, 30, 4, logits_out=logits_f)
    for got, want in zip((res.span, res.score, res.null), fused):
        assert torch.equal(_bits(got), _bits(want))
    monkeypatch.setenv("ATPU_ANSWER_FUSED", "0")
    plain = BertClassifier(cfg, eng.pack)
    assert not plain.answer_fused
    logits_u = torch.zeros((16, 128, 2), device=gpu)
    plain.spans(*dev, 30, 4, logits_out=logits_u)
    logits_ref = torch.zeros((16, 128, 2))
    BertClassifier(cfg, pack, fp32=True).spans(ids, lens, types, 30, 4, logits_out=logits_ref)
    live = torch.isfinite(logits_ref)
    bound = 0.05 * logits_ref[live].abs().max().item()
    lf, lu = logits_f.cpu(), logits_u.cpu()
    assert torch.equal(torch.isfinite(lf), live) and torch.equal(torch.isfinite(lu), live)
    print("fused vs unfused", (lf[live] - lu[live]).abs().max().item(), "fused vs oracle",
          (lf[live] - logits_ref[live]).abs().max().item(), "bound", bound)
    assert (lf[live] - lu[live]).abs().max().item() < bound
    _oracle_checks(res, lf, logits_ref, types, lens, goff, 30)


@pytest.fixture
def invariant():
    prev = ops.set_batch_invariant(True)
    yield
    ops.set_batch_invariant(prev)


def test_answer_rows_are_batch_invariant(gpu, base, invariant):
    """A pair's spans, scores and null score have the same bits alone, among 40 pairs, and across a chunk
    boundary (``batch_rows`` 32: 40 pairs are a chunk of 32 and one of 8, padded to the 16-row bucket)."""
    cfg, pack = base
    eng = ClassifyEngine(cfg, pack, gpu, batch_rows=32, seq_len=128, topk=1)  # its graphs are captured in this mode
    questions = make_text_rows(3, words_per_row=7, seed=11)
    groups = [make_text_rows(30, words_per_row=40, seed=12), make_text_rows(6, words_per_row=150, seed=13),
              make_text_rows(4, words_per_row=10, seed=14)]  # group 1 spans rows 30..35: both chunks
    flat, goff = _flat(groups)
    many = eng.answer_pairs(questions, flat, goff, top_k=3)
    assert many.score.shape == (40, 3)
    for q, i in ((0, 0), (0, 29), (1, 1), (1, 2), (2, 3)):  # rows 0, 29, 31 (first chunk), 32, 39 (second)
        one = eng.answer_pairs([questions[q]], [groups[q][i]], [0, 1], top_k=3)
        r = goff[q] + i
        assert torch.equal(one.span[0], many.span[r]) and torch.equal(_bits(one.score[0]), _bits(many.score[r])), (q, i)
        assert torch.equal(_bits(one.null[0]), _bits(many.null[r])), (q, i)
    half = eng.answer_pairs(questions[1:], groups[1] + groups[2], [0, 6, 10], top_k=3)
    assert torch.equal(half.span, many.span[30:]) and torch.equal(_bits(half.score), _bits(many.score[30:]))
    assert half.answers == many.answers[1:]
