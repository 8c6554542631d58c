"""Windows over long passages on the GPU: ``window_assemble`` bit-equal to the twin on every edge of the
geometry and on clamped table entries, ``span_topk`` with owned starts bit-equal to ``span_select_ref`` on the
kernel's own logits, ``window_best`` bit-equal to its reference, and ``ClassifyEngine.answer_pairs`` with
``doc_stride`` against ``BertClassifier.spans(own=)`` on the twin's window rows, its own eager form, the
unwindowed call where every passage fits, the fp32 CPU oracle, and itself across batch compositions."""
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


def _inside(t, gpu, pad=64):
    """``t`` on the device as a slice from the middle of a larger allocation (``pad`` rows of -3 either side),
    so that an index a little outside the tensor stays inside an allocation."""
    t = torch.as_tensor(t, dtype=torch.int32)
    big = torch.full((t.shape[0] + 2 * pad,) + tuple(t.shape[1:]), -3, dtype=torch.int32, device=gpu)
    big[pad:pad + t.shape[0]] = t.to(gpu)
    return big[pad:pad + t.shape[0]]


# ------------------------------------------------------------ window_assemble
def _assemble_case(S, L, mq):
    """Question rows of 0, mq and more than mq tokens; per question and stride, passages of every length at
    which the geometry takes another path, each with all of its table's windows."""
    g = np.random.default_rng(S * 1000 + L)
    nqs = [0, mq, min(mq + 3, S - 2)]
    Q = len(nqs)
    ids_q = g.integers(1000, 30000, size=(Q, S)).astype(np.int32)
    lens_q = np.array([n + 2 for n in nqs], np.int32)
    cases = []  # (stride, ids_p, lens_p, qidx, win_pair, win_start)
    for stride_kind in ("one", "cap", "cap+5"):
        lens_p, qidx = [], []
        # cap depends on the question: one stride per launch, so "cap" means the cap of question 1
        cap1 = S - 3 - min(nqs[1], mq)
        stride = {"one": 1, "cap": cap1, "cap+5": cap1 + 5}[stride_kind]
        for q in range(Q):
            cap = S - 3 - min(nqs[q], mq)
            step = min(stride, cap)
            for Tn in (0, 1, cap - 1, cap, cap + 1, cap + step, cap + step + 1, L - 2):
                lens_p.append(min(max(Tn, 0), L - 2) + 2)
                qidx.append(q)
        Pp = len(lens_p)
        ids_p = g.integers(1000, 30000, size=(Pp, L)).astype(np.int32)
        pair, start = [], []
        for p in range(Pp):
            nq = min(nqs[qidx[p]], mq)
            table = T.window_table(lens_p[p] - 2, nq, S, stride)
            if len(table) > 12:  # stride 1 over a long row: the first, some middle and the last windows
                table = table[:4] + table[len(table) // 2:len(table) // 2 + 3] + table[-4:]
            pair += [p] * len(table)
            start += [t[0] for t in table]
        if len(pair) % 4 == 0:  # R is not a multiple of the four rows of a workgroup
            pair.append(0), start.append(0)
        cases.append((stride, ids_p, np.array(lens_p, np.int32), np.array(qidx, np.int32), np.array(pair, np.int32),
                      np.array(start, np.int32)))
    return ids_q, lens_q, cases


@pytest.mark.parametrize("L", [18, 258])
@pytest.mark.parametrize("S", [8, 16, 128])
def test_window_assemble_equals_twin(gpu, S, L):
    mq = T.default_max_query_tokens(S)
    ids_q, lens_q, cases = _assemble_case(S, L, mq)
    cls_id, sep_id, pad_id = 7, 8, 9
    for stride, ids_p, lens_p, qidx, pair, start in cases:
        R, Pp = len(pair), len(lens_p)
        assert R % 4 != 0
        want = T.window_rows(ids_q, lens_q, ids_p, lens_p, qidx, pair, start, mq, stride, cls_id, sep_id, pad_id)
        # the twin's own on the table's starts is the table's (own_lo, own_hi)
        dev = [_inside(a, gpu) for a in (ids_q, lens_q, ids_p, lens_p, qidx, pair, start)]
        out = [torch.full((R + 3, S), -7, dtype=torch.int32, device=gpu),
               torch.full((R + 3, S), -7, dtype=torch.int32, device=gpu),
               torch.full((R + 3,), -7, dtype=torch.int32, device=gpu),
               torch.full((R + 3, 2), -7, dtype=torch.int32, device=gpu)]
        ops.window_assemble(*dev, mq, stride, cls_id, sep_id, pad_id, ids=out[0], type_ids=out[1], lens=out[2],
                            own=out[3], rows=R)
        for o, w, name in zip(out, want, ("ids", "type_ids", "lens", "own")):
            assert np.array_equal(o[:R].cpu().numpy(), w), (S, L, stride, name)
            assert o[R:].eq(-7).all(), (S, L, stride, name)  # rows past R are untouched
        fresh = ops.window_assemble(*dev, mq, stride, cls_id, sep_id, pad_id)
        for o, w in zip(fresh, want):
            assert np.array_equal(o.cpu().numpy(), w)
        # entries just outside their range give the twin's result on the clamped values
        bad_pair = np.concatenate([pair[:5], [-1, Pp, -1, Pp]]).astype(np.int32)
        Tn = lens_p - 2
        last = Pp - 1
        bad_start = np.concatenate([[-1, Tn[pair[1]] + 3, -1, Tn[pair[3]] + 3, start[4]],
                                    [0, 0, Tn[0] + 3, Tn[last] + 3]]).astype(np.int32)
        ok_pair = np.clip(bad_pair, 0, Pp - 1)
        ok_start = np.array([min(max(s, 0), max(Tn[p] - 1, 0)) for s, p in zip(bad_start, ok_pair)], np.int32)
        got = ops.window_assemble(*dev[:5], _inside(bad_pair, gpu), _inside(bad_start, gpu), mq, stride, cls_id, sep_id,
                                  pad_id)
        want_c = T.window_rows(ids_q, lens_q, ids_p, lens_p, qidx, ok_pair, ok_start, mq, stride, cls_id, sep_id, pad_id)
        twin_c = T.window_rows(ids_q, lens_q, ids_p, lens_p, qidx, bad_pair, bad_start, mq, stride, cls_id, sep_id,
                               pad_id)
        for o, w, t in zip(got, want_c, twin_c):
            assert np.array_equal(o.cpu().numpy(), w) and np.array_equal(t, w), (S, L, stride)
    with pytest.raises(ValueError):
        ops.window_assemble(*dev, mq, 0)
    with pytest.raises(ValueError):
        ops.window_assemble(*dev, -1, 3)


# -------------------------------------------------------- span_topk with own
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


@pytest.mark.parametrize("S", [7, 128])
def test_span_topk_with_own_equals_ref_on_own_logits(gpu, S):
    B, (x, lens, types, u, su, c, fin) = _tie_rows(S, gpu)
    np_ = S - 2 - (S - 4) // 3  # the passage tokens of a full row
    owns = {"empty": (2, 2), "one start": (1, 2), "full": (0, S), "past the end": (np_ - 1, np_ + 40),
            "below zero": (-9, 3), "middle": (np_ // 3, 2 * np_ // 3 + 1)}
    for use_fin in (True, False):
        f = fin if use_fin else None
        for n in (1, 3, 32):
            for max_len in sorted({1, min(30, S), S}):
                plain_lg = torch.zeros((B, S, 2), device=gpu)
                plain = ops.span_topk(x, lens, types, B, u, su, c, max_len, n, fin=f, logits_out=plain_lg)
                for name, (o0, o1) in owns.items():
                    own = torch.tensor([[o0, o1]] * B, dtype=torch.int32, device=gpu)
                    logits = torch.zeros((B, S, 2), device=gpu)
                    out = ops.span_topk(x, lens, types, B, u, su, c, max_len, n, fin=f, logits_out=logits, own=own)
                    tag = (S, use_fin, n, max_len, name)
                    assert torch.equal(_bits(logits), _bits(plain_lg)), tag  # the logits do not depend on own
                    want = ops.span_select_ref(logits.cpu(), types.cpu(), lens.cpu(), max_len, n, own.cpu())
                    assert torch.equal(out[0].cpu(), want[0]), tag
                    assert torch.equal(_bits(out[1]), _bits(want[1])), tag
                    assert torch.equal(_bits(out[2]), _bits(want[2])), tag
                    span = out[0].cpu()
                    if name == "empty":
                        assert span.eq(-1).all() and (out[1] == NINF).all()
                    if name == "one start":
                        assert (span[..., 0][span[..., 0] >= 0] == 1).all() and (span[0, 0] >= 0).all()
                    if name == "full":  # without own: the same bits as own = (0, S)
                        for a, b in zip(out, plain):
                            assert torch.equal(_bits(a), _bits(b)), tag
    # a different range per row, in larger buffers: rows past B untouched
    own = torch.tensor([[0, 2], [1, S], [0, S], [0, 0], [2, 5], [0, S], [3, 4], [1, 3], [0, 1], [0, 1]],
                       dtype=torch.int32, device=gpu)
    span = torch.full((B + 2, 4, 2), -7, dtype=torch.int32, device=gpu)
    score = torch.full((B + 2, 4), -7.0, device=gpu)
    null = torch.full((B + 2,), -7.0, device=gpu)
    logits = torch.zeros((B, S, 2), device=gpu)
    ops.span_topk(x, lens, types, B, u, su, c, 3, 4, fin=fin, span=span, score=score, null=null, logits_out=logits,
                  own=own)
    want = ops.span_select_ref(logits.cpu(), types.cpu(), lens.cpu(), 3, 4, own.cpu())
    assert torch.equal(span[:B].cpu(), want[0]) and torch.equal(_bits(score[:B]), _bits(want[1]))
    assert span[B:].eq(-7).all() and score[B:].eq(-7).all() and null[B:].eq(-7).all()
    for bad in (own[:B - 1], own.long(), own[:, :1].contiguous(), own.cpu()):
        with pytest.raises(ValueError):
            ops.span_topk(x, lens, types, B, u, su, c, 3, 4, fin=fin, own=bad)


# ---------------------------------------------------------------- window_best
@pytest.mark.parametrize("n", [1, 5, 32])
def test_window_best_equals_ref(gpu, n):
    g = torch.Generator().manual_seed(n)
    rows = [0, 1, 3, 70, 2, 0, 5]  # window rows per pair
    R, P = sum(rows), len(rows)
    wrow = torch.tensor(np.concatenate([[0], np.cumsum(rows)]), dtype=torch.int32)
    values = torch.tensor([-1.5, 0.0, -0.0, 2.5, 7.0, NINF])
    score_w = values[torch.randint(0, 6, (R, n), generator=g)]  # heavy ties across windows, signed zeros, -inf
    score_w[4 + 7, 0] = float("nan")
    score_w[4 + 30] = torch.randn(n, generator=g)
    score_w[4 + 69, n - 1] = float("nan")
    span_w = torch.randint(0, 30, (R, n, 2), generator=g, dtype=torch.int32)
    span_w[score_w == NINF] = -1  # exhausted slots of a window row
    span_w[4 + 3, 0] = torch.tensor([4, 9], dtype=torch.int32)  # a real span whose score is -inf
    score_w[4 + 3, 0] = NINF
    null_w = torch.randn(R, generator=g) * 3
    null_w[2], null_w[4 + 10] = float("nan"), NINF
    null_w[R - 5:] = torch.tensor([1.0, float("nan"), 0.5, float("nan"), 2.0])
    start = torch.randint(0, 2000, (R,), generator=g, dtype=torch.int32)
    want = ops.window_best_ref(span_w, score_w, null_w, start, wrow)
    assert want[2][0].item() == float("inf") and want[2][3].item() == NINF and want[2][6].item() == 0.5
    assert want[0][0].eq(-1).all() and (want[1][0] == NINF).all()
    dev = [t.to(gpu) for t in (span_w, score_w, null_w, start, wrow)]
    out = (torch.full((P + 2, n, 2), -7, dtype=torch.int32, device=gpu), torch.full((P + 2, n), -7.0, device=gpu),
           torch.full((P + 2,), -7.0, device=gpu))
    ops.window_best(*dev, span=out[0], score=out[1], null=out[2])
    fresh = ops.window_best(*dev)
    for o, f, w, name in zip(out, fresh, want, ("span", "score", "null")):
        assert torch.equal(_bits(o[:P]), _bits(w)), (n, name)
        assert torch.equal(_bits(f), _bits(w)), (n, name)
        assert o[P:].eq(-7).all(), (n, name)
    assert (want[1] != want[1]).sum() == 0  # a NaN score is returned as -inf
    # offsets outside [0, R] are clamped, a decreasing pair is an empty range (the offsets sit inside a larger tensor)
    odd = torch.tensor([-2, 3, 2, R + 5, R + 9], dtype=torch.int32)
    got = ops.window_best(*dev[:4], _inside(odd, gpu))
    want_o = ops.window_best_ref(span_w, score_w, null_w, start, odd)
    for a, b in zip(got, want_o):
        assert torch.equal(_bits(a), _bits(b))
    with pytest.raises(ValueError):
        ops.window_best(dev[0], dev[1], dev[2][:R - 1], dev[3], dev[4])


# --------------------------------------------------------------------- engine
QUESTIONS = ["how do gpus multiply matrices", "Weather tomorrow?", "kalo mira ten"]


def _flat(groups):
    goff = [0]
    for g in groups:
        goff.append(goff[-1] + len(g))
    return [p for g in groups for p in g], goff


def _twin_windows(eng, questions, flat, goff, stride):
    """The window rows of an engine call by the Python twins: ``(ids, types, lens, own, start, wrow, caps)``."""
    enc = lambda rows: [r.encode() for r in rows]  # noqa: E731
    L = eng.max_row_bytes + 2
    if eng.vocab is not None:
        tok = lambda rows, S: eng.vocab.tokenize_rows(enc(rows), S)  # noqa: E731
    else:
        tok = lambda rows, S: T.tokenize_rows(enc(rows), S, eng.cfg.vocab_size)  # noqa: E731
    mq = T.default_max_query_tokens(eng.S)
    ids_q, lens_q = tok(questions, eng.S)
    ids_p, lens_p = tok(flat, L)
    qidx = np.repeat(np.arange(len(questions)), np.diff(goff)).astype(np.int32)
    pair, start, wrow, caps = [], [], [0], []
    for r in range(len(flat)):
        nq = min(int(lens_q[qidx[r]]) - 2, mq)
        table = T.window_table(int(lens_p[r]) - 2, nq, eng.S, stride)
        pair += [r] * len(table)
        start += [t[0] for t in table]
        wrow.append(len(pair))
        caps.append(eng.S - 3 - nq)
    rows = T.window_rows(ids_q, lens_q, ids_p, lens_p, qidx, pair, start, mq, stride, *eng._special_ids())
    return tuple(torch.from_numpy(a) for a in rows) + (torch.tensor(start, dtype=torch.int32),
                                                       torch.tensor(wrow, dtype=torch.int32), caps)


def oracle_top(logits, types, lens, own, start, wrow, goff, max_len):
    """Per question: the oracle's best span ``(pair in group, i, j)`` (passage-absolute) over all its pairs'
    windows, and its lead over the runner-up, from fp32 ``logits [R, S, 2]``."""
    sp, sc, nl = ops.span_select_ref(logits, types, lens, max_len, 2, own)
    span, score, _ = ops.window_best_ref(sp, sc, nl, start, wrow)
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


def _oracle_checks(res, logits_g, logits_ref, tops):
    """The rule of test_answer_gpu.py with its bound: logits within 0.05 * max|logit| of the fp32 oracle; a
    question's top-1 span equals the oracle's wherever the oracle's top-1 leads its runner-up by more than
    twice that bound. Returns how many qualified."""
    live = torch.isfinite(logits_ref)
    bound = 0.05 * logits_ref[live].abs().max().item()
    assert torch.equal(torch.isfinite(logits_g), live)
    assert (logits_g[live] - logits_ref[live]).abs().max().item() < bound
    qualified = 0
    for q, top in enumerate(tops):
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
    return cfg, init_random(cfg, seed=WINDOW_SEED, bias_std=0.02), T.WordPieceVocab.load(str(path))


# Chosen from the fp32 CPU ORACLE alone (oracle_top and the oracle's own top 5, never from what the GPU returns), as
# TINY_SEED is in test_answer_gpu.py. WordPiece: the oracle's best span of question 2 starts at token 56, in a later
# window, and leads its runner-up by 2.4x the required 2 * bound (question 1: 2.1x); its top 5 hold three answers
# from later windows. Hash: three answers from later windows, no lead that qualifies.
WINDOW_SEED = 10


def _long_groups(tokenizer):
    """Passages of 0 tokens, fewer than cap, and 3 to 9 windows at S = 32 / doc_stride 8 (the WordPiece
    vocabulary of 300 entries cuts a word into about three pieces, the hash tokenizer into one): more window
    rows than batch_rows = 16."""
    words = lambda n, seed: " ".join(make_text_rows(1, words_per_row=n, seed=seed))  # noqa: E731
    w = (13, 18, 23, 27) if tokenizer == "wordpiece" else (34, 48, 62, 76)
    return [[], ["a recipe for bread"],
            ["matrix cores multiply tiles", "", words(w[0], 1), "rain, then sun", words(w[1], 2), words(w[2], 3),
             "it's (not) here", words(w[3], 4), "x"]]


@pytest.mark.parametrize("tokenizer", ["wordpiece", "hash"])
def test_answer_pairs_windows_tiny(gpu, tiny, tokenizer):
    cfg, pack, vocab = tiny
    vocab = vocab if tokenizer == "wordpiece" else None
    S, stride, n = 32, 8, 5
    kw = dict(batch_rows=16, seq_len=S, topk=1, vocab=vocab)
    eng_g = ClassifyEngine(cfg, pack, gpu, use_graph=True, **kw)
    eng_e = ClassifyEngine(cfg, pack, gpu, use_graph=False, **kw)
    flat, goff = _flat(_long_groups(tokenizer))
    call = lambda eng: eng.answer_pairs(QUESTIONS, flat, goff, top_k=n, max_answer_tokens=10, doc_stride=stride)  # noqa: E731
    res, again, eager = call(eng_g), call(eng_g), call(eng_e)
    ids, types, lens, own, start, wrow, caps = _twin_windows(eng_g, QUESTIONS, flat, goff, stride)
    per_pair = np.diff(wrow.numpy())
    R = int(wrow[-1])
    many = [c for c in per_pair.tolist() if c > 1]
    assert R > 16 and per_pair.min() == 1 and len(many) == 4 and min(many) >= 3 and max(many) <= 9, per_pair
    assert res.window_count == R and eng_g.window_counts.tolist() == per_pair.tolist()
    assert res.span.shape == (10, n, 2) and torch.isfinite(res.null).all()
    for other in (again, eager):  # graph replay == eager == second call, bit for bit
        assert torch.equal(res.span, other.span) and torch.equal(_bits(res.score), _bits(other.score))
        assert torch.equal(_bits(res.null), _bits(other.null)) and res.answers == other.answers
    # the per-pair rows are model.spans(own=) on the twin's window rows, folded by window_best_ref, bit for bit
    Rp = (R + 15) // 16 * 16
    padr = lambda t: torch.cat([t, t[:1].expand(Rp - R, *t.shape[1:])])  # noqa: E731
    logits_g = torch.zeros((Rp, S, 2), device=gpu)
    sp, sc, nl = eng_g.model.spans(padr(ids).to(gpu), padr(lens).to(gpu), padr(types).to(gpu), 10, n,
                                   logits_out=logits_g, own=padr(own).to(gpu))
    want = ops.window_best_ref(sp[:R].cpu(), sc[:R].cpu(), nl[:R].cpu(), start, wrow)
    for got, w in zip((res.span, res.score, res.null), want):
        assert torch.equal(_bits(got), _bits(w))
    # answers from later windows map to their passage's characters
    later = 0
    for q, row in enumerate(res.answers):
        for e in row:
            r = goff[q] + e["passage"]
            assert flat[r][e["start"]:e["end"]] == e["text"] and e["text"]
            later += e["tokens"][0] >= caps[r]
    assert later >= 1
    assert res.answers[0] == [] and len(res.answers[2]) == n
    # the oracle rule of test_answer_gpu.py, its bound unchanged
    oracle = BertClassifier(cfg, pack, fp32=True)
    logits_ref = torch.zeros((R, S, 2))
    oracle.spans(ids, lens, types, 10, n, logits_out=logits_ref, own=own)
    tops = oracle_top(logits_ref, types, lens, own, start, wrow, goff, 10)
    qualified = _oracle_checks(res, logits_g[:R].cpu(), logits_ref, tops)
    if tokenizer == "wordpiece":  # see WINDOW_SEED: one of the two is an answer the unwindowed reader cannot give
        assert qualified == 2 and tops[2][1][0] >= caps[goff[2] + tops[2][0]]
    # passages that all fit: the bits of the unwindowed call
    short = [["a recipe", ""], ["matrix cores", "rain, then sun", "x"], ["it's (not)"]]
    sflat, sgoff = _flat(short)
    assert np.diff(_twin_windows(eng_g, QUESTIONS, sflat, sgoff, stride)[5].numpy()).tolist() == [1] * 6
    for eng in (eng_g, eng_e):
        a = eng.answer_pairs(QUESTIONS, sflat, sgoff, top_k=n, max_answer_tokens=10, doc_stride=stride)
        b = eng.answer_pairs(QUESTIONS, sflat, sgoff, top_k=n, max_answer_tokens=10)
        assert a.window_count == 6 and b.window_count is None
        assert torch.equal(a.span, b.span) and torch.equal(_bits(a.score), _bits(b.score))
        assert torch.equal(_bits(a.null), _bits(b.null)) and a.answers == b.answers
    assert eng_g.memory_bytes() > eng_e.pack.nbytes


@pytest.fixture(scope="module")
def base():
    cfg = config_for("bert-base", num_labels=1, qa_head=True)
    return cfg, init_random(cfg, seed=1, bias_std=0.02)


@pytest.fixture
def invariant():
    prev = ops.set_batch_invariant(True)
    yield
    ops.set_batch_invariant(prev)


def test_window_rows_are_batch_invariant(gpu, base, invariant):
    """A long pair's spans, scores and null score have the same bits alone and among others, where its
    windows fall in two chunks of window rows (``batch_rows`` 16)."""
    cfg, pack = base
    eng = ClassifyEngine(cfg, pack, gpu, batch_rows=16, seq_len=128, topk=1)
    question = make_text_rows(1, words_per_row=7, seed=11)[0]
    long = " ".join(make_text_rows(2, words_per_row=150, seed=13))       # about 4 to 5 windows at stride 64
    others = make_text_rows(14, words_per_row=40, seed=12)                # one window each
    one = eng.answer_pairs([question], [long], [0, 1], top_k=3, doc_stride=64)
    w = int(eng.window_counts[0])
    assert w >= 3
    many = eng.answer_pairs([question], others + [long], [0, 15], top_k=3, doc_stride=64)
    assert eng.window_counts.tolist() == [1] * 14 + [w] and 14 < 16 < 14 + w  # rows 14 .. 14 + w - 1: two chunks
    assert torch.equal(one.span[0], many.span[14]) and torch.equal(_bits(one.score[0]), _bits(many.score[14]))
    assert torch.equal(_bits(one.null[0]), _bits(many.null[14]))
    assert (one.span[0][:, 0] >= 0).all()
