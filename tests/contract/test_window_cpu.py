"""Windows over long passages ("atpu-window v1") on the CPU: the geometry by brute force, the twins against
``pair_rows`` and hand-written rows, HF's overflowing windows, ``span_select_ref`` with owned starts against
a loop over every span, ``window_best_ref``, and the ``doc_stride`` key of ``map_answer`` on a CPU engine."""
import math

import numpy as np
import pytest
import torch

from agent_tpu_amd import ops
from agent_tpu_amd import tokenizer as T
from agent_tpu_amd.utils.synthetic import make_text_rows, make_wordpiece_vocab

MODEL = "bert-tiny?qa=1&batch=4&seq=40&seed=3"


# -------------------------------------------------------------------- geometry
def test_window_geometry_by_brute_force():
    """cap 1..13, step 1..cap + 2, T 0..59: the owned ranges partition [0, T), each lies inside its window,
    every span of at most ceil((cap - step) / 2) + 1 tokens is a candidate of exactly one window, and no
    span of any length is a candidate of two."""
    for cap in range(1, 14):
        S = cap + 3  # nq = 0
        for stride in range(1, cap + 3):
            step = min(stride, cap)
            guarantee = -(-(cap - step) // 2) + 1
            for Tn in range(0, 60):
                table = T.window_table(Tn, 0, S, stride)
                W = 1 if Tn <= cap else -(-(Tn - cap) // step) + 1
                assert len(table) == W
                a = np.array([t[0] for t in table])
                n = np.array([t[1] for t in table])
                lo, hi = a + np.array([t[2] for t in table]), a + np.array([t[3] for t in table])
                assert (a == np.arange(W) * step).all() and (n == np.minimum(cap, Tn - a)).all()
                assert (n >= 1).all() or Tn == 0
                assert lo[0] == 0 and hi[-1] == Tn and (lo[1:] == hi[:-1]).all() and (lo <= hi).all()  # a partition
                assert (lo >= a).all() and (hi <= a + n).all()  # inside the window
                if Tn == 0:
                    continue
                i = np.arange(Tn).reshape(1, Tn, 1)
                j = np.arange(Tn).reshape(1, 1, Tn)
                cand = ((i >= lo.reshape(W, 1, 1)) & (i < hi.reshape(W, 1, 1)) & (j < (a + n).reshape(W, 1, 1))
                        & (j >= i)).sum(0)  # [i, j]: the windows that propose span (i, j)
                assert cand.max() <= 1, (cap, stride, Tn)
                short = (j[0] >= i[0]) & (j[0] - i[0] < guarantee)
                assert (cand[short] == 1).all(), (cap, stride, Tn)
    # the bound is tight: one token more and a span across a window's end is lost
    table = T.window_table(30, 0, 13, 4)  # cap 10, step 4, h 3, guarantee 4
    a, n, _, own_hi = table[0]
    i = a + own_hi - 1  # the last start window 0 owns: 6; the window ends at 9
    assert i + 4 - 1 <= a + n - 1 < i + 5 - 1


def test_window_table_edges_and_errors():
    assert T.window_table(0, 0, 8, 3) == [(0, 0, 0, 0)]          # an empty passage: one empty window
    assert T.window_table(5, 0, 8, 3) == [(0, 5, 0, 5)]          # T == cap
    assert T.window_table(6, 0, 8, 3) == [(0, 5, 0, 4), (3, 3, 1, 3)]
    assert T.window_table(50, 5, 8, 1) == [(0, 0, 0, 0)]         # cap == 0: one window with an empty passage
    assert T.window_table(11, 0, 8, 99) == [(0, 5, 0, 5), (5, 5, 0, 5), (10, 1, 0, 1)]  # step cut at cap
    for bad in ((-1, 0, 8, 3), (5, 6, 8, 3), (5, 0, 3, 3), (5, 0, 8, 0)):
        with pytest.raises(ValueError):
            T.window_table(*bad)


# ----------------------------------------------------------------------- twins
def _long_rows(P, L, g, lens_p=None):
    ids_p = g.integers(1000, 4000, size=(P, L)).astype(np.int32)
    lens_p = g.integers(2, L + 1, size=P).astype(np.int32) if lens_p is None else np.asarray(lens_p, np.int32)
    for r in range(P):
        ids_p[r, 0], ids_p[r, lens_p[r] - 1], ids_p[r, lens_p[r]:] = T.CLS_ID, T.SEP_ID, T.PAD_ID
    return ids_p, lens_p


def test_window_rows_equal_pair_rows_when_the_passage_fits():
    g = np.random.default_rng(0)
    S, Q, P, mq = 16, 3, 40, 4
    ids_q, lens_q = _long_rows(Q, S, g, [2, 5, 16])
    ids_p, lens_p = _long_rows(P, S, g)
    qidx = g.integers(0, Q, size=P).astype(np.int32)
    ids, types, lens = T.pair_rows(ids_q, lens_q, ids_p, lens_p, qidx, mq)
    fits = np.array([lens_p[r] - 2 <= S - 3 - min(lens_q[qidx[r]] - 2, mq) for r in range(P)])
    assert fits.sum() > 10 and (~fits).sum() > 3
    for stride in (1, 3, 99):
        wi, wt, wl, own = T.window_rows(ids_q, lens_q, ids_p, lens_p, qidx, np.arange(P), np.zeros(P), mq, stride)
        assert wi.dtype == wt.dtype == wl.dtype == own.dtype == np.int32
        assert np.array_equal(wi[fits], ids[fits]) and np.array_equal(wt[fits], types[fits])
        assert np.array_equal(wl[fits], lens[fits])
        for r in np.nonzero(fits)[0]:
            assert tuple(own[r]) == (0, lens_p[r] - 2)  # the one window owns every start
        # a first window of a longer passage is the pair row too (both are cut at cap), but owns less
        assert np.array_equal(wi[~fits], ids[~fits]) and np.array_equal(wl[~fits], lens[~fits])


def test_window_rows_hand_written_case():
    """S = 12, nq = 2, T = 17, step = 3: cap = 7, h = 2, five windows at 0, 3, 6, 9, 12."""
    S, L = 12, 24
    q = np.array([[101, 11, 12, 13, 102] + [0] * 7], np.int32)        # three question tokens, cut at mq = 2
    p = np.array([[101] + list(range(200, 217)) + [102] + [0] * 5], np.int32)
    assert T.window_table(17, 2, S, 3) == [(0, 7, 0, 5), (3, 7, 2, 5), (6, 7, 2, 5), (9, 7, 2, 5), (12, 5, 2, 5)]
    ids, types, lens, own = T.window_rows(q, [5], p, [19], [0], [0, 0, 0, 0, 0], [0, 3, 6, 9, 12], 2, 3)
    head = [101, 11, 12, 102]
    assert ids.tolist() == [head + list(range(200, 207)) + [102],
                            head + list(range(203, 210)) + [102],
                            head + list(range(206, 213)) + [102],
                            head + list(range(209, 216)) + [102],
                            head + list(range(212, 217)) + [102, 0, 0]]
    assert types.tolist() == [[0] * 4 + [1] * 8] * 4 + [[0] * 4 + [1] * 6 + [0] * 2]
    assert lens.tolist() == [12, 12, 12, 12, 10]
    assert own.tolist() == [[0, 5], [2, 5], [2, 5], [2, 5], [2, 5]]
    # table entries outside their range are clamped: pair into [0, Pp), start into [0, T - 1]
    c = T.window_rows(q, [5], p, [19], [0], [-1, 1, 0], [-1, 20, 16], 2, 3)
    w = T.window_rows(q, [5], p, [19], [0], [0, 0, 0], [0, 16, 16], 2, 3)
    for a, b in zip(c, w):
        assert np.array_equal(a, b)
    assert c[0][1].tolist() == head + [216, 102] + [0] * 6 and c[3][1].tolist() == [2, 1]
    for bad in (dict(max_query_tokens=-1), dict(doc_stride=0)):
        kw = dict(max_query_tokens=2, doc_stride=3)
        kw.update(bad)
        with pytest.raises(ValueError):
            T.window_rows(q, [5], p, [19], [0], [0], [0], **kw)


@pytest.fixture(scope="module")
def small(tmp_path_factory):
    path = tmp_path_factory.mktemp("wp") / "vocab.txt"
    with open(path, "wb") as f:
        f.write("\n".join(make_wordpiece_vocab(300, seed=1)).encode("utf-8") + b"\n")
    return str(path), T.WordPieceVocab.load(str(path))


def test_window_rows_equal_hf_overflowing_windows(small):
    """HF's ``stride`` is the overlap, ``cap - step``. Questions that fit in ``max_query_tokens``."""
    transformers = pytest.importorskip("transformers")
    path, vocab = small
    hf = transformers.BertTokenizer(path, do_lower_case=True)
    probe = hf("kalo", "kalo mira ten kalo mira ten", truncation="only_second", max_length=6, stride=0,
               return_overflowing_tokens=True)["input_ids"]
    if not isinstance(probe[0], list):  # a slow tokenizer returns the overflow as one flat list: take the fast one
        try:
            hf = transformers.BertTokenizerFast(path, do_lower_case=True)
        except Exception as exc:
            pytest.skip(f"no tokenizer that returns overflowing windows as rows: {exc}")
    L = 400
    saw_many = 0
    for S, question, words, strides in ((16, "kalo mira", 14, (1, 3, 8)), (16, "", 9, (2, 13)),
                                        (24, "ten ten kalo mira ten", 30, (5, 16)), (12, "kalo", 2, (3,))):
        passage = " ".join(make_text_rows(1, words_per_row=words, seed=S + words))
        ids_q, lens_q = vocab.tokenize_rows([question.encode()], S)
        ids_p, lens_p = vocab.tokenize_rows([passage.encode()], L)
        nq, Tn = int(lens_q[0]) - 2, int(lens_p[0]) - 2
        cap = S - 3 - nq
        assert nq <= T.default_max_query_tokens(S) and Tn < L - 2
        for stride in strides:
            step = min(stride, cap)
            enc = hf(question, passage, truncation="only_second", max_length=S, stride=cap - step,
                     return_overflowing_tokens=True, padding="max_length")
            table = T.window_table(Tn, nq, S, stride)
            ids, types, lens, _ = T.window_rows(ids_q, lens_q, ids_p, lens_p, [0], [0] * len(table),
                                                [t[0] for t in table], T.default_max_query_tokens(S), stride,
                                                vocab.cls_id, vocab.sep_id, vocab.pad_id)
            assert ids.tolist() == enc["input_ids"], (S, stride)
            assert types.tolist() == enc["token_type_ids"], (S, stride)
            assert lens.tolist() == [sum(m) for m in enc["attention_mask"]], (S, stride)
            saw_many += len(table) > 2
    assert saw_many >= 3


# ------------------------------------------------- span_select_ref with own
def _brute_own(lg, types, length, max_len, n, own):
    """Every (i, j) in a Python loop; the order is (value desc, i * S + j asc) with NaN as -inf."""
    S = lg.shape[0]
    ln = min(max(int(length), 2), S)
    ones = [j for j in range(S) if int(types[j]) == 1]
    lo, hi = (ones[0] if ones else S), ln - 2
    o0, o1 = (min(max(int(v), 0), S) for v in own)
    cand = []
    for i in range(lo, hi + 1):
        if not lo + o0 <= i < lo + o1:
            continue
        for j in range(i, min(hi, i + max_len - 1) + 1):
            v = np.float32(lg[i, 0]) + np.float32(lg[j, 1])
            v = np.float32("-inf") if np.isnan(v) else v
            cand.append((-float(v), i * S + j, v))  # -0.0 == 0.0 in the key: they tie
    cand.sort(key=lambda c: c[:2])
    span = np.full((n, 2), -1, np.int32)
    score = np.full(n, -np.inf, np.float32)
    for r, (_, f, v) in enumerate(cand[:n]):
        span[r] = (f // S - lo, f % S - lo)
        score[r] = v
    return span, score


@pytest.mark.parametrize("S", [7, 24])
def test_span_select_ref_with_own_equals_brute_force(S):
    g = torch.Generator().manual_seed(S)
    B = 10
    values = torch.tensor([-1.0, -0.0, 0.0, 2.5])
    lg = values[torch.randint(0, 4, (B, S, 2), generator=g)]
    lg[9] = torch.randn(S, 2, generator=g)
    lg[1, 3, 0] = float("nan")
    q = (S - 4) // 3
    types = torch.zeros((B, S), dtype=torch.int32)
    types[:, q + 2:] = 1
    lens = torch.full((B,), S, dtype=torch.int32)
    lens[8] = S - 2
    types[8, S - 2:] = 0
    own = torch.tensor([[0, S], [0, S], [2, 2], [1, 2], [3, 1], [-4, 2], [2, S + 9], [S, S], [1, S], [1, 3]],
                       dtype=torch.int32)  # full, full, empty, one start, inverted, below 0, past the end, ...
    for n in (1, 4, 32):
        for max_len in sorted({1, 3, S}):
            span, score, null = ops.span_select_ref(lg, types, lens, max_len, n, own)
            plain = ops.span_select_ref(lg, types, lens, max_len, n)
            for b in range(B):
                want_s, want_v = _brute_own(lg[b].numpy(), types[b].numpy(), lens[b], max_len, n, own[b].tolist())
                assert np.array_equal(span[b].numpy(), want_s), (S, n, max_len, b)
                assert np.array_equal(score[b].numpy().view(np.int32), want_v.view(np.int32)), (S, n, max_len, b)
            assert torch.equal(null, plain[2])
            assert torch.equal(span[:2], plain[0][:2]) and torch.equal(score[:2], plain[1][:2])  # own = everything
            assert span[2].eq(-1).all() and span[4].eq(-1).all() and span[7].eq(-1).all()
            assert (span[3, :, 0][span[3, :, 0] >= 0] == 1).all()


def test_window_best_ref_and_cpu_path():
    n = 3
    span_w = torch.tensor([[[0, 1], [2, 2], [-1, -1]], [[1, 1], [0, 0], [3, 4]], [[2, 3], [-1, -1], [-1, -1]],
                           [[5, 5], [6, 6], [7, 7]]], dtype=torch.int32)
    ninf, nan = float("-inf"), float("nan")
    score_w = torch.tensor([[2.0, 1.0, ninf], [2.0, nan, 0.5], [3.0, ninf, ninf], [9.0, 8.0, 7.0]])
    null_w = torch.tensor([0.5, -1.5, nan, 4.0])
    start = torch.tensor([0, 10, 20, 30], dtype=torch.int32)
    wrow = torch.tensor([0, 3, 3, 4, 9], dtype=torch.int32)  # pairs of 3, 0, 1 and (clamped) 0 rows
    span, score, null = ops.window_best_ref(span_w, score_w, null_w, start, wrow)
    assert span[0].tolist() == [[22, 23], [0, 1], [11, 11]]  # 3.0, then the 2.0 tie in (row, slot) order
    assert score[0].tolist() == [3.0, 2.0, 2.0] and null[0].item() == -1.5  # the NaN null is skipped
    assert span[1].eq(-1).all() and (score[1] == ninf).all() and null[1].item() == float("inf")
    assert span[2].tolist() == [[35, 35], [36, 36], [37, 37]] and null[2].item() == 4.0
    assert span[3].eq(-1).all() and null[3].item() == float("inf")
    # more slots than elements: -inf elements keep their place in index order, exhausted ones stay (-1, -1)
    sp5, sc5, _ = ops.window_best_ref(span_w[:, :1].contiguous(), score_w[:, :1].contiguous(), null_w, start,
                                      torch.tensor([0, 1], dtype=torch.int32))
    assert sp5.tolist() == [[[0, 1]]] and sc5.tolist() == [[2.0]]
    out = (torch.full((6, n, 2), -7, dtype=torch.int32), torch.full((6, n), -7.0), torch.full((6,), -7.0))
    got = ops.window_best(span_w, score_w, null_w, start, wrow, span=out[0], score=out[1], null=out[2])
    assert torch.equal(got[0][:4], span) and torch.equal(got[1][:4], score) and torch.equal(got[2][:4], null)
    assert all(o[4:].eq(-7).all() for o in out)  # rows past P are not touched
    fresh = ops.window_best(span_w, score_w, null_w, start, wrow)
    assert torch.equal(fresh[0], span)
    with pytest.raises(ValueError):
        ops.window_best(span_w, score_w.double(), null_w, start, wrow)
    with pytest.raises(ValueError):
        ops.window_best(span_w, score_w, null_w[:3], start, wrow)
    with pytest.raises(ValueError):
        ops.window_best(span_w[:, :2].contiguous(), score_w, null_w, start, wrow)
    with pytest.raises(ValueError):
        ops.window_best(span_w, score_w, null_w, start.long(), wrow)


def test_window_assemble_cpu_path_and_checks():
    g = np.random.default_rng(1)
    S, L, Q, P = 12, 30, 2, 3
    ids_q, lens_q = _long_rows(Q, S, g, [4, 9])
    ids_p, lens_p = _long_rows(P, L, g, [30, 2, 11])
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32))  # noqa: E731
    args = [t(ids_q), t(lens_q), t(ids_p), t(lens_p), t([1, 0, 0]), t([0, 0, 0, 1, 2]), t([0, 4, 8, 0, 0])]
    got = ops.window_assemble(*args, 3, 4)
    want = T.window_rows(ids_q, lens_q, ids_p, lens_p, [1, 0, 0], [0, 0, 0, 1, 2], [0, 4, 8, 0, 0], 3, 4)
    for a, b in zip(got, want):
        assert a.dtype == torch.int32 and np.array_equal(a.numpy(), b)
    out = [torch.full((7, S), -7, dtype=torch.int32), torch.full((7, S), -7, dtype=torch.int32),
           torch.full((7,), -7, dtype=torch.int32), torch.full((7, 2), -7, dtype=torch.int32)]
    ops.window_assemble(*args, 3, 4, ids=out[0], type_ids=out[1], lens=out[2], own=out[3], rows=4)
    for o, b in zip(out, want):
        assert np.array_equal(o[:4].numpy(), b[:4]) and o[4:].eq(-7).all()  # rows past `rows` are not touched
    for kw in (dict(mq=-1), dict(mq=True), dict(stride=0), dict(stride=2.0)):
        a = dict(mq=3, stride=4)
        a.update(kw)
        with pytest.raises(ValueError):
            ops.window_assemble(*args, a["mq"], a["stride"])
    with pytest.raises(ValueError):  # the outputs come together
        ops.window_assemble(*args, 3, 4, ids=out[0])
    with pytest.raises(ValueError):
        ops.window_assemble(*(args[:5] + [args[5].long(), args[6]]), 3, 4)
    with pytest.raises(ValueError):  # qidx must name every passage row
        ops.window_assemble(*(args[:4] + [t([0, 0]), args[5], args[6]]), 3, 4)


# ------------------------------------------------------------- engine and op
@pytest.fixture()
def cpu_handle(monkeypatch):
    monkeypatch.setenv("CLASSIFY_DEVICE", "cpu")
    from ops._gpu_runtime import get_gpu_handle

    return get_gpu_handle(MODEL)


@pytest.fixture()
def op(monkeypatch):
    monkeypatch.setenv("CLASSIFY_DEVICE", "cpu")
    from ops import get_batch_op, get_op

    return get_op("map_answer"), get_batch_op("map_answer")


QUESTIONS = ["how do gpus multiply matrices", "weather tomorrow", "empty list"]
SHORT = [["matrix cores multiply tiles", "a recipe for bread", "", "gpus have many compute units",
          "gpus multiply matrices with matrix cores, naïve café", "rain is likely", "x"],
         ["rain is likely tomorrow", "sunny"], []]
LONG = [make_text_rows(3, words_per_row=60, seed=2) + ["", "short one"], make_text_rows(2, words_per_row=25, seed=3),
        []]


def test_engine_reads_past_the_first_window(cpu_handle):
    """A long passage on the CPU device: the per-pair rows are ``model.spans(own=)`` on the twin's window rows
    folded by ``window_best_ref``, and answers come from later windows. The model seed (``seed=3`` in MODEL) is
    one at which this CPU engine, the oracle of the GPU tests, returns an answer that starts past the first
    window; it was chosen on the CPU alone."""
    h, eng = cpu_handle, cpu_handle.engine
    S, stride, n = eng.S, 8, 3
    flat = [p for ps in LONG for p in ps]
    goff = [0, 5, 7, 7]
    res = eng.answer_pairs(QUESTIONS, flat, goff, top_k=n, doc_stride=stride)
    L = eng.max_row_bytes + 2
    mq = T.default_max_query_tokens(S)
    ids_q, lens_q = T.tokenize_rows([q.encode() for q in QUESTIONS], S, h.cfg.vocab_size)
    ids_p, lens_p = T.tokenize_rows([p.encode() for p in flat], L, h.cfg.vocab_size)
    qidx = np.repeat(np.arange(3), np.diff(goff)).astype(np.int32)
    pair, start, wrow, caps = [], [], [0], []
    for r in range(len(flat)):
        nq = min(int(lens_q[qidx[r]]) - 2, mq)
        table = T.window_table(int(lens_p[r]) - 2, nq, S, stride)
        pair += [r] * len(table)
        start += [t[0] for t in table]
        wrow.append(len(pair))
        caps.append(S - 3 - nq)
    assert res.window_count == len(pair) == int(eng.window_counts.sum()) and max(np.diff(wrow)) >= 5
    assert eng.window_counts.tolist() == np.diff(wrow).tolist()
    ids, types, lens, own = (torch.from_numpy(a) for a in
                             T.window_rows(ids_q, lens_q, ids_p, lens_p, qidx, pair, start, mq, stride))
    sp, sc, nl = eng.model.spans(ids, lens, types, 30, n, own=own)
    span, score, null = ops.window_best_ref(sp, sc, nl, torch.tensor(start, dtype=torch.int32),
                                            torch.tensor(wrow, dtype=torch.int32))
    assert torch.equal(res.span, span)
    torch.testing.assert_close(res.score, score, atol=1e-5, rtol=1e-5)  # the CPU path is not batch-invariant
    torch.testing.assert_close(res.null, null, atol=1e-5, rtol=1e-5)
    later = 0
    for q, row in enumerate(res.answers):
        for e in row:
            r = goff[q] + e["passage"]
            p = flat[r]
            assert p[e["start"]:e["end"]] == e["text"] and e["text"]
            t0, t1 = e["tokens"]
            toks = T.token_spans(p.encode(), h.cfg.vocab_size, L - 2)
            assert p.encode()[toks[t0][0]:toks[t1][1]].decode() == e["text"]
            later += t0 >= caps[r]
    assert later >= 1  # an answer the unwindowed reader cannot return
    plain = eng.answer_pairs(QUESTIONS, flat, goff, top_k=n)
    assert plain.window_count is None
    assert all(e["tokens"][1] < caps[goff[q] + e["passage"]] for q, row in enumerate(plain.answers) for e in row)
    for bad in (0, S - 2, True, 2.0):
        with pytest.raises(ValueError):
            eng.answer_pairs(QUESTIONS, flat, goff, doc_stride=bad)


def _same_answers(got, want, skip=()):
    strip = lambda r: [[{k: v for k, v in e.items() if k not in ("score", "null_score", "probability")} for e in x]  # noqa: E731
                       for x in r["answers"]]
    assert strip(got) == strip(want)
    for key in ("score", "null_score", "probability"):
        flat = lambda r: [e[key] for x in r["answers"] for e in x]  # noqa: E731
        np.testing.assert_allclose(flat(got), flat(want), atol=1e-5, rtol=0)
    skip = ("elapsed_ms", "pairs_per_sec", "answers", "null_scores") + tuple(skip)
    assert {k: v for k, v in got.items() if k not in skip} == {k: v for k, v in want.items() if k not in skip}


def test_op_doc_stride_key(op):
    run, _ = op
    import os

    import ops.map_answer as ma

    # passages that all fit: the answers of the job without the key
    base = {"questions": QUESTIONS, "passages": SHORT, "model_path": MODEL, "top_k": 4, "return_null_scores": True}
    plain, fit = run(base), run(dict(base, doc_stride=16))
    assert "doc_stride" not in plain and "window_count" not in plain
    assert fit["doc_stride"] == 16 and fit["window_count"] == 9 == fit["pair_count"]
    _same_answers(fit, plain, skip=("doc_stride", "window_count"))
    np.testing.assert_allclose(sum(fit["null_scores"], []), sum(plain["null_scores"], []), atol=1e-5, rtol=0)
    # both payload forms on long passages
    many = run({"questions": QUESTIONS, "passages": LONG, "model_path": MODEL, "doc_stride": 8})
    assert many["ok"] and many["window_count"] > many["pair_count"] == 7 and many["doc_stride"] == 8
    for q, row in enumerate(many["answers"]):
        assert [e["score"] for e in row] == sorted((e["score"] for e in row), reverse=True)
        for e in row:
            assert LONG[q][e["passage"]][e["start"]:e["end"]] == e["text"] and e["text"]
        if row:
            assert abs(math.fsum(e["probability"] for e in row) - 1.0) < 1e-12
    one = run({"question": QUESTIONS[0], "passages": LONG[0], "model_path": MODEL, "doc_stride": 8})
    assert one["query_count"] == 1 and 5 < one["window_count"] < many["window_count"]
    _same_answers({"answers": one["answers"][:1]}, {"answers": many["answers"][:1]})
    plain_long = run({"question": QUESTIONS[0], "passages": LONG[0], "model_path": MODEL})
    assert max(e["end"] for e in one["answers"][0]) > max(e["end"] for e in plain_long["answers"][0])
    # the error, before and after the model is known
    msg = ma.WINDOW_ERRORS["doc_stride"]
    assert msg == "payload.doc_stride must be an integer in [1, seq_len - 3]"
    for bad in (0, -3, 38, "8", 8.0, True):  # seq = 40: [1, 37]
        with pytest.raises(ValueError) as e:
            run(dict(base, doc_stride=bad))
        assert str(e.value) == msg, bad
    assert run(dict(base, doc_stride=37))["ok"] and run(dict(base, doc_stride=1))["ok"]
    contract = open(os.path.join(os.path.dirname(ma.__file__), "map_answer.CONTRACT.md")).read()
    assert msg in contract and "doc_stride" in contract and "window_count" in contract
    assert "ceil((cap - step) / 2) + 1" in contract


def test_batched_doc_stride_jobs_equal_single_jobs(op):
    run, batch = op
    jobs = [{"questions": QUESTIONS, "passages": LONG, "model_path": MODEL, "top_k": 2, "doc_stride": 8},
            {"question": QUESTIONS[1], "passages": LONG[0], "model_path": MODEL, "top_k": 5, "doc_stride": 8,
             "return_null_scores": True},
            {"question": QUESTIONS[0], "passages": LONG[1], "model_path": MODEL},            # another group: no key
            {"question": QUESTIONS[0], "passages": LONG[1], "model_path": MODEL, "doc_stride": 5},
            {"question": QUESTIONS[0], "passages": LONG[1], "model_path": MODEL, "doc_stride": 0},
            {"question": "q", "passages": [], "model_path": MODEL, "doc_stride": 8}]
    res = batch(jobs)
    assert [r[0] for r in res] == ["ok", "ok", "ok", "ok", "err", "ok"]
    assert str(res[4][1]) == "payload.doc_stride must be an integer in [1, seq_len - 3]"
    for job, (kind, got) in zip(jobs, res):
        if kind == "ok":
            want = run(job)
            _same_answers(got, want)
            assert got.get("window_count") == want.get("window_count")
            if "null_scores" in want:
                np.testing.assert_allclose(sum(got["null_scores"], []), sum(want["null_scores"], []), atol=1e-5)
    assert res[0][1]["window_count"] > 7 and res[5][1]["window_count"] == 0 and "window_count" not in res[2][1]
