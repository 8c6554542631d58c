"""The reader on the CPU: the pack layout with and without the span head, HF parity of the start / end
logits through the fp32 oracle, ``ops.span_topk_ref`` against a brute-force loop over every span,
``token_spans`` of both tokenizers, the character-boundary widening of the engine, and the
``map_answer`` op contract on a CPU engine, lease batching included."""
import hashlib
import math

import numpy as np
import pytest
import torch

from agent_tpu_amd import ops
from agent_tpu_amd import tokenizer as T
from agent_tpu_amd.models.bert import (BertClassifier, BertConfig, config_for, from_hf_state_dict, init_random,
                                       param_specs)
from agent_tpu_amd.utils.synthetic import make_text_rows, make_wordpiece_vocab

MODEL = "bert-tiny?qa=1&batch=4&seq=40&seed=3"


@pytest.fixture(scope="module")
def small(tmp_path_factory):
    path = tmp_path_factory.mktemp("wp") / "vocab.txt"
    with open(path, "wb") as f:
        f.write("\n".join(make_wordpiece_vocab(300, seed=1)).encode("utf-8") + b"\n")
    return str(path), T.WordPieceVocab.load(str(path))


# ---------------------------------------------------------------- pack layout
def test_pack_layout_without_and_with_the_span_head():
    cfg = config_for("bert-tiny", num_labels=3)
    qa = config_for("bert-tiny", num_labels=3, qa_head=True)
    assert BertConfig().qa_head is False and cfg.qa_head is False
    plain, with_qa = list(param_specs(cfg)), list(param_specs(qa))
    H = cfg.hidden
    assert plain[-1][0] == "cls_b" and all(not n.startswith("qa_") for n, _, _ in plain)
    assert with_qa[:-2] == plain  # only qa_w / qa_b are added, after cls_b
    assert with_qa[-2:] == [("qa_w", (2, H), torch.bfloat16), ("qa_b", (2,), torch.float32)]
    count = lambda specs: sum(math.prod(s) for _, s, _ in specs)  # noqa: E731
    assert cfg.param_count() == count(plain) and qa.param_count() == count(with_qa) == count(plain) + 2 * H + 2
    a, b = init_random(cfg, seed=5, bias_std=0.02), init_random(qa, seed=5, bias_std=0.02)
    assert list(a.names()) == [n for n, _, _ in plain] and list(b.names()) == [n for n, _, _ in with_qa]
    for name in a.names():  # rand_fill is keyed by name: the other tensors keep their bits
        assert torch.equal(a[name], b[name]), name
    assert a.buffer.numel() <= b.buffer.numel() and torch.equal(a.buffer, b.buffer[:a.buffer.numel()])
    assert b["qa_w"].float().std().item() > 0.01 and b["qa_b"].abs().sum().item() > 0
    # the bits of the pack without the head, as they were before the span head existed
    digest = hashlib.sha256(init_random(cfg, seed=0).buffer.view(torch.uint8).numpy().tobytes()).hexdigest()
    assert digest == PLAIN_PACK_SHA256


#: sha256 of init_random(bert-tiny, num_labels=3, seed=0) computed on the commit before the span head
PLAIN_PACK_SHA256 = "f885b05bb79819e9e2fc35127de95f51241096c01aa11b1a62b71d8f4aa3e714"


def test_span_inputs_fold_the_last_layernorm():
    qa = config_for("bert-tiny", qa_head=True)
    pack = init_random(qa, seed=2, bias_std=0.02)
    last = f"l{qa.layers - 1}."
    pack[last + "ln2_g"].copy_(torch.linspace(0.5, 1.5, qa.hidden))
    pack[last + "ln2_b"].copy_(torch.linspace(-0.2, 0.3, qa.hidden))
    model = BertClassifier(qa, pack)
    si = model.span_inputs()
    assert si is model.span_inputs()  # built once
    w, g, b = pack["qa_w"].double(), pack[last + "ln2_g"].double(), pack[last + "ln2_b"].double()
    assert all(t.dtype == torch.float32 for t in si.values())
    assert torch.equal(si["u"], (pack[last + "ln2_g"].view(1, -1) * pack["qa_w"].float()))
    assert torch.equal(si["su"], si["u"].double().sum(1).float())
    assert torch.equal(si["c"], ((b.view(1, -1) * w).sum(1) + pack["qa_b"].double()).float())
    assert torch.equal(si["w"], pack["qa_w"].float()) and torch.equal(si["b"], pack["qa_b"]) and not si["z"].any()
    # the fused form is the LayerNorm followed by the head
    x = torch.randn(6, qa.hidden, dtype=torch.float64)
    mu, var = x.mean(1, keepdim=True), x.var(1, unbiased=False, keepdim=True)
    rstd = 1 / torch.sqrt(var + qa.eps)
    want = ((x - mu) * rstd * g + b) @ w.t() + pack["qa_b"].double()
    fin = torch.cat([rstd, rstd * mu], 1)
    got = ops.span_logits_ref(x, torch.tensor([6]), 1, si["u"], si["su"], si["c"], fin=fin, dtype=torch.float64)
    torch.testing.assert_close(got.view(6, 2), want, atol=1e-6, rtol=1e-6)
    with pytest.raises(ValueError, match="model has no QA head"):
        BertClassifier(config_for("bert-tiny"), init_random(config_for("bert-tiny"))).span_inputs()


# ------------------------------------------------------------------ HF parity
def test_span_logits_match_hf_question_answering():
    transformers = pytest.importorskip("transformers")
    hcfg = transformers.BertConfig(vocab_size=4096, hidden_size=256, num_hidden_layers=2, num_attention_heads=4,
                                   intermediate_size=1024, max_position_embeddings=512, type_vocab_size=2,
                                   hidden_act="gelu", layer_norm_eps=1e-12, attn_implementation="eager")
    torch.manual_seed(13)
    hf = transformers.BertForQuestionAnswering(hcfg).eval()
    with torch.no_grad():
        for p in hf.parameters():  # our pack stores bf16 weights: give HF the same values
            p.copy_(p.bfloat16().float())
        hf.qa_outputs.bias.copy_(torch.tensor([0.25, -0.5]))
    sd = hf.state_dict()
    assert not any("pooler" in k or k.startswith("classifier") for k in sd)
    cfg = config_for("bert-tiny", qa_head=True)
    ours = BertClassifier(cfg, from_hf_state_dict(cfg, sd), fp32=True)
    S = 64
    rows = [r.encode() for r in make_text_rows(6, words_per_row=12, seed=4)] + [b"", b"short one"]
    ids_q, lens_q = T.tokenize_rows(rows[:2], S, 4096)
    ids_p, lens_p = T.tokenize_rows(rows, S, 4096)
    ids, types, lens = T.pair_rows(ids_q, lens_q, ids_p, lens_p, np.arange(8, dtype=np.int32) % 2, 8)
    assert types.any() and lens.min() < S and len(set(lens.tolist())) > 2  # mixed lengths
    mask = (np.arange(S)[None, :] < lens[:, None]).astype(np.int64)
    logits = torch.zeros((8, S, 2))
    with torch.no_grad():
        ref = hf(input_ids=torch.from_numpy(ids).long(), attention_mask=torch.from_numpy(mask),
                 token_type_ids=torch.from_numpy(types).long())
        span, score, null = ours.spans(torch.from_numpy(ids), torch.from_numpy(lens), torch.from_numpy(types), 10, 3,
                                       logits_out=logits)
    live = torch.from_numpy(mask).bool()
    torch.testing.assert_close(logits[..., 0][live], ref.start_logits[live], atol=2e-4, rtol=1e-4)
    torch.testing.assert_close(logits[..., 1][live], ref.end_logits[live], atol=2e-4, rtol=1e-4)
    assert torch.isinf(logits[~live]).all() and (logits[~live] < 0).all()
    torch.testing.assert_close(null, ref.start_logits[:, 0] + ref.end_logits[:, 0], atol=4e-4, rtol=1e-4)
    want = ops.span_select_ref(logits, torch.from_numpy(types), torch.from_numpy(lens), 10, 3)
    assert torch.equal(span, want[0]) and torch.equal(score, want[1])
    assert span[6].eq(-1).all()  # the empty passage has no span
    # a model without the head: the dict's qa_outputs are ignored, and spans() refuses
    plain = config_for("bert-tiny")
    assert "qa_w" not in from_hf_state_dict(plain, sd)


# -------------------------------------------------- span_topk_ref, brute force
def _brute(lg, types, length, max_len, n):
    """Every (i, j) in a Python loop; the order is (value desc, i * S + j asc) with NaN as -inf."""
    S = lg.shape[0]
    ln = min(max(int(length), 2), S)
    ones = [j for j in range(S) if int(types[j]) == 1]
    lo, hi = (ones[0] if ones else S), ln - 2
    cand = []
    for i in range(lo, hi + 1):
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


def span_cases(S, seed=0):
    """Edge rows at width ``S``: ``(logits [B, S, 2], type_ids [B, S], lens [B])`` -- heavy ties with signed
    zeros, a NaN and infinities, an empty passage, lens out of range, no type-1 position at all, type 1
    from position 0, and a plain random row."""
    g = torch.Generator().manual_seed(seed + S)
    B = 8
    values = torch.tensor([-1.0, -0.0, 0.0, 2.5])
    lg = values[torch.randint(0, 4, (B, S, 2), generator=g)]
    lg[7] = torch.randn(S, 2, generator=g)
    lg[1, 2, 0], lg[1, S - 2, 1] = float("nan"), float("nan")
    lg[1, 1, 1], lg[1, S - 3 if S > 4 else 1, 0] = float("inf"), float("-inf")
    types = torch.zeros((B, S), dtype=torch.int32)
    lens = torch.full((B,), S, dtype=torch.int32)
    q = (S - 4) // 3                           # question tokens (0 at S = 4: [CLS] [SEP] p [SEP])
    types[:, q + 2:] = 1                       # [CLS] q tokens [SEP] | passage ... [SEP]
    lens[0] = S
    lens[1] = S
    lens[2] = q + 3                            # an empty passage: lo = q + 2 > hi = q + 1
    types[2, q + 3:] = 0
    lens[3], lens[4] = -5, S + 100             # out of range: clamped into [2, S]
    types[5] = 0                               # no type-1 position at all
    types[6] = 1                               # type 1 from position 0
    lens[6] = max(4, S - 1)
    lens[7] = max(4, (3 * S) // 4)
    types[7, int(lens[7]):] = 0
    return lg, types, lens


@pytest.mark.parametrize("S", [4, 7, 24])
def test_span_select_ref_equals_brute_force(S):
    lg, types, lens = span_cases(S)
    B = lg.shape[0]
    for n in (1, 3, 32):  # 32 > the candidate count of the short rows
        for max_len in sorted({1, min(3, S), S}):
            span, score, null = ops.span_select_ref(lg, types, lens, max_len, n)
            assert span.shape == (B, n, 2) and span.dtype == torch.int32 and score.dtype == torch.float32
            for b in range(B):
                want_s, want_v = _brute(lg[b].numpy(), types[b].numpy(), lens[b], max_len, n)
                assert np.array_equal(span[b].numpy(), want_s), (S, n, max_len, b)
                assert np.array_equal(score[b].numpy().view(np.int32), want_v.view(np.int32)), (S, n, max_len, b)
            assert np.array_equal(null.numpy().view(np.int32), (lg[:, 0, 0] + lg[:, 0, 1]).numpy().view(np.int32))
            assert span[2].eq(-1).all() and torch.isinf(score[2]).all()   # the empty passage
            assert span[5].eq(-1).all()                                   # no passage segment
            assert span[3].eq(-1).all()                                   # len clamped to 2: hi = 0 < lo


def test_span_topk_cpu_path_and_checks():
    S, H, B = 8, 64, 3
    g = torch.Generator().manual_seed(3)
    x = torch.randn(B * S, H, generator=g)
    u, c = torch.randn(2, H, generator=g), torch.randn(2, generator=g)
    su = torch.zeros(2)
    types = torch.zeros((B, S), dtype=torch.int32)
    types[:, 3:] = 1
    lens = torch.tensor([8, 6, 5], dtype=torch.int32)
    x[S + 6:2 * S] = float("nan")  # padding rows: never the source of a value
    logits = torch.zeros(B, S, 2)
    span, score, null = ops.span_topk(x, lens, types, B, u, su, c, 4, 5, logits_out=logits)
    want = (x @ u.t() + c).view(B, S, 2)
    for b in range(B):
        torch.testing.assert_close(logits[b, :lens[b]], want[b, :lens[b]])
        assert torch.isinf(logits[b, lens[b]:]).all()
    sp, sc, nl, lg = ops.span_topk_ref(x, lens, types, B, u, su, c, 4, 5)
    assert torch.equal(span, sp) and torch.equal(score, sc) and torch.equal(null, nl) and torch.equal(logits, lg)
    assert torch.isfinite(score[1, 0]) and span[2, 1:].eq(-1).all()  # row 2 has one candidate: (0, 0)
    # given outputs: rows past B are not touched
    out = (torch.full((B + 2, 5, 2), -7, dtype=torch.int32), torch.full((B + 2, 5), -7.0), torch.full((B + 2,), -7.0))
    ops.span_topk(x, lens, types, B, u, su, c, 4, 5, span=out[0], score=out[1], null=out[2])
    assert torch.equal(out[0][:B], sp) and all(o[B:].eq(-7).all() for o in out)
    for kw in (dict(n=0), dict(n=33), dict(n=True), dict(max_len=0), dict(max_len=S + 1), dict(max_len=2.0)):
        args = dict(max_len=4, n=5)
        args.update(kw)
        with pytest.raises(ValueError):
            ops.span_topk(x, lens, types, B, u, su, c, args["max_len"], args["n"])
    with pytest.raises(ValueError):  # H not a multiple of 64
        ops.span_topk(x[:, :40].contiguous(), lens, types, B, u[:, :40].contiguous(), su, c, 4, 5)
    with pytest.raises(ValueError):  # S < 4
        ops.span_topk(x[:9], lens, types[:, :3].contiguous(), B, u, su, c, 1, 1)
    empty = ops.span_topk(x[:0], lens, types, 0, u, su, c, 4, 5)
    assert empty[0].shape == (0, 5, 2) and empty[1].shape == (0, 5) and empty[2].shape == (0,)


# ---------------------------------------------------------------- token_spans
ROWS = ["Hello, world! it's (not) here.", "", "   ", "a" * 30 + " " + "b" * 49 + "!",
        "w" * 101 + " after", "naïve café über straße", "日本語 のテキスト x€y", "tab\there\nnew\x01ctl\x7f",
        "kalo mira ten, kalomira-ten; TEN", "x" * 24 + "€" * 9, "ends with punct ...", "é" * 120 + " tail"]


def _check_spans(row, ids, spans, retok):
    assert len(spans) == len(ids)
    prev = 0
    for (a, b), tid in zip(spans, ids):
        assert prev <= a < b <= len(row), (row, spans)  # increasing, non-overlapping, inside the row
        assert all(T._CLASS[c] != 0 for c in row[a:b]), (row, a, b)  # no separator byte
        prev = b
    for (a, b), tid in zip(spans, ids):
        if a == 0 or T._CLASS[row[a - 1]] != 2 or T._CLASS[row[a]] == 1:  # a word-initial token
            assert retok(row[a:b])[0] == tid, (row, a, b)


@pytest.mark.parametrize("cap", [1, 3, 7, 126])
def test_token_spans_hash(cap):
    extra = [r for r in make_text_rows(10, words_per_row=9, seed=6)]
    for text in ROWS + extra:
        row = text.encode("utf-8")
        ids = T.token_ids(row, 4096, cap)
        spans = T.token_spans(row, 4096, cap)
        _check_spans(row, ids, spans, lambda b: T.token_ids(b, 4096, 8))
        assert all(b - a <= T.PIECE_BYTES for a, b in spans)
    row = ("a" * 30 + " " + "b" * 49 + "!").encode()
    assert T.token_spans(row, 4096, 126) == [(0, 24), (24, 30), (31, 55), (55, 79), (79, 80), (80, 81)]
    assert T.token_spans(row, 4096, 3) == [(0, 24), (24, 30), (31, 55)]  # the cap cuts inside a word


@pytest.mark.parametrize("cap", [1, 3, 7, 126])
def test_token_spans_wordpiece(small, cap):
    _, vocab = small
    extra = [r for r in make_text_rows(10, words_per_row=9, seed=6)]
    saw_unk = saw_pieces = False
    for text in ROWS + extra:
        row = text.encode("utf-8")
        ids = vocab.token_ids(row, cap)
        spans = vocab.token_spans(row, cap)
        _check_spans(row, ids, spans, lambda b: vocab.token_ids(b, 8))
        for k, ((a, b), tid) in enumerate(zip(spans, ids)):
            if tid == vocab.unk_id:  # [UNK] gets the whole word
                saw_unk = True
                assert (a == 0 or T._CLASS[row[a - 1]] != 2) and (b == len(row) or T._CLASS[row[b]] != 2
                                                                  or T._CLASS[row[a]] == 1)
            if k and spans[k - 1][1] == a and T._CLASS[row[a]] == 2 and T._CLASS[row[a - 1]] == 2:
                saw_pieces = True
    assert saw_unk and (saw_pieces or cap == 1)
    row = ("w" * 101 + " after").encode()
    assert vocab.token_ids(row, 9)[0] == vocab.unk_id and vocab.token_spans(row, 9)[0] == (0, 101)


def test_token_spans_equal_hf_offsets(small):
    transformers = pytest.importorskip("transformers")
    path, vocab = small
    try:
        hf = transformers.BertTokenizerFast(path, do_lower_case=True)
    except Exception as exc:  # no fast tokenizer backend here
        pytest.skip(f"BertTokenizerFast not available: {exc}")
    rows = [r for r in ROWS if r.isascii() and r.isprintable()] + make_text_rows(40, words_per_row=12, seed=9)
    rows += ["it's (not) here; a-b_c x.y?", "w" * 101 + " after", "  lead and trail  "]
    for text in rows:
        enc = hf(text, add_special_tokens=False, return_offsets_mapping=True)
        row = text.encode()
        assert vocab.token_ids(row, 512) == enc["input_ids"], text
        assert vocab.token_spans(row, 512) == [tuple(o) for o in enc["offset_mapping"]], text


# ---------------------------------------------- engine: characters of the span
@pytest.fixture()
def cpu_handle(monkeypatch):
    monkeypatch.setenv("CLASSIFY_DEVICE", "cpu")
    from ops._gpu_runtime import get_gpu_handle

    return get_gpu_handle(MODEL)


def test_answer_widens_to_character_boundaries(cpu_handle):
    eng = cpu_handle.engine
    passage = "a" + "€" * 10 + " end"  # 31 word bytes: pieces [0, 24) and [24, 31), the cut inside the 8th '€'
    row = passage.encode()
    assert T.token_spans(row, 4096, 38)[:2] == [(0, 24), (24, 31)] and 0x80 <= row[24] <= 0xBF
    span = torch.tensor([[[1, 1], [0, 0], [0, 2], [-1, -1]]], dtype=torch.int32)
    score = torch.tensor([[3.0, 2.0, 1.0, float("-inf")]])
    res = eng.rank_spans(span, score, torch.tensor([0.5]), [passage], [0, 1], top_k=4)
    a = res.answers[0]
    assert len(a) == 3  # the -inf entry is dropped
    assert (a[0]["start"], a[0]["end"], a[0]["text"]) == (8, 11, "€" * 3)         # starts inside a character
    assert (a[1]["start"], a[1]["end"], a[1]["text"]) == (0, 9, "a" + "€" * 8)    # ends inside a character
    assert (a[2]["start"], a[2]["end"], a[2]["text"]) == (0, 15, passage)
    for e in a:
        assert passage[e["start"]:e["end"]] == e["text"] and e["null_score"] == 0.5 and e["passage"] == 0
    # a row longer than max_row_bytes is tokenized as the device cut it; offsets are those of the full string
    long = "é" * (eng.max_row_bytes // 2 + 40) + " tail"
    res = eng.rank_spans(torch.tensor([[[0, 0]]], dtype=torch.int32), torch.tensor([[1.0]]), torch.tensor([0.0]),
                         [long], [0, 1], top_k=1)
    assert res.answers[0][0]["text"] == "é" * 12 and res.answers[0][0]["start"] == 0


def test_engine_spans_equal_model_on_twin_rows(cpu_handle):
    """More pairs than ``batch_rows`` (chunks of 4), a group across a chunk boundary, empty groups."""
    h, eng = cpu_handle, cpu_handle.engine
    flat = [p for ps in PASSAGES for p in ps]
    goff = [0, 7, 9, 9]
    res = eng.answer_pairs(QUESTIONS, flat, goff, top_k=3, max_answer_tokens=5)
    ids_q, lens_q = T.tokenize_rows([q.encode() for q in QUESTIONS], eng.S, h.cfg.vocab_size)
    ids_p, lens_p = T.tokenize_rows([p.encode() for p in flat], eng.S, h.cfg.vocab_size)
    qidx = np.repeat(np.arange(3), np.diff(goff)).astype(np.int32)
    ids, types, lens = T.pair_rows(ids_q, lens_q, ids_p, lens_p, qidx, T.default_max_query_tokens(eng.S))
    logits = torch.zeros(9, eng.S, 2)
    span, score, null = eng.model.spans(torch.from_numpy(ids), torch.from_numpy(lens), torch.from_numpy(types), 5, 3,
                                        logits_out=logits)
    torch.testing.assert_close(res.score, score, atol=1e-5, rtol=1e-5)
    torch.testing.assert_close(res.null, null, atol=1e-5, rtol=1e-5)
    assert res.span.shape == (9, 3, 2) and (res.span[:, :, 1] - res.span[:, :, 0] < 5).all()
    assert res.span[2].eq(-1).all()  # the empty passage
    assert [len(a) for a in res.answers] == [3, 3, 0]
    for q, row in enumerate(res.answers):
        scores = [e["score"] for e in row]
        assert scores == sorted(scores, reverse=True)
        for e in row:
            p = flat[goff[q] + e["passage"]]
            assert p[e["start"]:e["end"]] == e["text"] and e["text"]
            t0, t1 = e["tokens"]
            toks = T.token_spans(p.encode(), h.cfg.vocab_size, eng.S - 2)
            assert p.encode()[toks[t0][0]:toks[t1][1]].decode() == e["text"]  # ASCII rows: nothing to widen
    for bad in ([0, 7, 9], [1, 7, 9, 9]):
        with pytest.raises(ValueError):
            eng.answer_pairs(QUESTIONS, flat, bad)
    for kw in (dict(top_k=0), dict(top_k=33), dict(max_answer_tokens=0), dict(max_answer_tokens=eng.S - 2)):
        with pytest.raises(ValueError):
            eng.answer_pairs(QUESTIONS, flat, goff, **kw)
    assert eng.memory_bytes() > h.engine.pack.nbytes


# ------------------------------------------------------------- op contract
@pytest.fixture()
def op(monkeypatch):
    monkeypatch.setenv("CLASSIFY_DEVICE", "cpu")
    from ops import get_batch_op, get_op

    return get_op("map_answer"), get_batch_op("map_answer")


QUESTIONS = ["how do gpus multiply matrices", "weather tomorrow", "empty list"]
PASSAGES = [["matrix cores multiply tiles", "a recipe for bread", "", "gpus have many compute units",
             "gpus multiply matrices with matrix cores, naïve café", "rain is likely", "x"],
            ["rain is likely tomorrow", "sunny"], []]


def _close(got, want):
    """Two results of the op on a CPU engine: the same answers, the scores equal up to the last bits (the
    PyTorch reference path is not batch-invariant: a pair's fp32 sums depend on the rows it is batched with)."""
    strip = lambda r: [[{k: v for k, v in e.items() if k not in ("score", "null_score", "probability")} for e in x]  # noqa: E731
                       for x in r["answers"]]
    assert strip(got) == strip(want)
    for key in ("score", "null_score", "probability"):
        flat = lambda r: [e[key] for x in r["answers"] for e in x]  # noqa: E731
        np.testing.assert_allclose(flat(got), flat(want), atol=1e-5, rtol=0)
    assert ("null_scores" in got) == ("null_scores" in want)
    if "null_scores" in got:
        np.testing.assert_allclose(sum(got["null_scores"], []), sum(want["null_scores"], []), atol=1e-5, rtol=0)
    skip = ("elapsed_ms", "pairs_per_sec", "answers", "null_scores")
    assert {k: v for k, v in got.items() if k not in skip} == {k: v for k, v in want.items() if k not in skip}


def test_op_output_both_forms(op):
    run, _ = op
    r = run({"questions": QUESTIONS, "passages": PASSAGES, "model_path": MODEL, "top_k": 4, "return_null_scores": True})
    for key in ("ok", "op", "query_count", "pair_count", "top_k", "max_answer_tokens", "model_path", "elapsed_ms",
                "pairs_per_sec", "answers", "null_scores"):
        assert key in r, key
    assert r["ok"] and r["op"] == "map_answer" and r["query_count"] == 3 and r["pair_count"] == 9 and r["top_k"] == 4
    assert r["max_answer_tokens"] == 30 and "dp_world_size" not in r
    assert [len(x) for x in r["answers"]] == [4, 4, 0] and [len(s) for s in r["null_scores"]] == [7, 2, 0]
    for q, row in enumerate(r["answers"]):
        assert [e["score"] for e in row] == sorted((e["score"] for e in row), reverse=True)
        if row:
            assert abs(math.fsum(e["probability"] for e in row) - 1.0) < 1e-12
        for e in row:
            assert set(e) == {"passage", "start", "end", "text", "score", "null_score", "probability"}
            assert PASSAGES[q][e["passage"]][e["start"]:e["end"]] == e["text"] and e["text"]
            assert e["null_score"] == r["null_scores"][q][e["passage"]]
        ex = [math.exp(e["score"] - row[0]["score"]) for e in row]
        np.testing.assert_allclose([e["probability"] for e in row], [v / math.fsum(ex) for v in ex], rtol=1e-12)
    # the single-question form is the first question alone, and a smaller top_k is a prefix
    one = run({"question": QUESTIONS[0], "passages": PASSAGES[0], "model_path": MODEL, "top_k": 2})
    assert one["query_count"] == 1 and "null_scores" not in one and len(one["answers"][0]) == 2
    for a, b in zip(one["answers"][0], r["answers"][0]):
        assert (a["passage"], a["start"], a["end"], a["text"]) == (b["passage"], b["start"], b["end"], b["text"])
        assert abs(a["score"] - b["score"]) < 1e-5
    none = run({"question": "q", "passages": [], "model_path": MODEL})
    assert none["answers"] == [[]] and none["pair_count"] == 0 and none["top_k"] == 3
    # max_answer_tokens bounds the span; min_score_over_null drops before the softmax
    short = run({"questions": QUESTIONS, "passages": PASSAGES, "model_path": MODEL, "top_k": 8, "max_answer_tokens": 1})
    assert all(" " not in e["text"] for x in short["answers"] for e in x)
    margins = sorted((e["score"] - e["null_score"] for e in r["answers"][0]), reverse=True)
    cut = (margins[1] + margins[2]) / 2 if margins[1] > margins[2] else margins[1]
    m = run({"questions": QUESTIONS, "passages": PASSAGES, "model_path": MODEL, "top_k": 4, "min_score_over_null": cut})
    kept = [e for e in r["answers"][0] if e["score"] - e["null_score"] >= cut]
    assert 0 < len(kept) < 4 and len(m["answers"][0]) == len(kept)
    assert all(e["score"] - e["null_score"] >= cut - 1e-5 for x in m["answers"] for e in x)
    assert abs(math.fsum(e["probability"] for e in m["answers"][0]) - 1.0) < 1e-12
    everything = run({"question": QUESTIONS[0], "passages": PASSAGES[0], "model_path": MODEL,
                      "min_score_over_null": 1e9})
    assert everything["answers"] == [[]]


def test_op_errors(op):
    run, _ = op
    from ops.map_answer import ERRORS

    base = {"question": "q", "passages": ["a", "b"], "model_path": MODEL}
    cases = [({"passages": ["a"]}, "missing"), ({"question": "q"}, "missing"),
             (dict(base, questions=["q"]), "both"), (dict(base, question=5), "question"),
             (dict(base, passages="a"), "passages"), (dict(base, passages=["a", 3]), "passages"),
             ({"questions": "q", "passages": [["a"]]}, "questions"),
             ({"questions": ["q", 2], "passages": [["a"], []]}, "questions"),
             ({"questions": ["q"], "passages": ["a"]}, "passage_lists"),
             ({"questions": ["q", "r"], "passages": [["a"]]}, "passage_lists"),
             (dict(base, top_k=0), "top_k"), (dict(base, top_k=33), "top_k"), (dict(base, top_k="3"), "top_k"),
             (dict(base, top_k=True), "top_k"),
             (dict(base, max_answer_tokens=0), "max_answer_tokens"), (dict(base, max_answer_tokens=38), "max_answer_tokens"),
             (dict(base, max_answer_tokens=2.0), "max_answer_tokens"),
             (dict(base, max_query_tokens=0), "max_query_tokens"), (dict(base, max_query_tokens=37), "max_query_tokens"),
             (dict(base, max_query_tokens=2.0), "max_query_tokens"),
             (dict(base, min_score_over_null="0"), "min_score_over_null"),
             (dict(base, min_score_over_null=float("nan")), "min_score_over_null"),
             (dict(base, min_score_over_null=True), "min_score_over_null"),
             (dict(base, return_null_scores=1), "return_null_scores"),
             (dict(base, model_path="bert-tiny?batch=4&seq=40"), "qa")]
    seen = set()
    for payload, key in cases:
        with pytest.raises(ValueError) as e:
            run(payload)
        assert str(e.value) == ERRORS[key], (payload, key)
        seen.add(key)
    assert seen == set(ERRORS)
    assert run(dict(base, max_query_tokens=36, max_answer_tokens=37))["ok"]  # seq_len - 4, seq_len - 3
    # every message is in the contract
    import os

    import ops.map_answer as ma

    contract = open(os.path.join(os.path.dirname(ma.__file__), "map_answer.CONTRACT.md")).read()
    for msg in ERRORS.values():
        assert msg in contract, msg


def test_model_specs(tmp_path):
    import json

    from safetensors.torch import save_file

    from ops._gpu_runtime import _load_host_pack, parse_spec

    assert parse_spec("bert-tiny").qa is False and parse_spec("bert-tiny?qa=1").qa is True
    assert parse_spec("bert-tiny?qa=1").head is True and parse_spec("bert-tiny?qa=0").qa is False
    qa = config_for("bert-tiny", qa_head=True)
    pack = init_random(qa, seed=4)
    tensors = {n: pack[n].clone() for n in pack.names() if not n.startswith(("pool_", "cls_"))}
    path = str(tmp_path / "reader.safetensors")
    save_file(tensors, path)
    with open(path + ".json", "w") as f:
        json.dump({"preset": "bert-tiny", "head": "qa"}, f)
    spec = parse_spec(path)
    assert spec.qa is True and spec.head is False
    got = _load_host_pack(spec, config_for(spec.preset, num_labels=spec.labels, qa_head=spec.qa))
    assert torch.equal(got["qa_w"], pack["qa_w"]) and not got["pool_w"].any() and not got["cls_w"].any()
    # map_classify / map_rerank refuse it with the error of a headless encoder
    from types import SimpleNamespace

    from ops.map_rerank import ERRORS, check_model, options

    with pytest.raises(ValueError) as e:
        check_model(SimpleNamespace(spec=spec), options({}))
    assert str(e.value) == ERRORS["head"]
    del tensors["qa_w"]
    save_file(tensors, path)
    with pytest.raises(KeyError, match="qa_w"):
        _load_host_pack(spec, qa)


def test_batched_jobs_equal_single_jobs(op):
    run, batch = op
    jobs = [{"questions": QUESTIONS, "passages": PASSAGES, "model_path": MODEL, "top_k": 2, "return_null_scores": True},
            {"question": 7, "passages": []},
            {"question": QUESTIONS[1], "passages": PASSAGES[0], "model_path": MODEL, "top_k": 7,
             "min_score_over_null": -0.3},
            {"question": QUESTIONS[0], "passages": PASSAGES[1], "model_path": MODEL, "max_query_tokens": 2},
            {"question": "q", "passages": [], "model_path": MODEL},
            {"question": QUESTIONS[0], "passages": ["a b c d"], "model_path": MODEL, "max_answer_tokens": 2},
            {"question": QUESTIONS[0], "passages": ["a"], "model_path": MODEL, "max_answer_tokens": 99}]
    res = batch(jobs)
    assert [r[0] for r in res] == ["ok", "err", "ok", "ok", "ok", "ok", "err"]
    assert str(res[1][1]) == "payload.question must be a string" and isinstance(res[6][1], ValueError)
    for job, (kind, got) in zip(jobs, res):
        if kind == "ok":
            _close(got, run(job))
