"""Zero-shot classification on the CPU: the premise twin (``atpu-premise v1``) against HF ``BertTokenizer``
``only_first`` pair encoding and on the edge rows HF has no counterpart for, the CPU references of
``ops.premise_assemble`` and ``ops.nli_rank``, HF ``ZeroShotClassificationPipeline`` parity of ``map_zero_shot``
end to end, and the op contract on a CPU engine, lease batching included."""
import json
import os

import numpy as np
import pytest
import torch

from agent_tpu_amd import ops
from agent_tpu_amd import tokenizer as T
from agent_tpu_amd.utils.synthetic import make_text_rows, make_wordpiece_vocab

MODEL = "bert-tiny?nli=1&batch=4&seq=32&seed=3"


@pytest.fixture(scope="module")
def small(tmp_path_factory):
    path = tmp_path_factory.mktemp("wp") / "vocab.txt"
    with open(path, "wb") as f:
        f.write("\n".join(make_wordpiece_vocab(300, seed=1)).encode("utf-8") + b"\n")
    return str(path), T.WordPieceVocab.load(str(path))


# ------------------------------------------------------------------ the twin
@pytest.mark.parametrize("S", [16, 128])
def test_premise_rows_equal_hf_only_first_encoding(small, S):
    transformers = pytest.importorskip("transformers")
    path, vocab = small
    hf = transformers.BertTokenizer(path, do_lower_case=True)
    mh = T.default_max_query_tokens(S)
    cand = [" ".join(r.split()[:w]) for w in (1, 2, 3, 5) for r in make_text_rows(12, words_per_row=8, seed=S + w)]
    _, lens_c = vocab.tokenize_rows([c.encode() for c in cand], S)
    # only hypotheses the twin tokenizes to <= mh tokens: HF never truncates the second segment
    hyps = [c for c, n in zip(cand, lens_c) if n - 2 <= mh][:12]
    assert len(hyps) >= 6
    texts = ["", "ka"] + make_text_rows(10, words_per_row=6, seed=7) + make_text_rows(6, words_per_row=150, seed=8)
    pairs = [(t, h) for t in range(len(texts)) for h in range(len(hyps))]
    ids_t, lens_t = vocab.tokenize_rows([t.encode() for t in texts], S)
    ids_h, lens_h = vocab.tokenize_rows([h.encode() for h in hyps], S)
    tidx = np.asarray([t for t, _ in pairs], dtype=np.int32)
    hidx = np.asarray([h for _, h in pairs], dtype=np.int32)
    ids, types, lens = T.premise_rows(ids_t, lens_t, ids_h, lens_h, tidx, hidx, mh, vocab.cls_id, vocab.sep_id,
                                      vocab.pad_id)
    enc = hf([texts[t] for t, _ in pairs], [hyps[h] for _, h in pairs], truncation="only_first", max_length=S,
             padding="max_length")
    np.testing.assert_array_equal(ids, np.asarray(enc["input_ids"], dtype=np.int32))
    np.testing.assert_array_equal(types, np.asarray(enc["token_type_ids"], dtype=np.int32))
    np.testing.assert_array_equal(lens, np.asarray(enc["attention_mask"], dtype=np.int32).sum(1))
    assert (lens == S).any() and (lens < S).any()  # an overflowing text and a short one
    overflow = (lens_t[tidx] - 2) > (S - 3 - (lens_h[hidx] - 2))
    assert overflow.any() and (~overflow).any()  # both kinds of text occurred
    assert (lens[overflow] == S).all()


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


def test_premise_rows_edge_cases():
    S = 8
    ids_t, lens_t = _rows(S, [3, 0, 6])              # texts 1000.., 1100.. (empty), 1200..
    ids_h, lens_h = _rows(S, [2, 0, 6, 1], 2000)     # hypotheses 2000.., (empty), 2200.., 2300
    i32 = lambda *v: np.asarray(v, np.int32)  # noqa: E731
    ids, types, lens = T.premise_rows(ids_t, lens_t, ids_h, lens_h, i32(2, 1, 0, 0), i32(0, 0, 1, 2), 2)
    # a text longer than its room: cut to what the hypothesis leaves
    assert ids[0].tolist() == [101, 1200, 1201, 1202, 102, 2000, 2001, 102] and lens[0] == 8
    assert types[0].tolist() == [0, 0, 0, 0, 0, 1, 1, 1]
    # an empty text
    assert ids[1].tolist() == [101, 102, 2000, 2001, 102, 0, 0, 0] and types[1].tolist() == [0, 0, 1, 1, 1, 0, 0, 0]
    # an empty hypothesis
    assert ids[2].tolist() == [101, 1000, 1001, 1002, 102, 102, 0, 0] and types[2].tolist() == [0, 0, 0, 0, 0, 1, 0, 0]
    # a hypothesis longer than mh: cut to mh tokens (HF has no such cut)
    assert ids[3].tolist() == [101, 1000, 1001, 1002, 102, 2200, 2201, 102] and types[3].tolist() == [0, 0, 0, 0, 0, 1, 1, 1]
    assert lens.tolist() == [8, 5, 6, 8]
    # mh = 0: no hypothesis tokens
    ids, types, lens = T.premise_rows(ids_t, lens_t, ids_h, lens_h, i32(0, 2), i32(0, 2), 0)
    assert ids[0].tolist() == [101, 1000, 1001, 1002, 102, 102, 0, 0] and types[0].tolist() == [0, 0, 0, 0, 0, 1, 0, 0]
    assert ids[1].tolist() == [101, 1200, 1201, 1202, 1203, 1204, 102, 102] and types[1].tolist() == [0] * 7 + [1]
    assert lens.tolist() == [6, 8]
    # mh >= S: the hypothesis keeps at most S - 3 tokens, so both [SEP] always fit
    ids, types, lens = T.premise_rows(ids_t, lens_t, ids_h, lens_h, i32(0, 1), i32(2, 3), S + 5)
    assert ids[0].tolist() == [101, 102, 2200, 2201, 2202, 2203, 2204, 102] and lens[0] == 8
    assert types[0].tolist() == [0, 0, 1, 1, 1, 1, 1, 1]
    assert ids[1].tolist() == [101, 102, 2300, 102, 0, 0, 0, 0] and types[1].tolist() == [0, 0, 1, 1, 0, 0, 0, 0]
    # lens out of range are clamped into [2, S]; tidx / hidx out of range into [0, T) / [0, Hn)
    bad_t, bad_h = i32(-4, 1, 99), i32(99, -1, 0, 3)
    got = T.premise_rows(ids_t, bad_t, ids_h, bad_h, i32(-1, 7, 0, 2), i32(9, -2, 3, 1), 3)
    want = T.premise_rows(ids_t, i32(2, 2, S), ids_h, i32(S, 2, 2, 3), i32(0, 2, 0, 2), i32(3, 0, 3, 1), 3)
    for a, b in zip(got, want):
        np.testing.assert_array_equal(a, b)
    assert got[2].tolist() == [4, 8, 4, 8]
    with pytest.raises(ValueError):
        T.premise_rows(ids_t[:, :3], lens_t, ids_h[:, :3], lens_h, i32(0), i32(0), 2)  # S < 4
    with pytest.raises(ValueError):
        T.premise_rows(ids_t, lens_t, ids_h, lens_h, i32(0), i32(0), -1)
    with pytest.raises(ValueError):
        T.premise_rows(ids_t, lens_t, ids_h, lens_h, i32(0, 1), i32(0), 2)


def test_premise_assemble_cpu_ref_equals_twin(small):
    _, vocab = small
    S = 16
    rows = [r.encode() for r in make_text_rows(9, words_per_row=5, seed=2)] + [b""]
    tidx = np.asarray([0, 0, 2, 1, 9, -3, 1, 2, 0, 12], dtype=np.int32)
    hidx = np.asarray([0, 1, 2, 0, 1, 2, 5, -1, 0, 1], dtype=np.int32)
    ids_t, lens_t = vocab.tokenize_rows(rows, S)
    ids_h, lens_h = vocab.tokenize_rows(rows[:3], S)
    sp = (vocab.cls_id, vocab.sep_id, vocab.pad_id)
    want = T.premise_rows(ids_t, lens_t, ids_h, lens_h, tidx, hidx, 4, *sp)
    t = [torch.from_numpy(a) for a in (ids_t, lens_t, ids_h, lens_h, tidx, hidx)]
    got = ops.premise_assemble(*t, 4, *sp)
    for a, b in zip(got, want):
        assert a.dtype == torch.int32 and np.array_equal(a.numpy(), b)
    assert got[0][0, 0] == sp[0] and (got[0] == sp[1]).sum(1).eq(2).all()
    # preallocated outputs, the first `rows` rows only: the rest is not touched
    out = [torch.full((12, S), -7, dtype=torch.int32), torch.full((12, S), -7, dtype=torch.int32),
           torch.full((12,), -7, dtype=torch.int32)]
    ops.premise_assemble(*t, 4, *sp, ids=out[0], type_ids=out[1], lens=out[2], rows=7)
    for a, b in zip(out, want):
        assert np.array_equal(a[:7].numpy(), b[:7]) and (a[7:] == -7).all()
    with pytest.raises(ValueError):
        ops.premise_assemble(t[0].long(), *t[1:], 4)
    with pytest.raises(ValueError):
        ops.premise_assemble(*t, -1)
    with pytest.raises(ValueError):
        ops.premise_assemble(*t, 4, rows=11)  # more rows than tidx / hidx name
    with pytest.raises(ValueError):
        ops.premise_assemble(*t, 4, ids=out[0])


# ----------------------------------------------------------------- nli_rank
def _hf_postprocess(logits, ent, con, multi):
    """``ZeroShotClassificationPipeline.postprocess`` on one sequence's ``[labels, C]`` logits, in fp64."""
    logits = np.asarray(logits, dtype=np.float64)
    if multi or logits.shape[0] == 1:
        ec = logits[:, [con, ent]]
        scores = (np.exp(ec) / np.exp(ec).sum(-1, keepdims=True))[:, 1]
    else:
        e = logits[:, ent]
        scores = np.exp(e) / np.exp(e).sum()
    return scores


@pytest.mark.parametrize("multi", [False, True])
def test_nli_rank_ref_is_hf_postprocess(multi):
    g = torch.Generator().manual_seed(5 + multi)
    lens = [0, 1, 2, 9, 300, 0, 5]
    goff = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    P = int(goff[-1])
    pair = torch.randn(P, 2, generator=g) * 3
    order, score = ops.nli_rank(pair, torch.from_numpy(goff), multi)
    assert order.dtype == torch.int32 and score.dtype == torch.float32 and order.shape == score.shape == (P,)
    for t, n in enumerate(lens):
        a, b = int(goff[t]), int(goff[t + 1])
        # column 0 is the entailment logit, column 1 the contradiction logit
        want = _hf_postprocess(pair[a:b].numpy(), 0, 1, multi) if n else np.zeros(0)
        by_label = np.zeros(n)
        by_label[order[a:b].numpy()] = score[a:b].numpy()
        np.testing.assert_allclose(by_label, want, atol=1e-6, rtol=1e-6)
        assert sorted(order[a:b].tolist()) == list(range(n))
        assert (np.diff(score[a:b].numpy()) <= 0).all()  # ranked: the score is monotone in the key
    # a group of one in single-label mode takes the multi-label formula (HF's rule)
    one = torch.tensor([[0.3, 1.1]])
    o, s = ops.nli_rank(one, torch.tensor([0, 1], dtype=torch.int32), False)
    assert o.tolist() == [0] and abs(s.item() - 1 / (1 + np.exp(0.8))) < 1e-7 and s.item() != 1.0


def test_nli_rank_ref_ties_nan_and_inf():
    i32 = lambda *v: torch.tensor(v, dtype=torch.int32)  # noqa: E731
    nan, inf = float("nan"), float("inf")
    # ties rank by index; +0.0 and -0.0 tie
    pair = torch.tensor([[0.0, 9.0], [-0.0, 1.0], [-1.0, 0.0], [-0.0, 2.0], [0.0, 0.0], [2.5, 0.0], [2.5, 7.0]])
    o, s = ops.nli_rank(pair, i32(0, 7), False)
    assert o.tolist() == [5, 6, 0, 1, 3, 4, 2] and s[0] == s[1] and s[2] == s[3] == s[4] == s[5]
    o, _ = ops.nli_rank(torch.tensor([[1.0, 1.0], [-2.0, -2.0], [0.0, -0.0], [3.0, 4.0]]), i32(0, 4), True)
    assert o.tolist() == [0, 1, 2, 3]  # keys 0.0, 0.0, 0.0, -1.0
    # a NaN logit, in either column, ranks as -inf and scores 0, in both modes
    pair = torch.tensor([[1.0, 0.0], [nan, 0.0], [2.0, nan], [-inf, 0.0], [0.5, 0.0]])
    for multi in (False, True):
        o, s = ops.nli_rank(pair, i32(0, 5), multi)
        assert o.tolist() == [0, 4, 1, 2, 3] and s[2:].eq(0).all() and (s[:2] > 0).all() and torch.isfinite(s).all()
    o, s = ops.nli_rank(pair, i32(0, 5), False)
    assert abs(s[:2].sum().item() - 1.0) < 1e-6
    # +inf: in mode 0 the +inf keys share the mass; in mode 1 inf - inf is a NaN, so -inf
    pair = torch.tensor([[-inf, 0.0], [inf, 0.0], [inf, inf], [0.0, inf]])
    o, s = ops.nli_rank(pair, i32(0, 4), False)
    assert o.tolist() == [1, 2, 3, 0] and s.tolist() == [0.5, 0.5, 0.0, 0.0]
    o, s = ops.nli_rank(pair, i32(0, 4), True)
    assert o.tolist() == [1, 0, 2, 3] and s.tolist() == [1.0, 0.0, 0.0, 0.0]
    # a group whose best key is -inf scores 0 throughout
    o, s = ops.nli_rank(torch.tensor([[nan, 0.0], [-inf, 1.0], [3.0, nan]]), i32(0, 3), False)
    assert o.tolist() == [0, 1, 2] and s.eq(0).all()
    # offsets are clamped into [0, P], a decreasing pair is an empty group, uncovered positions hold (-1, 0)
    pair = torch.tensor([[1.0, 0.0], [2.0, 0.0], [0.0, 0.0], [5.0, 0.0], [4.0, 0.0]])
    o, s = ops.nli_rank(pair, i32(-4, 2, 99, 3), False)
    assert o.tolist() == [1, 0, 1, 2, 0]
    o, s = ops.nli_rank(pair, i32(1, 3, 1), False)
    assert o.tolist() == [-1, 0, 1, -1, -1] and s[0] == 0 and s[3:].eq(0).all()
    for bad in ((pair.double(), i32(0, 5), False), (pair[:, 0], i32(0, 5), False), (pair, i32(0, 5).long(), False),
                (pair, i32(0, 5), 1)):
        with pytest.raises(ValueError):
            ops.nli_rank(*bad)


# ----------------------------------------------------- HF parity, end to end
ATOL, RTOL = 2e-4, 1e-4  # test_rerank_cpu.py: the fp32 oracle against HF


def test_map_zero_shot_matches_hf_pipeline(small, tmp_path, monkeypatch):
    transformers = pytest.importorskip("transformers")
    from safetensors.torch import save_file

    from agent_tpu_amd.models.bert import BertClassifier, config_for, from_hf_state_dict

    monkeypatch.setenv("CLASSIFY_DEVICE", "cpu")
    vocab_path, vocab = small
    names = ["entailment", "neutral", "contradiction"]  # entailment id 0: HF's contradiction id is then the last
    hcfg = transformers.BertConfig(vocab_size=4096, hidden_size=256, num_hidden_layers=2, num_attention_heads=4,
                                   intermediate_size=1024, max_position_embeddings=512, type_vocab_size=2,
                                   num_labels=3, hidden_act="gelu", layer_norm_eps=1e-12,
                                   attn_implementation="eager", id2label=dict(enumerate(names)),
                                   label2id={n: i for i, n in enumerate(names)})
    torch.manual_seed(11)
    hf = transformers.BertForSequenceClassification(hcfg).eval()
    with torch.no_grad():
        # HF's default init gives flat scores (0.2 for five labels single-label, 0.5007 multi-label): the scaled
        # classifier spreads them. Scaling alone moves every entailment - contradiction difference off zero
        # by the same amount (the pooled state's common part), which flattens the sigmoid again, so the
        # contradiction bias below takes that common part out
        hf.classifier.weight.mul_(300.0)
        for p in hf.parameters():  # our pack stores bf16 weights: give HF the same values
            p.copy_(p.bfloat16().float())
    S = 32
    words = [w.lower() for r in make_text_rows(1, words_per_row=12, seed=21) for w in r.split()]
    labels = list(dict.fromkeys(words))[:5]
    template = f"{words[-1]} {words[-2]} {{}}"
    texts = make_text_rows(4, words_per_row=7, seed=22) + make_text_rows(2, words_per_row=60, seed=23) + ["ka"]
    tok = transformers.BertTokenizer(vocab_path, do_lower_case=True, model_max_length=S)
    pipe = transformers.ZeroShotClassificationPipeline(model=hf, tokenizer=tok)
    assert pipe.entailment_id == 0
    flat = np.asarray([s for r in pipe(texts, candidate_labels=labels, hypothesis_template=template, multi_label=True)
                       for s in r["scores"]], dtype=np.float64)
    with torch.no_grad():
        hf.classifier.bias[2] = torch.tensor(float(np.log(flat / (1 - flat)).mean())).bfloat16().float()
    cfg = config_for("bert-tiny", num_labels=3)
    pack = from_hf_state_dict(cfg, hf.state_dict())
    path = str(tmp_path / "nli.safetensors")
    save_file({n: pack[n].clone() for n in pack.names()}, path)
    with open(path + ".json", "w") as f:
        json.dump({"preset": "bert-tiny", "num_labels": 3, "vocab": vocab_path, "nli_labels": names}, f)
    model = path + f"?batch=4&seq={S}"
    from ops import get_op
    from ops._gpu_runtime import get_gpu_handle

    # the CPU engine's model is the bf16 reference path; the parity bound is the fp32 oracle's, so the engine
    # of this file's handle gets the oracle on the weights it loaded
    h = get_gpu_handle(model)
    assert h.spec.nli == (0, 2) and h.engine.vocab is not None
    h.engine.model = BertClassifier(h.cfg, h.engine.pack, fp32=True)
    run = get_op("map_zero_shot")
    for multi in (False, True):
        want = pipe(texts, candidate_labels=labels, hypothesis_template=template, multi_label=multi)
        got = run({"texts": texts, "candidate_labels": labels, "hypothesis_template": template, "multi_label": multi,
                   "model_path": model})
        assert got["entailment_id"] == 0 and got["contradiction_id"] == 2 and got["pair_count"] == 35
        clear = total = 0
        for w, g in zip(want, got["results"]):
            ws = np.asarray(w["scores"], dtype=np.float64)
            by_label = dict(zip(g["labels"], g["scores"]))
            np.testing.assert_allclose([by_label[name] for name in w["labels"]], ws, atol=ATOL, rtol=RTOL)
            # HF's order is binding only where its neighbouring scores are more than twice the tolerance apart
            gap = np.abs(np.diff(ws)) > 2 * ATOL
            ok = np.concatenate([[True], gap]) & np.concatenate([gap, [True]])
            clear += int(ok.sum())
            total += len(ws)
            assert [n for n, c in zip(g["labels"], ok) if c] == [n for n, c in zip(w["labels"], ok) if c]
        assert clear >= 0.75 * total, (multi, clear, total)  # else the order check compares nothing


# ------------------------------------------------------------- op contract
@pytest.fixture()
def op(monkeypatch):
    monkeypatch.setenv("CLASSIFY_DEVICE", "cpu")
    from ops import get_batch_op, get_op

    return get_op("map_zero_shot"), get_batch_op("map_zero_shot")


TEXTS = ["how do gpus multiply matrices", "rain is likely tomorrow", "", "a recipe for bread " * 12]
LABELS = ["technology", "weather", "cooking", "sports", "x"]


def _close(got, want):
    """Two results of the op on a CPU engine: the same ranking, the scores equal up to the last bits (the
    PyTorch reference path is not batch-invariant: a pair's fp32 sums depend on the rows it is batched with)."""
    assert [x["labels"] for x in got["results"]] == [x["labels"] for x in want["results"]]
    np.testing.assert_allclose([s for x in got["results"] for s in x["scores"]],
                               [s for x in want["results"] for s in x["scores"]], atol=1e-5, rtol=0)
    skip = ("elapsed_ms", "pairs_per_sec", "results")
    assert {k: v for k, v in got.items() if k not in skip} == {k: v for k, v in want.items() if k not in skip}


def test_op_output_both_forms_and_top_k(op):
    run, _ = op
    r = run({"texts": TEXTS, "candidate_labels": LABELS, "model_path": MODEL})
    for key in ("ok", "op", "model_path", "row_count", "label_count", "pair_count", "multi_label", "hypothesis_template",
                "entailment_id", "contradiction_id", "elapsed_ms", "pairs_per_sec", "results"):
        assert key in r, key
    assert r["ok"] and r["op"] == "map_zero_shot" and r["row_count"] == 4 and r["label_count"] == 5
    assert r["pair_count"] == 20 and r["multi_label"] is False and r["hypothesis_template"] == "This example is {}."
    assert (r["entailment_id"], r["contradiction_id"]) == (2, 0) and "dp_world_size" not in r  # ?nli=1: the MNLI order
    json.dumps(r)
    for x in r["results"]:
        assert set(x) == {"labels", "scores"} and sorted(x["labels"]) == sorted(LABELS)
        assert x["scores"] == sorted(x["scores"], reverse=True) and abs(sum(x["scores"]) - 1.0) < 1e-5
    # the single-text form is that text alone; top_k cuts the ranked list and not the softmax
    one = run({"text": TEXTS[1], "candidate_labels": LABELS, "model_path": MODEL, "top_k": 2})
    assert one["row_count"] == 1 and [len(x["labels"]) for x in one["results"]] == [2]
    want = dict(r, row_count=1, pair_count=5,
                results=[{"labels": r["results"][1]["labels"][:2], "scores": r["results"][1]["scores"][:2]}])
    _close(one, want)
    assert run({"text": "a", "candidate_labels": LABELS, "model_path": MODEL, "top_k": 99})["results"][0]["labels"]
    # multi-label: every label on its own, entailment against contradiction
    m = run({"texts": TEXTS, "candidate_labels": LABELS, "model_path": MODEL, "multi_label": True})
    assert m["multi_label"] is True
    for x in m["results"]:
        assert all(0.0 < s < 1.0 for s in x["scores"]) and x["scores"] == sorted(x["scores"], reverse=True)
    # one label: the multi-label formula in either mode (HF's rule)
    a = run({"text": TEXTS[0], "candidate_labels": ["weather"], "model_path": MODEL})
    b = run({"text": TEXTS[0], "candidate_labels": ["weather"], "model_path": MODEL, "multi_label": True})
    assert a["results"] == b["results"] and 0.0 < a["results"][0]["scores"][0] < 1.0
    # texts: [] gives results: []
    none = run({"texts": [], "candidate_labels": LABELS, "model_path": MODEL})
    assert none["results"] == [] and none["row_count"] == 0 and none["pair_count"] == 0
    # the template, the hypothesis budget and the label ids are part of the result
    t = run({"texts": TEXTS, "candidate_labels": LABELS, "model_path": MODEL, "hypothesis_template": "about {} it is"})
    assert t["hypothesis_template"] == "about {} it is" and t["results"] != r["results"]
    h1 = run({"texts": TEXTS, "candidate_labels": LABELS, "model_path": MODEL, "max_hypothesis_tokens": 1})
    assert h1["results"] != r["results"]
    sw = run({"texts": TEXTS, "candidate_labels": LABELS, "model_path": MODEL, "entailment_id": 0, "contradiction_id": 2})
    assert (sw["entailment_id"], sw["contradiction_id"]) == (0, 2) and sw["results"] != r["results"]
    # without ?nli=1 and without ids: (num_labels - 1, 0)
    d = run({"text": "a", "candidate_labels": LABELS, "model_path": "bert-tiny?labels=4&batch=4&seq=32"})
    assert (d["entailment_id"], d["contradiction_id"]) == (3, 0)


def test_op_errors(op):
    run, _ = op
    from ops.map_zero_shot import ERRORS

    base = {"text": "a b", "candidate_labels": ["x", "y"], "model_path": MODEL}
    cases = [({"candidate_labels": ["x"]}, "missing"), (dict(base, texts=["a"]), "both"), (dict(base, text=5), "text"),
             ({"texts": "a", "candidate_labels": ["x"]}, "texts"), ({"texts": ["a", 3], "candidate_labels": ["x"]}, "texts"),
             ({"text": "a"}, "candidate_labels"), (dict(base, candidate_labels=[]), "candidate_labels"),
             (dict(base, candidate_labels="x"), "candidate_labels"), (dict(base, candidate_labels=["x", ""]), "candidate_labels"),
             (dict(base, candidate_labels=["x", 3]), "candidate_labels"),
             (dict(base, candidate_labels=["x"] * 257), "candidate_labels"),
             (dict(base, hypothesis_template="no slot"), "hypothesis_template"),
             (dict(base, hypothesis_template="{} and {}"), "hypothesis_template"),
             (dict(base, hypothesis_template=3), "hypothesis_template"),
             (dict(base, multi_label=1), "multi_label"), (dict(base, multi_label="yes"), "multi_label"),
             (dict(base, top_k=0), "top_k"), (dict(base, top_k="3"), "top_k"), (dict(base, top_k=True), "top_k"),
             (dict(base, max_hypothesis_tokens=0), "max_hypothesis_tokens"),
             (dict(base, max_hypothesis_tokens=29), "max_hypothesis_tokens"),
             (dict(base, max_hypothesis_tokens=2.0), "max_hypothesis_tokens"),
             (dict(base, entailment_id=-1), "label_ids"), (dict(base, entailment_id=3), "label_ids"),
             (dict(base, contradiction_id="0"), "label_ids"), (dict(base, entailment_id=1, contradiction_id=1), "label_ids"),
             (dict(base, contradiction_id=2), "label_ids"),  # the model's entailment id is 2
             (dict(base, model_path="bert-tiny?labels=1&batch=4&seq=32"), "labels")]
    seen = set()
    for payload, key in cases:
        with pytest.raises(ValueError) as e:
            run(payload)
        assert str(e.value) == ERRORS[key], (payload, key)
        seen.add(key)
    assert seen == set(ERRORS) - {"head"}
    # an encoder without pooler and classifier ("head": "none" in the model json) cannot score
    from types import SimpleNamespace

    from ops.map_zero_shot import check_model, options

    with pytest.raises(ValueError) as e:
        check_model(SimpleNamespace(spec=SimpleNamespace(head=False)), options(base))
    assert str(e.value) == ERRORS["head"]
    assert run(dict(base, max_hypothesis_tokens=28))["ok"]  # seq_len - 4
    assert run(dict(base, candidate_labels=["x"] * 256, top_k=1))["label_count"] == 256
    import ops.map_zero_shot as mz

    contract = open(os.path.join(os.path.dirname(mz.__file__), "map_zero_shot.CONTRACT.md")).read()
    for msg in ERRORS.values():
        assert msg in contract, msg
    for section in ("## Purpose", "## Inputs (payload)", "## Outputs", "## Notes"):
        assert section in contract


def test_model_specs(tmp_path):
    from ops._gpu_runtime import nli_ids_of, parse_spec

    assert parse_spec("bert-tiny").nli is None and parse_spec("bert-tiny").labels == 2
    spec = parse_spec("bert-tiny?nli=1")
    assert spec.nli == (2, 0) and spec.labels == 3 and spec.head is True
    assert parse_spec("bert-tiny?nli=1&labels=5").labels == 5
    assert nli_ids_of(["contradiction", "neutral", "ENTAILMENT"], 3, "x") == (2, 0)
    assert nli_ids_of(["Entails", "not"], 2, "x") == (0, 1)  # HF: the last label when entailment is label 0
    assert nli_ids_of(["a", "entailment", "entail2"], 3, "x") == (1, 0)  # the first match
    for bad in (["a", "b"], ["entailment"], "entailment", ["entailment", 3]):
        with pytest.raises(ValueError):
            nli_ids_of(bad, 2, "x")
    path = str(tmp_path / "nli.safetensors")
    open(path, "wb").close()
    with open(path + ".json", "w") as f:
        json.dump({"preset": "bert-tiny", "num_labels": 3, "nli_labels": ["entailment", "neutral", "contradiction"]}, f)
    assert parse_spec(path).nli == (0, 2) and parse_spec(path).labels == 3
    with open(path + ".json", "w") as f:
        json.dump({"preset": "bert-tiny", "num_labels": 3, "nli_labels": ["entailment", "neutral"]}, f)
    with pytest.raises(ValueError, match="nli_labels"):
        parse_spec(path)
    with open(path + ".json", "w") as f:
        json.dump({"preset": "bert-tiny", "num_labels": 3}, f)
    assert parse_spec(path).nli is None


def test_batched_jobs_equal_single_jobs(op):
    run, batch = op
    jobs = [{"texts": TEXTS, "candidate_labels": LABELS, "model_path": MODEL, "top_k": 3},
            {"text": 7, "candidate_labels": LABELS},
            {"text": TEXTS[1], "candidate_labels": ["weather", "cooking"], "model_path": MODEL,
             "hypothesis_template": "it is about {}"},                          # another label set and template
            {"texts": TEXTS[:2], "candidate_labels": LABELS, "model_path": MODEL, "multi_label": True},  # another group
            {"texts": [], "candidate_labels": LABELS, "model_path": MODEL},
            {"text": TEXTS[0], "candidate_labels": ["x"], "model_path": MODEL},   # one label: the multi-label formula
            {"text": TEXTS[0], "candidate_labels": LABELS, "model_path": MODEL, "entailment_id": 7},
            {"text": TEXTS[0], "candidate_labels": [], "model_path": MODEL}]
    res = batch(jobs)
    assert [r[0] for r in res] == ["ok", "err", "ok", "ok", "ok", "ok", "err", "err"]
    assert str(res[1][1]) == "payload.text must be a string" and isinstance(res[6][1], ValueError)
    for job, (kind, got) in zip(jobs, res):
        if kind == "ok":
            _close(got, run(job))


def test_engine_chunks_and_shared_texts(op):
    """More pairs than ``batch_rows`` (chunks of 4), a text's labels across a chunk boundary, texts without
    labels: the engine's logits are the model's on the twin's rows."""
    from ops._gpu_runtime import get_gpu_handle

    h = get_gpu_handle(MODEL)
    eng = h.engine
    hyps = ["This example is %s." % name for name in LABELS]
    ranges = [(0, 5), (2, 2), (1, 4), (0, 0)]
    res = eng.zero_shot(TEXTS, hyps, ranges, ent=2, con=0)
    assert res.goff == [0, 5, 5, 8, 8] and res.logits.shape == (8, 2)
    ids_t, lens_t = T.tokenize_rows([t.encode() for t in TEXTS], eng.S, h.cfg.vocab_size)
    ids_h, lens_h = T.tokenize_rows([x.encode() for x in hyps], eng.S, h.cfg.vocab_size)
    tidx = np.asarray([0] * 5 + [2] * 3, np.int32)
    hidx = np.asarray([0, 1, 2, 3, 4, 1, 2, 3], np.int32)
    ids, types, lens = T.premise_rows(ids_t, lens_t, ids_h, lens_h, tidx, hidx, T.default_max_query_tokens(eng.S))
    want = eng.model.nli_logits(torch.from_numpy(ids), torch.from_numpy(lens), torch.from_numpy(types), 2, 0)
    torch.testing.assert_close(res.logits, want, atol=1e-5, rtol=1e-5)
    order, score = ops.nli_rank_ref(res.logits, torch.tensor(res.goff, dtype=torch.int32), False)
    assert torch.equal(res.order, order) and torch.equal(res.score, score)
    assert res.ranked(1) == ([], []) and sorted(res.ranked(2)[0]) == [0, 1, 2]
    for bad in ([(0, 5)], [(0, 6), (0, 0), (0, 0), (0, 0)], [(3, 2), (0, 0), (0, 0), (0, 0)]):
        with pytest.raises(ValueError):
            eng.zero_shot(TEXTS, hyps, bad)
    with pytest.raises(ValueError):
        eng.zero_shot(TEXTS, hyps, ranges, ent=1, con=1)
