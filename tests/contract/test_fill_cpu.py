"""Masked-token prediction on the CPU: the ``fill_rows`` twin against a plain-Python construction, the pack
layout with the MLM head, HF parity of the fp32 oracle, the reference ``vocab_topk`` (order, edges, ``lse_in``),
the engine on the twin's rows, and the ``map_fill`` op contract."""
import hashlib
import json
import math
import os

import numpy as np
import pytest
import torch

from agent_tpu_amd import ops
from agent_tpu_amd import tokenizer as T
from agent_tpu_amd.models.bert import (BertClassifier, BertConfig, config_for, from_hf_state_dict, init_random,
                                       param_specs)
from agent_tpu_amd.utils.synthetic import make_text_rows, make_wordpiece_vocab

MODEL = "bert-tiny?mlm=1&batch=4&seq=40&seed=3"
NINF = float("-inf")

#: sha256 of init_random(bert-tiny, num_labels=3, seed=0) computed on the commit before the span, tag and MLM heads
PLAIN_PACK_SHA256 = "f885b05bb79819e9e2fc35127de95f51241096c01aa11b1a62b71d8f4aa3e714"


@pytest.fixture(scope="module")
def small(tmp_path_factory):
    d = tmp_path_factory.mktemp("wp")
    with open(d / "vocab.txt", "wb") as f:
        f.write("\n".join(make_wordpiece_vocab(300, seed=1)).encode("utf-8") + b"\n")
    with open(d / "nomask.txt", "wb") as f:  # the same ids, the [MASK] entry renamed
        f.write("\n".join("[unused]" if e == "[MASK]" else e for e in make_wordpiece_vocab(300, seed=1)).encode()
                + b"\n")
    return str(d / "vocab.txt"), T.WordPieceVocab.load(str(d / "vocab.txt")), str(d / "nomask.txt")


# ------------------------------------------------------------------ fill_rows
def _texts(S):
    """No mask; a mask first and last; adjacent masks (empty pieces); a mask landing exactly at position S - 2
    (kept) and at S - 1 (cut: a '.' is one token for both tokenizers); 16 masks; an empty text; a lone mask."""
    return ["plain words, no mask", "[MASK] middle words [MASK]", "a [MASK][MASK] b", ". " * (S - 3) + "[MASK]",
            ". " * (S - 2) + "[MASK] tail", " ".join(["x [MASK]"] * 16), "", "[MASK]"]


@pytest.mark.parametrize("tokenizer", ["hash", "wordpiece"])
@pytest.mark.parametrize("S", [3, 4, 8, 128])
def test_fill_rows_equal_a_plain_construction(small, S, tokenizer):
    vocab = small[1] if tokenizer == "wordpiece" else None
    cls, sep, pad, mask = ((vocab.cls_id, vocab.sep_id, vocab.pad_id, vocab.mask_id) if vocab
                           else (T.CLS_ID, T.SEP_ID, T.PAD_ID, T.MASK_ID))
    assert mask == (vocab.entries.index(b"[MASK]") if vocab else 103)
    toks = (lambda b, cap: vocab.token_ids(b, cap)) if vocab else (lambda b, cap: T.token_ids(b, 4096, cap))
    texts = _texts(S)
    pieces, segoff = [], [0]
    for t in texts:
        ps, spans = T.split_masks(t)
        assert len(ps) == len(spans) + 1 and all(t[a:b] == "[MASK]" for a, b in spans)
        assert "[MASK]".join(ps) == t
        pieces += ps
        segoff.append(len(pieces))
    rows = [p.encode() for p in pieces]
    ids_s, lens_s = vocab.tokenize_rows(rows, S) if vocab else T.tokenize_rows(rows, S, 4096)
    ids, lens, pos = T.fill_rows(ids_s, lens_s, np.array(segoff, dtype=np.int32), 16, cls, sep, pad, mask)
    assert ids.dtype == lens.dtype == pos.dtype == np.int32 and pos.shape == (len(texts), 16)
    for b, t in enumerate(texts):  # the plain construction: tokenize the pieces, join with the mask id, cut
        c, where = [], []
        for i, p in enumerate(T.split_masks(t)[0]):
            if i:
                where.append(len(c))
                c.append(mask)
            c += toks(p.encode(), S - 2)
        kept = c[:S - 2]
        want = [cls] + kept + [sep] + [pad] * (S - 2 - len(kept))
        assert ids[b].tolist() == want and lens[b] == len(kept) + 2, (S, b)
        want_pos = [w + 1 if w < S - 2 else -1 for w in where] + [-1] * (16 - len(where))
        assert pos[b].tolist() == want_pos, (S, b)
        for p in pos[b]:
            assert p < 0 or ids[b, p] == mask
    assert pos[3, 0] == S - 2 and pos[4, 0] == -1 and (pos[0] == -1).all() and pos[7, 0] == 1
    assert (pos[5] >= 0).sum() == min(16, (S - 2) // 2)
    # the CPU path of the op is the twin; device data is clamped, not trusted
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a))  # noqa: E731
    got = ops.fill_assemble(t(ids_s), t(lens_s), t(np.array(segoff, dtype=np.int32)), 16, cls, sep, pad, mask)
    assert torch.equal(got[0], t(ids)) and torch.equal(got[1], t(lens)) and torch.equal(got[2], t(pos))
    bad_off = np.array(segoff, dtype=np.int32)
    bad_off[2], bad_off[5] = -9, 2 ** 31 - 1
    bad_len = lens_s.copy()
    bad_len[0], bad_len[-1] = -4, 2 ** 31 - 1
    ids2, lens2, pos2 = T.fill_rows(ids_s, bad_len, bad_off, 3, cls, sep, pad, mask)
    assert ((lens2 >= 2) & (lens2 <= S)).all() and pos2.shape[1] == 3 and (pos2 < S - 1).all()
    with pytest.raises(ValueError):
        T.fill_rows(ids_s, lens_s, segoff, 17)
    with pytest.raises(ValueError):
        T.fill_rows(ids_s[:, :2], lens_s, segoff, 4)
    with pytest.raises(ValueError):
        T.split_masks("a", "")


def test_a_vocabulary_without_mask_is_refused(small):
    from agent_tpu_amd.runtime.classify import ClassifyEngine

    cfg = config_for("bert-tiny", mlm_head=True)
    vocab = T.WordPieceVocab.load(small[2])
    assert vocab.mask_id is None and small[1].mask_id == small[1].entries.index(b"[MASK]")
    eng = ClassifyEngine(cfg, init_random(cfg, seed=0), torch.device("cpu"), batch_rows=4, seq_len=16, vocab=vocab)
    with pytest.raises(ValueError) as e:
        eng.fill_texts(["a [MASK]"])
    assert str(e.value) == eng.FILL_NO_MASK_ID == "vocabulary has no [MASK] token"


def test_a_long_tailed_text_does_not_depend_on_its_chunk():
    """The pieces of a text are cut to ``max_row_bytes`` in total, text by text: the last text of a full chunk
    of long-tailed texts keeps its words before the mask (one budget for the whole chunk would run out and
    leave it ``[CLS] [MASK] [SEP]``) and gives what it gives alone."""
    from agent_tpu_amd.runtime.classify import ClassifyEngine

    cfg = config_for("bert-tiny", mlm_head=True)
    eng = ClassifyEngine(cfg, init_random(cfg, seed=3, bias_std=0.02), torch.device("cpu"), batch_rows=4, seq_len=32,
                         max_row_bytes=64)
    texts = [w + " [MASK] " + "tail " * 30 for w in make_text_rows(4, words_per_row=3, seed=9)]
    assert sum(len(t) for t in texts) > 4 * 64 + 4 * 60
    many = eng.fill_texts(texts, 5)
    assert (many.pos[:, 0] >= 2).all() and many.truncated == []
    for r in range(4):
        one = eng.fill_texts([texts[r]], 5)
        assert torch.equal(one.pos[0], many.pos[r]) and torch.equal(one.tok[0], many.tok[r]), r
        torch.testing.assert_close(one.prob[0], many.prob[r], atol=1e-6, rtol=0)
    # the cut itself: 64 bytes of pieces per text, the masks kept
    long = "a " * 40 + "[MASK] b [MASK]"
    res = eng.fill_texts([long], 2)
    assert res.pos[0].tolist() == [-1, -1] or res.pos[0, 1] == res.pos[0, 0] + 1  # nothing is left between them


# ---------------------------------------------------------------- pack layout
def test_pack_layout_without_and_with_the_mlm_head():
    cfg = config_for("bert-tiny", num_labels=3)
    mlm = config_for("bert-tiny", num_labels=3, mlm_head=True)
    every = config_for("bert-tiny", num_labels=3, qa_head=True, tag_labels=7, mlm_head=True)
    assert BertConfig().mlm_head is False and cfg.mlm_head is False
    plain, with_mlm, with_all = list(param_specs(cfg)), list(param_specs(mlm)), list(param_specs(every))
    H, V = cfg.hidden, cfg.vocab_size
    assert plain[-1][0] == "cls_b" and all(not n.startswith("mlm_") for n, _, _ in plain)
    assert with_mlm[:-5] == plain  # only the five MLM tensors are added, after the existing heads
    assert with_mlm[-5:] == [("mlm_w", (H, H), torch.bfloat16), ("mlm_b", (H,), torch.float32),
                             ("mlm_ln_g", (H,), torch.float32), ("mlm_ln_b", (H,), torch.float32),
                             ("mlm_out_b", (V,), torch.float32)]
    assert [n for n, _, _ in with_all[-9:-5]] == ["qa_w", "qa_b", "tag_w", "tag_b"] and with_all[-5:] == with_mlm[-5:]
    count = lambda specs: sum(math.prod(s) for _, s, _ in specs)  # noqa: E731
    assert cfg.param_count() == count(plain) and every.param_count() == count(with_all)
    assert mlm.param_count() == count(with_mlm) == count(plain) + H * H + 3 * H + V  # no second [V, H] table
    a, b = init_random(cfg, seed=5, bias_std=0.02), init_random(mlm, seed=5, bias_std=0.02)
    for name in a.names():  # rand_fill is keyed by name: the other tensors keep their bits
        assert torch.equal(a[name], b[name]), name
    assert torch.equal(a.buffer, b.buffer[:a.buffer.numel()])  # packs of existing configs: byte-identical
    assert b["mlm_w"].float().std().item() > 0.01 and b["mlm_b"].abs().sum().item() > 0
    assert (b["mlm_ln_g"] == 1).all() and not b["mlm_ln_b"].any() and b["mlm_out_b"].abs().sum().item() > 0
    assert not init_random(mlm, seed=5)["mlm_out_b"].any()  # *_b is a bias: zero without bias_std
    digest = hashlib.sha256(init_random(cfg, seed=0).buffer.view(torch.uint8).numpy().tobytes()).hexdigest()
    assert digest == PLAIN_PACK_SHA256
    model = BertClassifier(mlm, b)
    fi = model.fill_inputs()
    assert fi is model.fill_inputs() and fi["E"].data_ptr() == b["emb.word"].data_ptr()  # tied: the same storage
    with pytest.raises(ValueError, match="model has no MLM head"):
        BertClassifier(cfg, a).fill_inputs()


# ------------------------------------------------------------------ HF parity
HF_SEED = 13  # HF alone leaves 15 of 16 masks comparable at k = 5 (every gap between ranks 1 .. 6 above 4e-4)


def test_mask_logits_match_hf_masked_lm():
    transformers = pytest.importorskip("transformers")
    hcfg = transformers.BertConfig(vocab_size=4096, hidden_size=256, num_hidden_layers=2, num_attention_heads=4,
                                   intermediate_size=1024, max_position_embeddings=512, type_vocab_size=2,
                                   hidden_act="gelu", layer_norm_eps=1e-12, attn_implementation="eager",
                                   tie_word_embeddings=True)
    torch.manual_seed(HF_SEED)
    hf = transformers.BertForMaskedLM(hcfg).eval()
    with torch.no_grad():
        for p in hf.parameters():  # our pack stores bf16 weights: give HF the same values
            p.copy_(p.bfloat16().float())
        hf.cls.predictions.bias.copy_(torch.linspace(-0.5, 0.5, 4096))
        hf.cls.predictions.transform.LayerNorm.weight.copy_(torch.linspace(0.75, 1.25, 256))
        hf.cls.predictions.transform.LayerNorm.bias.copy_(torch.linspace(-0.125, 0.125, 256))
    sd = hf.state_dict()
    assert "cls.predictions.transform.dense.weight" in sd and "cls.predictions.bias" in sd
    cfg = config_for("bert-tiny", mlm_head=True)
    pack = from_hf_state_dict(cfg, sd, head="mlm")
    assert torch.equal(pack["mlm_w"].float(), sd["cls.predictions.transform.dense.weight"])
    assert torch.equal(pack["mlm_out_b"], sd["cls.predictions.bias"]) and not pack["cls_w"].any()
    ours = BertClassifier(cfg, pack, fp32=True)
    S, k = 64, 5
    texts = [" ".join(w.split()[:3 + i] + ["[MASK]"] + w.split()[3 + i:] + (["[MASK]"] if i % 2 else []))
             for i, w in enumerate(make_text_rows(10, words_per_row=12, seed=4))] + ["[MASK]"]
    pieces, segoff, mrow, mord = [], [0], [], []
    for i, t in enumerate(texts):
        ps = T.split_masks(t)[0]
        pieces += ps
        segoff.append(len(pieces))
        mrow += [i] * (len(ps) - 1)
        mord += list(range(len(ps) - 1))
    ids_s, lens_s = T.tokenize_rows([p.encode() for p in pieces], S, 4096)
    ids, lens, pos = T.fill_rows(ids_s, lens_s, np.array(segoff, dtype=np.int32), 4)
    R = len(mrow)
    mask = (np.arange(S)[None, :] < lens[:, None]).astype(np.int64)
    logits = torch.zeros((R, 4096))
    i32 = lambda a: torch.tensor(a, dtype=torch.int32)  # noqa: E731
    with torch.no_grad():
        ref_all = hf(input_ids=torch.from_numpy(ids).long(), attention_mask=torch.from_numpy(mask)).logits
        tok, logit, prob, lse = ours.fills(torch.from_numpy(ids), torch.from_numpy(lens), torch.from_numpy(pos),
                                           i32(mrow), i32(mord), k, logits_out=logits)
    ref = torch.stack([ref_all[b, pos[b, j]] for b, j in zip(mrow, mord)])
    assert R == 16 and (tok >= 0).all()
    torch.testing.assert_close(logits, ref, atol=2e-4, rtol=1e-4)
    torch.testing.assert_close(lse, torch.logsumexp(ref, 1), atol=2e-4, rtol=1e-4)
    rp = torch.softmax(ref, 1)
    torch.testing.assert_close(prob, torch.gather(rp, 1, tok.long()), atol=1e-4, rtol=0)
    # the top-k ids equal HF's wherever HF's own gap between ranks k and k + 1 exceeds twice the atol
    top = ref.topk(k + 1, 1)
    gaps = top.values[:, :-1] - top.values[:, 1:]
    comparable = (gaps > 2 * 2e-4).all(1)
    assert comparable.float().mean().item() >= 0.75, comparable.float().mean().item()
    assert torch.equal(tok[comparable].long(), top.indices[comparable, :k])
    # an untied decoder is refused; a tied one that is present is accepted
    tied = dict(sd)
    tied["cls.predictions.decoder.weight"] = sd["bert.embeddings.word_embeddings.weight"].clone()
    assert torch.equal(from_hf_state_dict(cfg, tied, head="mlm").buffer, pack.buffer)
    untied = dict(sd)
    untied["cls.predictions.decoder.weight"] = sd["bert.embeddings.word_embeddings.weight"] + 1e-3
    with pytest.raises(ValueError, match="untied MLM decoder"):
        from_hf_state_dict(cfg, untied, head="mlm")
    with pytest.raises(ValueError):
        from_hf_state_dict(config_for("bert-tiny"), sd, head="mlm")


# --------------------------------------------------------- reference vocab_topk
def test_vocab_select_ref_order_and_edges():
    lg = torch.tensor([[1.0, 3.0, 3.0, -0.0, 0.0, float("nan"), 3.0, NINF],
                       [float("nan")] * 8,
                       [2.0, 2.0, 2.0, 2.0, 2.0, 2.0, 2.0, 2.0]])
    tok, val, prob, lse = ops.vocab_select_ref(lg, 10)
    assert tok[0].tolist() == [1, 2, 6, 0, 3, 4, 5, 7, -1, -1]  # ties by token id; -0.0 == 0.0; NaN as -inf; k > V
    assert val[0, :4].tolist() == [3.0, 3.0, 3.0, 1.0] and (val[0, 6:] == NINF).all() and (prob[0, 6:] == 0).all()
    want = math.log(3 * math.exp(3.0) + math.exp(1.0) + 2.0)
    assert abs(lse[0].item() - want) < 1e-6 and abs(prob[0, 0].item() - math.exp(3.0 - want)) < 1e-7
    assert abs(prob[0, :8].sum().item() - 1) < 1e-6
    assert tok[1].tolist() == list(range(8)) + [-1, -1] and (val[1] == NINF).all() and (prob[1] == 0).all()
    assert lse[1].item() == NINF  # an empty sum
    assert tok[2].tolist() == list(range(8)) + [-1, -1] and abs(lse[2].item() - (2.0 + math.log(8))) < 1e-6
    # lse_in replaces the normaliser of prob only; an invalid slot is (-1, -inf, 0) with lse = 0
    given = torch.tensor([5.0, 1.0, 4.0])
    valid = torch.tensor([1, 1, 0], dtype=torch.int32)
    tok2, val2, prob2, lse2 = ops.vocab_select_ref(lg, 3, valid=valid, lse_in=given)
    assert torch.equal(tok2[:2], tok[:2, :3]) and torch.equal(lse2[:2], lse[:2])
    assert abs(prob2[0, 0].item() - math.exp(3.0 - 5.0)) < 1e-7
    assert tok2[2].tolist() == [-1, -1, -1] and (val2[2] == NINF).all() and (prob2[2] == 0).all() and lse2[2] == 0
    # the CPU path of the op: logits_out, then the selection of them
    g = torch.Generator().manual_seed(3)
    t, E, b = torch.randn(5, 64, generator=g), torch.randn(40, 64, generator=g), torch.randn(40, generator=g)
    out = torch.zeros(5, 40)
    got = ops.vocab_topk(t, E, b, 7, logits_out=out)
    torch.testing.assert_close(out, t @ E.t() + b)
    for x, y in zip(got, ops.vocab_select_ref(out, 7)):
        assert torch.equal(x, y)
    for kw in (dict(k=0), dict(k=33)):
        with pytest.raises(ValueError):
            ops.vocab_topk(t, E, b, kw["k"])
    with pytest.raises(ValueError):
        ops.vocab_topk(t[:, :48], E[:, :48], b, 3)
    assert ops.vocab_topk_splits(30522) == 60 and ops.vocab_topk_splits(1) == 1 and ops.vocab_topk_splits(513) == 2


def test_mask_gather_ref_and_targets_on_the_cpu():
    cfg = config_for("bert-tiny", mlm_head=True)
    pack = init_random(cfg, seed=2, bias_std=0.02)
    model = BertClassifier(cfg, pack, fp32=True)
    ids_s, lens_s = T.tokenize_rows([b"alpha beta", b"gamma", b"", b"delta epsilon zeta"], 16, 4096)
    ids, lens, pos = T.fill_rows(ids_s, lens_s, np.array([0, 2, 4], dtype=np.int32), 2)
    i32 = lambda a: torch.tensor(a, dtype=torch.int32)  # noqa: E731
    args = (torch.from_numpy(ids), torch.from_numpy(lens), torch.from_numpy(pos), i32([0, 1, 1, 5]), i32([0, 0, 1, 0]))
    lg = torch.zeros(4, 4096)
    tok, logit, prob, lse = model.fills(*args, 4, logits_out=lg)
    assert (tok[:2] >= 0).all() and (tok[2:] == -1).all() and (lse[2:] == 0).all()  # a missing mask, a bad row
    tids = torch.tensor([int(tok[0, 1]), 9, int(tok[0, 0]), 4000])
    t2, l2, p2, lse2 = model.fills(*args, 3, tids=tids)
    assert t2.shape == (4, 3) and t2[0, :2].tolist() == [int(tok[0, 0]), int(tok[0, 1])]
    assert torch.equal(l2[0, :2], logit[0, :2]) and torch.equal(p2[0, :2], prob[0, :2]) and torch.equal(lse2, lse)
    assert set(t2[1].tolist()) <= set(tids.tolist()) and (t2[2:] == -1).all()
    assert torch.equal(l2[1], lg[1][t2[1].long()])


# ------------------------------------------------------------- op contract
TEXTS = ["matrix cores [MASK] tiles", "a [MASK] for [MASK]", "[MASK]", "gpus multiply [MASK], naïve café in [MASK]",
         "lorem ipsum " * 30 + "[MASK]"]


@pytest.fixture()
def op(monkeypatch):
    monkeypatch.setenv("CLASSIFY_DEVICE", "cpu")
    from ops import get_batch_op, get_op

    return get_op("map_fill"), get_batch_op("map_fill")


def _close(got, want):
    """Two results of the op on a CPU engine: the same candidates, the scores equal up to the last bits (the
    PyTorch reference path is not batch-invariant)."""
    strip = lambda r: [[(m["start"], m["end"], [(c["token_id"], c["token"]) for c in m["candidates"]])  # noqa: E731
                        for m in x] for x in r["fills"]]
    assert strip(got) == strip(want)
    flat = lambda r: [c["score"] for x in r["fills"] for m in x for c in m["candidates"]]  # noqa: E731
    np.testing.assert_allclose(flat(got), flat(want), atol=1e-6, rtol=0)
    skip = ("elapsed_ms", "rows_per_sec", "fills")
    assert {k: v for k, v in got.items() if k not in skip} == {k: v for k, v in want.items() if k not in skip}


def test_op_output_both_forms(op, small):
    run, _ = op
    r = run({"texts": TEXTS, "model_path": MODEL, "top_k": 3})
    for key in ("ok", "op", "model_path", "row_count", "elapsed_ms", "rows_per_sec", "top_k", "mask_token", "fills",
                "truncated"):
        assert key in r, key
    assert r["ok"] and r["op"] == "map_fill" and r["row_count"] == len(TEXTS) and r["top_k"] == 3
    assert "dp_world_size" not in r and len(r["fills"]) == len(TEXTS) and r["mask_token"] == "[MASK]"
    assert r["truncated"] == [[4, 0]] and r["fills"][4][0]["candidates"] == []  # beyond the 38 tokens of a row
    for text, row in zip(TEXTS, r["fills"]):
        assert len(row) == text.count("[MASK]")
        assert [m["start"] for m in row] == sorted(m["start"] for m in row)
        for m in row:
            assert set(m) == {"start", "end", "candidates"} and text[m["start"]:m["end"]] == "[MASK]"
            for c in m["candidates"]:
                assert set(c) == {"token_id", "token", "score"} and c["token"] is None and 0 < c["score"] <= 1
    assert all(len(m["candidates"]) == 3 for row in r["fills"][:4] for m in row)
    json.dumps(r)
    one = run({"text": TEXTS[1], "model_path": MODEL, "top_k": 3})
    assert one["row_count"] == 1 and len(one["fills"]) == 1
    _close(dict(one, row_count=0, truncated=0), dict(r, row_count=0, truncated=0, fills=[r["fills"][1]]))
    assert run({"texts": [], "model_path": MODEL})["fills"] == []
    # another mask token: the same row, the offsets of the literal string
    alt = run({"text": "a <m> for <m>", "model_path": MODEL, "top_k": 3, "mask_token": "<m>"})
    assert [(m["start"], m["end"]) for m in alt["fills"][0]] == [(2, 5), (10, 13)] and alt["mask_token"] == "<m>"
    assert [[c["token_id"] for c in m["candidates"]] for m in alt["fills"][0]] == [
        [c["token_id"] for c in m["candidates"]] for m in one["fills"][0]]
    # targets as ids: only those tokens, best first, top_k capped by their number, the full-vocabulary score
    best = one["fills"][0][0]["candidates"][0]
    tg = run({"text": TEXTS[1], "model_path": MODEL, "top_k": 5, "targets": [7, best["token_id"], 7, 1234]})
    for m in tg["fills"][0]:
        assert len(m["candidates"]) == 3 and {c["token_id"] for c in m["candidates"]} == {7, best["token_id"], 1234}
    first = tg["fills"][0][0]["candidates"][0]
    assert first["token_id"] == best["token_id"] and abs(first["score"] - best["score"]) < 1e-7
    # targets as strings on a WordPiece vocabulary; token strings in the candidates
    wp = MODEL + "&vocab=" + small[0]
    vocab = small[1]
    names = [vocab.entries[20].decode(), vocab.entries[33].decode()]
    ws = run({"text": "x [MASK] y", "model_path": wp, "targets": names + [20], "top_k": 1})
    assert len(ws["fills"][0][0]["candidates"]) == 1 and ws["fills"][0][0]["candidates"][0]["token"] in names
    full = run({"text": "x [MASK] y", "model_path": wp, "top_k": 32})
    for c in full["fills"][0][0]["candidates"]:
        assert c["token"] == (vocab.entries[c["token_id"]].decode() if c["token_id"] < len(vocab) else None)


def test_op_errors(op, small):
    run, _ = op
    from ops.map_fill import ERRORS

    base = {"text": "a [MASK]", "model_path": MODEL}
    cases = [({}, "missing"), ({"model_path": MODEL}, "missing"), (dict(base, texts=["[MASK]"]), "both"),
             (dict(base, text=5), "text"), ({"texts": "a"}, "texts"), ({"texts": ["[MASK]", 3]}, "texts"),
             (dict(base, top_k=0), "top_k"), (dict(base, top_k=33), "top_k"), (dict(base, top_k="3"), "top_k"),
             (dict(base, top_k=True), "top_k"), (dict(base, mask_token=""), "mask_token"),
             (dict(base, mask_token=4), "mask_token"), (dict(base, targets=[]), "targets"),
             (dict(base, targets="cat"), "targets"), (dict(base, targets=[1.5]), "targets"),
             (dict(base, targets=[""]), "targets"), (dict(base, targets=list(range(33))), "targets"),
             (dict(base, targets=[True]), "targets"),
             (dict(base, model_path="bert-tiny?batch=4&seq=40"), "mlm"),
             (dict(base, model_path=MODEL + "&vocab=" + small[2]), "mask_id"),
             (dict(base, targets=["cat"]), "target_vocab"),
             (dict(base, targets=[4096]), "target_unknown"), (dict(base, targets=[-1]), "target_unknown"),
             (dict(base, targets=["no-such-token"], model_path=MODEL + "&vocab=" + small[0]), "target_unknown")]
    seen = set()
    for payload, key in cases:
        with pytest.raises(ValueError) as e:
            run(payload)
        assert str(e.value) == ERRORS[key], (payload, key)
        seen.add(key)
    for payload, key, index in (({"texts": ["[MASK]", "none"], "model_path": MODEL}, "no_mask", 1),
                                (dict(base, mask_token="<m>"), "no_mask", 0),
                                ({"texts": ["[MASK] a", "b", " ".join(["[MASK]"] * 17)], "model_path": MODEL}, "no_mask", 1),
                                ({"texts": ["[MASK] a", " ".join(["[MASK]"] * 17)], "model_path": MODEL}, "too_many", 1)):
        with pytest.raises(ValueError) as e:
            run(payload)
        assert str(e.value) == ERRORS[key].format(index=index) and str(index) in str(e.value)
        seen.add(key)
    assert seen == set(ERRORS)
    assert run({"text": " ".join(["[MASK]"] * 16), "model_path": MODEL})["ok"]
    import ops.map_fill as mf

    contract = open(os.path.join(os.path.dirname(mf.__file__), "map_fill.CONTRACT.md")).read()
    for msg in ERRORS.values():
        assert msg in contract, msg
    for section in ("## Purpose", "## Inputs (payload)", "## Outputs", "## Notes"):
        assert section in contract


def test_model_specs(tmp_path, monkeypatch):
    monkeypatch.setenv("CLASSIFY_DEVICE", "cpu")
    from safetensors.torch import save_file

    from ops import get_op
    from ops._gpu_runtime import _load_host_pack, parse_spec

    assert parse_spec("bert-tiny").mlm is False and parse_spec("bert-tiny?mlm=1").mlm is True
    assert parse_spec("bert-tiny?mlm=1").head is True and parse_spec("bert-tiny?mlm=0").mlm is False
    cfg = config_for("bert-tiny", mlm_head=True)
    pack = init_random(cfg, seed=4, bias_std=0.02)
    tensors = {n: pack[n].clone() for n in pack.names() if not n.startswith(("pool_", "cls_"))}
    path = str(tmp_path / "mlm.safetensors")
    save_file(tensors, path)
    with open(path + ".json", "w") as f:
        json.dump({"preset": "bert-tiny", "head": "mlm"}, f)
    spec = parse_spec(path)
    assert spec.mlm is True and spec.head is False and spec.qa is False and spec.tags == 0
    got = _load_host_pack(spec, config_for(spec.preset, num_labels=spec.labels, mlm_head=spec.mlm))
    assert torch.equal(got["mlm_out_b"], pack["mlm_out_b"]) and not got["pool_w"].any() and not got["cls_w"].any()
    # the other ops refuse it, as they refuse "qa" and "token" files
    from types import SimpleNamespace

    from ops import map_answer, map_rerank, map_tag

    with pytest.raises(ValueError) as e:
        map_rerank.check_model(SimpleNamespace(spec=spec), map_rerank.options({}))
    assert str(e.value) == map_rerank.ERRORS["head"]
    with pytest.raises(ValueError) as e:
        map_answer.check_model(SimpleNamespace(spec=spec), map_answer.options({}))
    assert str(e.value) == map_answer.ERRORS["qa"]
    with pytest.raises(ValueError) as e:
        map_tag.check_model(SimpleNamespace(spec=spec), map_tag.options({}))
    assert str(e.value) == map_tag.ERRORS["tags"]
    r = get_op("map_fill")({"text": "a [MASK] b", "model_path": path + "?batch=4&seq=40", "top_k": 2})
    assert len(r["fills"][0][0]["candidates"]) == 2
    with pytest.raises(ValueError) as e:
        get_op("map_classify")({"texts": ["a"], "model_path": path + "?batch=4&seq=40", "allow_fallback": False})
    assert str(e.value) == "model has no classifier head"
    del tensors["mlm_out_b"]
    save_file(tensors, path)
    with pytest.raises(KeyError, match="mlm_out_b"):
        _load_host_pack(spec, cfg)


def test_batched_jobs_equal_single_jobs(op):
    run, batch = op
    jobs = [{"texts": TEXTS, "model_path": MODEL, "top_k": 3},
            {"text": 7},
            {"text": TEXTS[1], "model_path": MODEL, "top_k": 3},
            {"texts": TEXTS[3:], "model_path": MODEL, "targets": [5, 6, 7]},
            {"texts": [], "model_path": MODEL},
            {"text": "no mask", "model_path": MODEL},
            {"text": TEXTS[0], "model_path": MODEL, "targets": ["cat"]},
            {"text": TEXTS[0], "model_path": "bert-tiny?batch=4&seq=40"}]
    res = batch(jobs)
    assert [r[0] for r in res] == ["ok", "err", "ok", "ok", "ok", "err", "err", "err"]
    assert str(res[1][1]) == "payload.text must be a string" and isinstance(res[6][1], ValueError)
    assert str(res[5][1]) == "payload text 0 has no mask token"
    assert res[3][1]["truncated"] == [[1, 0]] and res[0][1]["truncated"] == [[4, 0]]
    for job, (kind, got) in zip(jobs, res):
        if kind == "ok":
            _close(got, run(job))
