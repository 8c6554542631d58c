"""Token classification on the CPU: the pack layout with the tag head, the folded head inputs, HF parity of
the fp32 oracle, ``tag_select_ref`` against a brute-force grouping and hand-worked cases, the CPU path of
``tag_entities`` and its checks, the character mapping, and the ``map_tag`` op contract."""
import hashlib
import itertools
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

MODEL = "bert-tiny?tags=5&batch=4&seq=40&seed=3"

#: sha256 of init_random(bert-tiny, num_labels=3, seed=0) computed on the commit before the span and tag heads
PLAIN_PACK_SHA256 = "f885b05bb79819e9e2fc35127de95f51241096c01aa11b1a62b71d8f4aa3e714"


@pytest.fixture(scope="module")
def small(tmp_path_factory):
    path = tmp_path_factory.mktemp("wp") / "vocab.txt"
    with open(path, "wb") as f:
        f.write("\n".join(make_wordpiece_vocab(300, seed=1)).encode("utf-8") + b"\n")
    return str(path), T.WordPieceVocab.load(str(path))


# ---------------------------------------------------------------- pack layout
def test_pack_layout_without_and_with_the_tag_head():
    cfg = config_for("bert-tiny", num_labels=3)
    tag = config_for("bert-tiny", num_labels=3, tag_labels=7)
    both = config_for("bert-tiny", num_labels=3, qa_head=True, tag_labels=7)
    assert BertConfig().tag_labels == 0 and cfg.tag_labels == 0
    plain, with_tag, with_both = list(param_specs(cfg)), list(param_specs(tag)), list(param_specs(both))
    H = cfg.hidden
    assert plain[-1][0] == "cls_b" and all(not n.startswith("tag_") for n, _, _ in plain)
    assert with_tag[:-2] == plain  # only tag_w / tag_b are added, after the existing heads
    assert with_tag[-2:] == [("tag_w", (7, H), torch.bfloat16), ("tag_b", (7,), torch.float32)]
    assert [n for n, _, _ in with_both[-4:]] == ["qa_w", "qa_b", "tag_w", "tag_b"]
    count = lambda specs: sum(math.prod(s) for _, s, _ in specs)  # noqa: E731
    assert cfg.param_count() == count(plain) and tag.param_count() == count(with_tag) == count(plain) + 7 * H + 7
    assert both.param_count() == count(with_both)
    a, b = init_random(cfg, seed=5, bias_std=0.02), init_random(tag, seed=5, bias_std=0.02)
    for name in a.names():  # rand_fill is keyed by name: the other tensors keep their bits
        assert torch.equal(a[name], b[name]), name
    assert torch.equal(a.buffer, b.buffer[:a.buffer.numel()])
    assert b["tag_w"].float().std().item() > 0.01 and b["tag_b"].abs().sum().item() > 0
    digest = hashlib.sha256(init_random(cfg, seed=0).buffer.view(torch.uint8).numpy().tobytes()).hexdigest()
    assert digest == PLAIN_PACK_SHA256


def test_tag_inputs_fold_the_last_layernorm():
    cfg = config_for("bert-tiny", tag_labels=5)
    pack = init_random(cfg, seed=2, bias_std=0.02)
    last = f"l{cfg.layers - 1}."
    pack[last + "ln2_g"].copy_(torch.linspace(0.5, 1.5, cfg.hidden))
    pack[last + "ln2_b"].copy_(torch.linspace(-0.2, 0.3, cfg.hidden))
    model = BertClassifier(cfg, pack)
    ti = model.tag_inputs()
    assert ti is model.tag_inputs()  # built once
    w, g, b = pack["tag_w"].double(), pack[last + "ln2_g"].double(), pack[last + "ln2_b"].double()
    assert all(t.dtype == torch.float32 for t in ti.values())
    assert torch.equal(ti["u"], (pack[last + "ln2_g"].view(1, -1) * pack["tag_w"].float()))
    assert torch.equal(ti["su"], ti["u"].double().sum(1).float())
    assert torch.equal(ti["c"], ((b.view(1, -1) * w).sum(1) + pack["tag_b"].double()).float())
    assert torch.equal(ti["w"], pack["tag_w"].float()) and torch.equal(ti["b"], pack["tag_b"])
    # the fused form is the LayerNorm followed by the head, at the text tokens
    x = torch.randn(6, cfg.hidden, dtype=torch.float64)
    mu, var = x.mean(1, keepdim=True), x.var(1, unbiased=False, keepdim=True)
    rstd = 1 / torch.sqrt(var + cfg.eps)
    want = ((x - mu) * rstd * g + b) @ w.t() + pack["tag_b"].double()
    fin = torch.cat([rstd, rstd * mu], 1)
    got = ops.tag_logits_ref(x, torch.tensor([6]), 1, ti["u"], ti["su"], ti["c"], fin=fin, dtype=torch.float64)
    torch.testing.assert_close(got.view(6, 5)[1:5], want[1:5], atol=1e-6, rtol=1e-6)
    assert torch.isinf(got.view(6, 5)[[0, 5]]).all()
    with pytest.raises(ValueError, match="model has no tag head"):
        BertClassifier(config_for("bert-tiny"), init_random(config_for("bert-tiny"))).tag_inputs()


# ------------------------------------------------------------------ HF parity
def test_tag_logits_match_hf_token_classification():
    transformers = pytest.importorskip("transformers")
    hcfg = transformers.BertConfig(vocab_size=4096, hidden_size=256, num_hidden_layers=2, num_attention_heads=4,
                                   intermediate_size=1024, max_position_embeddings=512, type_vocab_size=2,
                                   hidden_act="gelu", layer_norm_eps=1e-12, attn_implementation="eager", num_labels=7,
                                   classifier_dropout=0.0)
    torch.manual_seed(13)
    hf = transformers.BertForTokenClassification(hcfg).eval()
    with torch.no_grad():
        for p in hf.parameters():  # our pack stores bf16 weights: give HF the same values
            p.copy_(p.bfloat16().float())
        hf.classifier.bias.copy_(torch.linspace(-0.5, 0.5, 7))
    sd = hf.state_dict()
    assert not any("pooler" in k for k in sd)
    cfg = config_for("bert-tiny", tag_labels=7)
    pack = from_hf_state_dict(cfg, sd, head="token")
    assert torch.equal(pack["tag_w"].float(), sd["classifier.weight"]) and not pack["cls_w"].any()
    ours = BertClassifier(cfg, pack, fp32=True)
    S = 64
    rows = [r.encode() for r in make_text_rows(6, words_per_row=12, seed=4)] + [b"", b"short one"]
    ids, lens = T.tokenize_rows(rows, S, 4096)
    mask = (np.arange(S)[None, :] < lens[:, None]).astype(np.int64)
    logits = torch.zeros((8, S, 7))
    lt, lb = ops.tag_tables(ops.default_tag_names(7))[1:]
    with torch.no_grad():
        ref = hf(input_ids=torch.from_numpy(ids).long(), attention_mask=torch.from_numpy(mask)).logits
        ent, ent_sum, count = ours.tags(torch.from_numpy(ids), torch.from_numpy(lens), lt, lb, 1, 16,
                                        logits_out=logits)
    pos = torch.arange(S).view(1, S)
    text = (pos >= 1) & (pos <= torch.from_numpy(lens).view(-1, 1) - 2)
    assert text.any() and not text[6].any()
    torch.testing.assert_close(logits[text], ref[text], atol=2e-4, rtol=1e-4)
    assert torch.isinf(logits[~text]).all() and (logits[~text] < 0).all()
    want = ops.tag_select_ref(logits, torch.from_numpy(lens), lt, lb, 1, 16)
    assert torch.equal(ent, want[0]) and torch.equal(ent_sum, want[1]) and torch.equal(count, want[2])
    assert count[6] == 0  # the empty row
    # the default routing keeps classifier.* in the row classifier, and a model without the head ignores it
    seq = from_hf_state_dict(config_for("bert-tiny", num_labels=7), sd)
    assert "tag_w" not in seq and torch.equal(seq["cls_w"].float(), sd["classifier.weight"])
    with pytest.raises(ValueError):
        from_hf_state_dict(cfg, sd, head="other")


# ------------------------------------------------- selection: the reference twin
def _brute(logits, length, lt, lb, mode, ids, cont):
    """Independent grouping: runs of one effective type (itertools.groupby), each cut before every token
    that begins (B- label or first of the text) and is not a continuation."""
    S, L = logits.shape
    hi = min(max(length, 2), S) - 2
    own = {}
    for j in range(1, hi + 1):
        row = [float("-inf") if math.isnan(v) else v for v in logits[j].tolist()]
        own[j] = min(range(L), key=lambda c: (-row[c], c))
    is_cont = {j: mode == 2 and j > 1 and 0 <= ids[j] < len(cont) and bool(cont[ids[j]]) for j in own}
    eff = {}
    for j in sorted(own):
        eff[j] = eff[j - 1] if is_cont[j] else own[j]
    recs = []
    if mode == 0:
        return [(j - 1, j - 1, eff[j], [j]) for j in sorted(own) if lt[eff[j]] >= 0]
    for t, run in itertools.groupby(sorted(own), key=lambda j: lt[eff[j]]):
        run = list(run)
        if t < 0:
            continue
        cuts = [0] + [i for i, j in enumerate(run) if i > 0 and lb[eff[j]] and not is_cont[j]] + [len(run)]
        for a, b in zip(cuts, cuts[1:]):
            seg = run[a:b]
            recs.append((seg[0] - 1, seg[-1] - 1, t, [j for j in seg if not is_cont[j]]))
    return recs


@pytest.mark.parametrize("S", [3, 9, 40])
def test_tag_select_ref_equals_brute_force(S):
    g = torch.Generator().manual_seed(S)
    B, L, V = 6, 7, 20
    values = torch.tensor([-1.0, 0.0, 0.5, 0.5, 2.0])
    logits = values[torch.randint(0, 5, (B, S, L), generator=g)]
    if S > 3:
        logits[1, 2] = float("nan")
        logits[1, 3, 4] = float("nan")
    lens = torch.tensor([S, S - 1, 2, -4, S + 9, max(3, S // 2)], dtype=torch.int32)
    names = ["O", "B-A", "I-A", "B-B", "I-B", "MISC", "PAD"]
    types, lt, lb = ops.tag_tables(names, outside=("O", "PAD"))
    assert types == ["A", "B", "MISC"] and lt.tolist() == [-1, 0, 0, 1, 1, 2, -1] and lb.tolist() == [0, 1, 0, 1, 0, 0, 0]
    ids = torch.randint(-2, V + 2, (B, S), generator=g, dtype=torch.int32)
    cont = (torch.rand(V, generator=g) < 0.5).to(torch.uint8)
    for mode in (0, 1, 2):
        for E in (1, 3, 64):
            ent, ent_sum, count, label, prob = ops.tag_select_ref(logits, lens, lt, lb, mode, E, ids, cont)
            for b in range(B):
                recs = _brute(logits[b], int(lens[b]), lt.tolist(), lb.tolist(), mode, ids[b].tolist(), cont.tolist())
                assert int(count[b]) == len(recs), (mode, E, b)
                for e in range(E):
                    if e < len(recs):
                        first, last, third, scored = recs[e]
                        assert ent[b, e].tolist() == [first, last, third, len(scored)], (mode, E, b, e)
                        want = np.float32(0)
                        for j in scored:
                            want = np.float32(want + np.float32(prob[b, j].item()))
                        assert ent_sum[b, e].item() == float(want)
                    else:
                        assert ent[b, e].tolist() == [-1, -1, -1, 0] and ent_sum[b, e].item() == 0.0
    # the probability is the softmax of the argmax, NaN logits aside
    lg = logits[0].double()
    sm = torch.softmax(lg, -1).max(-1).values
    hi = int(lens[0]) - 2
    torch.testing.assert_close(prob[0, 1:hi + 1].double(), sm[1:hi + 1], atol=1e-7, rtol=1e-6)
    assert label[0, 0] == -1 and prob[0, 0] == 0 and label[3].eq(-1).all()
    if S > 3:
        assert label[1, 2] == 0 and prob[1, 2] == 0  # an all-NaN token


def _hand(labels, names, mode, cont_at=(), outside=("O",)):
    """Entities of one row whose tokens carry ``labels`` (names), as (first, last, type name or label name, n)."""
    L, S = len(names), len(labels) + 2
    types, lt, lb = ops.tag_tables(names, outside)
    logits = torch.zeros(1, S, L)
    for j, name in enumerate(labels):
        logits[0, j + 1, names.index(name)] = 5.0
    ids = torch.zeros(1, S, dtype=torch.int32)
    for j in cont_at:
        ids[0, j + 1] = 1
    cont = torch.tensor([0, 1], dtype=torch.uint8)
    ent, _, count, _, _ = ops.tag_select_ref(logits, torch.tensor([S], dtype=torch.int32), lt, lb, mode, 8, ids, cont)
    k = int(count[0])
    return [(f, l, names[t] if mode == 0 else types[t], n) for f, l, t, n in ent[0, :k].tolist()]


def test_tag_grouping_hand_worked_cases():
    names = ["O", "B-X", "I-X", "B-Y", "I-Y", "MISC"]
    for mode in (1, 2):
        assert _hand(["O", "B-X", "I-X", "O"], names, mode) == [(1, 2, "X", 2)]
        assert _hand(["B-X", "B-X"], names, mode) == [(0, 0, "X", 1), (1, 1, "X", 1)]
        assert _hand(["I-X", "I-Y"], names, mode) == [(0, 0, "X", 1), (1, 1, "Y", 1)]
        assert _hand(["O", "I-X"], names, mode) == [(1, 1, "X", 1)]
        assert _hand(["MISC", "MISC", "B-X"], names, mode) == [(0, 1, "MISC", 2), (2, 2, "X", 1)]  # an untagged name
        assert _hand(["O", "O"], names, mode) == []
    assert _hand(["O", "B-X", "I-X", "O"], names, 0) == [(1, 1, "B-X", 1), (2, 2, "I-X", 1)]
    assert _hand(["MISC"], names, 0) == [(0, 0, "MISC", 1)]
    # a continuation whose own argmax differs from its head's: "simple" splits the word, "first" does not
    labels = ["B-X", "B-Y", "I-X", "O"]
    assert _hand(labels, names, 1, cont_at=(1,)) == [(0, 0, "X", 1), (1, 1, "Y", 1), (2, 2, "X", 1)]
    assert _hand(labels, names, 2, cont_at=(1,)) == [(0, 2, "X", 2)]  # the piece extends and is not scored
    assert _hand(["O", "B-X"], names, 2, cont_at=(1,)) == []           # a piece of an outside word
    assert _hand(["B-X", "O"], names, 2, cont_at=(0,)) == [(0, 0, "X", 1)]  # token 1 is never a continuation


def test_tag_entities_cpu_path_and_checks():
    g = torch.Generator().manual_seed(1)
    B, S, H, L, E = 3, 12, 64, 5, 4
    x = torch.randn(B * S, H, generator=g).bfloat16()
    u, c = torch.randn(L, H, generator=g) * 0.2, torch.randn(L, generator=g)
    su = u.double().sum(1).float()
    fin = torch.stack([torch.rand(B * S, generator=g) + 0.5, torch.randn(B * S, generator=g) * 0.1], 1)
    lens = torch.tensor([S, 7, 2], dtype=torch.int32)
    lt, lb = ops.tag_tables(ops.default_tag_names(L))[1:]
    ids = torch.randint(0, 9, (B, S), generator=g, dtype=torch.int32)
    cont = torch.tensor([0, 1, 0, 1, 0, 0, 1, 0, 0], dtype=torch.uint8)
    assert ops.tag_ok(S, H, L) and not ops.tag_ok(2, H, L) and not ops.tag_ok(S, 96, L) and not ops.tag_ok(S, H, 65)
    for mode in (0, 1, 2):
        for f in (fin, None):
            logits, label, prob = torch.zeros(B + 1, S, L), torch.zeros(B + 1, S, dtype=torch.int32), torch.zeros(B + 1, S)
            logits[B], label[B], prob[B] = 9.0, 9, 9.0
            ent, ent_sum, count = ops.tag_entities(x, lens, B, S, u, su, c, lt, lb, mode, E, fin=f, ids=ids, cont=cont,
                                                   label_out=label, prob_out=prob, logits_out=logits)
            want_lg = ops.tag_logits_ref(x, lens, B, u, su, c, f)
            want = ops.tag_select_ref(want_lg, lens, lt, lb, mode, E, ids, cont)
            assert torch.equal(logits[:B], want_lg) and torch.equal(ent, want[0]) and torch.equal(ent_sum, want[1])
            assert torch.equal(count, want[2]) and torch.equal(label[:B], want[3]) and torch.equal(prob[:B], want[4])
            assert (logits[B] == 9).all() and (label[B] == 9).all() and (prob[B] == 9).all()  # rows past B untouched
            assert count[2] == 0 and ent.shape == (B, E, 4)
    e0 = ops.tag_entities(x[:0], lens, 0, S, u, su, c, lt, lb, 1, E)
    assert e0[0].shape == (0, E, 4) and e0[2].shape == (0,)
    ok = dict(x=x, lens=lens, B=B, S=S, u=u, su=su, c=c, label_type=lt, label_begin=lb, mode=1, max_entities=E)
    bad = [dict(S=11), dict(mode=3), dict(mode=True), dict(max_entities=0), dict(max_entities=513),
           dict(max_entities=2.0), dict(lens=lens.long()), dict(lens=lens[:2]), dict(u=u[:, :32]), dict(c=c[:3]),
           dict(label_type=lt[:3]), dict(label_begin=lb.long()), dict(fin=fin[:5]), dict(fin=fin, su=None),
           dict(mode=2), dict(mode=2, ids=ids.long(), cont=cont), dict(mode=2, ids=ids, cont=cont.int()),
           dict(ent=torch.zeros(B, E, 3, dtype=torch.int32)), dict(count=torch.zeros(B - 1, dtype=torch.int32)),
           dict(logits_out=torch.zeros(B, S, L + 1)), dict(B=-1)]
    for kw in bad:
        with pytest.raises(ValueError):
            ops.tag_entities(**dict(ok, **kw))
    for S2, H2, L2 in ((2, 64, 5), (513, 64, 5), (12, 96, 5), (12, 1088, 5), (12, 64, 65)):
        with pytest.raises(ValueError, match="unsupported shape"):
            ops.tag_entities(torch.zeros(S2, H2, dtype=torch.bfloat16), torch.tensor([S2], dtype=torch.int32), 1, S2,
                             torch.zeros(L2, H2), None, torch.zeros(L2), torch.zeros(L2, dtype=torch.int32),
                             torch.zeros(L2, dtype=torch.int32), 1, 4)


# ---------------------------------------------- engine: characters of an entity
@pytest.fixture()
def cpu_handle(monkeypatch):
    monkeypatch.setenv("CLASSIFY_DEVICE", "cpu")
    from ops._gpu_runtime import get_gpu_handle

    return get_gpu_handle(MODEL)


def test_entities_widen_to_character_boundaries(cpu_handle):
    eng = cpu_handle.engine
    text = "a" + "€" * 10 + " end"  # 31 word bytes: pieces [0, 24) and [24, 31), the cut inside the 8th '€'
    row = text.encode()
    assert T.token_spans(row, 4096, 38)[:2] == [(0, 24), (24, 31)] and 0x80 <= row[24] <= 0xBF
    ent = torch.tensor([[[0, 0, 0, 1], [1, 1, 1, 2], [2, 2, 0, 1], [-1, -1, -1, 0]]], dtype=torch.int32)
    ent_sum = torch.tensor([[0.5, 1.5, 0.25, 0.0]])
    res = eng.map_tags(ent, ent_sum, torch.tensor([3], dtype=torch.int32), [text], "simple")
    a = res.entities[0]
    assert [(e["start"], e["end"], e["word"]) for e in a] == [(0, 9, "a" + "€" * 8), (8, 11, "€" * 3), (12, 15, "end")]
    assert [e["entity_group"] for e in a] == ["T0", "T1", "T0"] and [e["score"] for e in a] == [0.5, 0.75, 0.25]
    assert all(text[e["start"]:e["end"]] == e["word"] for e in a) and res.truncated == [] and res.counts == [3]
    none = eng.map_tags(torch.tensor([[[2, 2, 4, 1]]], dtype=torch.int32), torch.tensor([[0.5]]),
                        torch.tensor([5], dtype=torch.int32), [text], "none")
    assert none.entities[0] == [{"entity": "I-T1", "score": 0.5, "index": 3, "word": "end", "start": 12, "end": 15}]
    assert none.truncated == [0] and none.counts == [5]
    # a row longer than max_row_bytes is tokenized as the device cut it; offsets are those of the full string
    long = "é" * (eng.max_row_bytes // 2 + 40) + " tail"
    res = eng.map_tags(torch.tensor([[[0, 0, 1, 1]]], dtype=torch.int32), torch.tensor([[1.0]]),
                       torch.tensor([1], dtype=torch.int32), [long], "first")
    assert res.entities[0][0]["word"] == "é" * 12 and res.entities[0][0]["start"] == 0


TEXTS = ["matrix cores multiply tiles", "", "gpus multiply matrices with matrix cores, naïve café", "x",
         "rain is likely tomorrow in Zürich", "a recipe for bread " * 12, "sunny"]


def test_engine_tags_equal_model_on_twin_rows(cpu_handle):
    """More rows than ``batch_rows`` (chunks of 4), an empty row and a row longer than seq_len - 2 tokens."""
    h, eng = cpu_handle, cpu_handle.engine
    ids, lens = T.tokenize_rows([t.encode() for t in TEXTS], eng.S, h.cfg.vocab_size)
    assert lens.max() == eng.S and lens.min() == 2
    st = eng._tag_state()
    for mode, name in ((1, "simple"), (0, "none")):
        res = eng.tag_texts(TEXTS, name, 6)
        ent, ent_sum, count = eng.model.tags(torch.from_numpy(ids), torch.from_numpy(lens), st["label_type"],
                                             st["label_begin"], mode, 6)
        assert torch.equal(res.ent, ent) and res.counts == count.tolist()
        torch.testing.assert_close(res.ent_sum, ent_sum, atol=1e-5, rtol=1e-5)
        assert res.truncated == [i for i, c in enumerate(res.counts) if c > 6] and res.counts[1] == 0
        assert any(res.entities) and res.entities[1] == []
        for text, row, recs in zip(TEXTS, res.entities, res.ent.tolist()):
            toks = T.token_spans(text.encode(), h.cfg.vocab_size, eng.S - 2)
            for e, (first, last, third, n) in zip(row, recs):
                assert text[e["start"]:e["end"]] == e["word"] and e["word"] and 0 < e["score"] <= 1
                assert e["start"] <= len(text.encode()[:toks[first][0]].decode("utf-8", "ignore")) and n >= 1
                if mode == 0:
                    assert e["index"] == first + 1 and e["entity"] == st["names"][third]
    with pytest.raises(ValueError) as e:
        eng.tag_texts(TEXTS, "first", 6)
    assert str(e.value) == eng.TAG_NEEDS_VOCAB
    for kw in (dict(mode="average"), dict(mode=3), dict(max_entities=0), dict(max_entities=513)):
        with pytest.raises(ValueError):
            eng.tag_texts(TEXTS, **kw)
    assert eng.tag_texts([], "simple", 4).entities == []


def test_engine_first_mode_on_a_wordpiece_vocabulary(small, monkeypatch):
    monkeypatch.setenv("CLASSIFY_DEVICE", "cpu")
    from ops._gpu_runtime import get_gpu_handle

    path, vocab = small
    h = get_gpu_handle(MODEL + "&vocab=" + path)
    eng = h.engine
    cont = eng._tag_cont()
    assert cont is eng._tag_cont() and cont.dtype == torch.uint8 and cont.numel() == len(vocab)
    assert cont.tolist() == [int(len(e) > 2 and e.startswith(b"##")) for e in vocab.entries] and cont.any()
    rows = make_text_rows(6, words_per_row=7, seed=2)
    ids, lens = vocab.tokenize_rows([r.encode() for r in rows], eng.S)
    pieces = cont[torch.from_numpy(ids).long().clamp(0, len(vocab) - 1)].bool()
    assert pieces[:, 1:].any()  # the rows do hold ## pieces
    res = eng.tag_texts(rows, "first", 16)
    st = eng._tag_state()
    ent, ent_sum, count = eng.model.tags(torch.from_numpy(ids), torch.from_numpy(lens), st["label_type"],
                                         st["label_begin"], 2, 16, cont=cont)
    assert torch.equal(res.ent, ent) and res.counts == count.tolist()
    for i, (text, row, recs) in enumerate(zip(rows, res.entities, res.ent.tolist())):
        for e, (first, last, _, n) in zip(row, recs):
            assert text[e["start"]:e["end"]] == e["word"] and e["word"]
            assert not pieces[i, first + 1] or first == 0  # a group starts at a word head


# ------------------------------------------------------------- op contract
@pytest.fixture()
def op(monkeypatch):
    monkeypatch.setenv("CLASSIFY_DEVICE", "cpu")
    from ops import get_batch_op, get_op

    return get_op("map_tag"), get_batch_op("map_tag")


def _close(got, want):
    """Two results of the op on a CPU engine: the same entities, the scores equal up to the last bits (the
    PyTorch reference path is not batch-invariant)."""
    strip = lambda r: [[{k: v for k, v in e.items() if k != "score"} for e in x] for x in r["entities"]]  # noqa: E731
    assert strip(got) == strip(want)
    flat = lambda r: [e["score"] for x in r["entities"] for e in x]  # noqa: E731
    np.testing.assert_allclose(flat(got), flat(want), atol=1e-5, rtol=0)
    skip = ("elapsed_ms", "rows_per_sec", "entities")
    assert {k: v for k, v in got.items() if k not in skip} == {k: v for k, v in want.items() if k not in skip}


def test_op_output_both_forms(op):
    run, _ = op
    r = run({"texts": TEXTS, "model_path": MODEL, "max_entities": 5})
    for key in ("ok", "op", "model_path", "row_count", "elapsed_ms", "rows_per_sec", "aggregation", "max_entities",
                "entities", "entity_counts", "truncated"):
        assert key in r, key
    assert r["ok"] and r["op"] == "map_tag" and r["row_count"] == len(TEXTS) and r["aggregation"] == "simple"
    assert "dp_world_size" not in r and len(r["entities"]) == len(TEXTS) == len(r["entity_counts"])
    assert r["truncated"] == [i for i, c in enumerate(r["entity_counts"]) if c > 5] and r["truncated"]
    for text, row, c in zip(TEXTS, r["entities"], r["entity_counts"]):
        assert len(row) == min(c, 5)
        assert [e["start"] for e in row] == sorted(e["start"] for e in row)  # token order
        for e in row:
            assert set(e) == {"entity_group", "score", "word", "start", "end"}
            assert text[e["start"]:e["end"]] == e["word"] and e["entity_group"] in ("T0", "T1")
    json.dumps(r)
    one = run({"text": TEXTS[2], "model_path": MODEL, "max_entities": 5})
    assert one["row_count"] == 1 and len(one["entities"]) == 1
    _close(dict(one, row_count=0, entities=[one["entities"][0]], entity_counts=0, truncated=0),
           dict(r, row_count=0, entities=[r["entities"][2]], entity_counts=0, truncated=0))
    tok = run({"text": TEXTS[2], "model_path": MODEL, "aggregation": "none"})
    assert tok["max_entities"] == 64 and tok["entities"][0]
    for e in tok["entities"][0]:
        assert set(e) == {"entity", "score", "index", "word", "start", "end"} and e["entity"][:2] in ("B-", "I-")
    assert run({"texts": [], "model_path": MODEL})["entities"] == []
    # min_score drops entities but not their count
    scores = sorted(e["score"] for x in r["entities"] for e in x)
    cut = scores[len(scores) // 2]
    m = run({"texts": TEXTS, "model_path": MODEL, "max_entities": 5, "min_score": cut})
    assert m["entity_counts"] == r["entity_counts"]
    assert 0 < sum(map(len, m["entities"])) < sum(map(len, r["entities"]))
    assert all(e["score"] >= cut for x in m["entities"] for e in x)


def test_op_errors(op, small):
    run, _ = op
    from ops.map_tag import ERRORS

    base = {"text": "a b", "model_path": MODEL}
    cases = [({}, "missing"), ({"model_path": MODEL}, "missing"), (dict(base, texts=["a"]), "both"),
             (dict(base, text=5), "text"), ({"texts": "a"}, "texts"), ({"texts": ["a", 3]}, "texts"),
             (dict(base, aggregation="average"), "aggregation"), (dict(base, aggregation=1), "aggregation"),
             (dict(base, max_entities=0), "max_entities"), (dict(base, max_entities=513), "max_entities"),
             (dict(base, max_entities="3"), "max_entities"), (dict(base, max_entities=True), "max_entities"),
             (dict(base, min_score="0"), "min_score"), (dict(base, min_score=float("nan")), "min_score"),
             (dict(base, min_score=True), "min_score"),
             (dict(base, model_path="bert-tiny?batch=4&seq=40"), "tags"),
             (dict(base, aggregation="first"), "vocab")]
    seen = set()
    for payload, key in cases:
        with pytest.raises(ValueError) as e:
            run(payload)
        assert str(e.value) == ERRORS[key], (payload, key)
        seen.add(key)
    assert seen == set(ERRORS)
    assert run(dict(base, aggregation="first", model_path=MODEL + "&vocab=" + small[0]))["ok"]
    import ops.map_tag as mt

    contract = open(os.path.join(os.path.dirname(mt.__file__), "map_tag.CONTRACT.md")).read()
    for msg in ERRORS.values():
        assert msg in contract, msg
    for section in ("## Purpose", "## Inputs (payload)", "## Outputs", "## Notes"):
        assert section in contract


def test_model_specs(tmp_path):
    from safetensors.torch import save_file

    from ops._gpu_runtime import _load_host_pack, parse_spec

    assert parse_spec("bert-tiny").tags == 0 and parse_spec("bert-tiny?tags=9").tags == 9
    assert parse_spec("bert-tiny?tags=9").head is True and parse_spec("bert-tiny?tags=9").tag_names is None
    for bad in ("bert-tiny?tags=65", "bert-tiny?tags=-1"):
        with pytest.raises(ValueError):
            parse_spec(bad)
    assert ops.default_tag_names(5) == ["O", "B-T0", "I-T0", "B-T1", "I-T1"]
    names = ["O", "B-PER", "I-PER", "B-LOC", "I-LOC", "DATE", "X"]
    cfg = config_for("bert-tiny", tag_labels=len(names))
    pack = init_random(cfg, seed=4)
    tensors = {n: pack[n].clone() for n in pack.names() if not n.startswith(("pool_", "cls_"))}
    path = str(tmp_path / "ner.safetensors")
    save_file(tensors, path)
    with open(path + ".json", "w") as f:
        json.dump({"preset": "bert-tiny", "head": "token", "tag_labels": names, "outside": ["O", "X"]}, f)
    spec = parse_spec(path)
    assert spec.tags == 7 and spec.head is False and spec.qa is False
    assert spec.tag_names == tuple(names) and spec.tag_outside == ("O", "X")
    got = _load_host_pack(spec, config_for(spec.preset, num_labels=spec.labels, tag_labels=spec.tags))
    assert torch.equal(got["tag_w"], pack["tag_w"]) and not got["pool_w"].any() and not got["cls_w"].any()
    types, lt, lb = ops.tag_tables(spec.tag_names, spec.tag_outside)
    assert types == ["PER", "LOC", "DATE"] and lt.tolist() == [-1, 0, 0, 1, 1, 2, -1] and lb.tolist() == [0, 1, 0, 1, 0, 0, 0]
    # the other ops refuse it: a headless encoder for map_classify / map_rerank, no QA head for map_answer
    from types import SimpleNamespace

    from ops import map_answer, map_rerank

    with pytest.raises(ValueError) as e:
        map_rerank.check_model(SimpleNamespace(spec=spec), map_rerank.options({}))
    assert str(e.value) == map_rerank.ERRORS["head"]
    with pytest.raises(ValueError) as e:
        map_answer.check_model(SimpleNamespace(spec=spec), map_answer.options({}))
    assert str(e.value) == map_answer.ERRORS["qa"]
    with open(path + ".json", "w") as f:
        json.dump({"preset": "bert-tiny", "head": "token"}, f)
    with pytest.raises(ValueError, match="tag_labels"):
        parse_spec(path)
    del tensors["tag_w"]
    save_file(tensors, path)
    with pytest.raises(KeyError, match="tag_w"):
        _load_host_pack(spec, cfg)


def test_a_token_head_file_serves_map_tag_and_not_map_classify(tmp_path, monkeypatch):
    monkeypatch.setenv("CLASSIFY_DEVICE", "cpu")
    from safetensors.torch import save_file

    from ops import get_op

    names = ["O", "B-PER", "I-PER", "DATE"]
    cfg = config_for("bert-tiny", tag_labels=4)
    pack = init_random(cfg, seed=4)
    path = str(tmp_path / "ner.safetensors")
    save_file({n: pack[n].clone() for n in pack.names() if not n.startswith(("pool_", "cls_"))}, path)
    with open(path + ".json", "w") as f:
        json.dump({"preset": "bert-tiny", "head": "token", "tag_labels": names}, f)
    r = get_op("map_tag")({"text": TEXTS[2], "model_path": path + "?batch=4&seq=40", "aggregation": "none"})
    assert r["entities"][0] and {e["entity"] for e in r["entities"][0]} <= set(names[1:])
    g = get_op("map_tag")({"text": TEXTS[2], "model_path": path + "?batch=4&seq=40"})
    assert {e["entity_group"] for e in g["entities"][0]} <= {"PER", "DATE"}
    with pytest.raises(ValueError) as e:
        get_op("map_classify")({"texts": ["a"], "model_path": path + "?batch=4&seq=40", "allow_fallback": False})
    assert str(e.value) == "model has no classifier head"


def test_batched_jobs_equal_single_jobs(op):
    run, batch = op
    jobs = [{"texts": TEXTS, "model_path": MODEL, "max_entities": 3},
            {"text": 7},
            {"text": TEXTS[2], "model_path": MODEL, "max_entities": 3, "min_score": 0.3},
            {"texts": TEXTS[3:], "model_path": MODEL, "aggregation": "none"},
            {"texts": [], "model_path": MODEL},
            {"text": TEXTS[0], "model_path": MODEL, "aggregation": "first"},
            {"text": TEXTS[0], "model_path": "bert-tiny?batch=4&seq=40"}]
    res = batch(jobs)
    assert [r[0] for r in res] == ["ok", "err", "ok", "ok", "ok", "err", "err"]
    assert str(res[1][1]) == "payload.text must be a string" and isinstance(res[5][1], ValueError)
    for job, (kind, got) in zip(jobs, res):
        if kind == "ok":
            _close(got, run(job))
