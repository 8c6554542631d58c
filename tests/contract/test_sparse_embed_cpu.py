"""map_sparse_embed on CPU engines: the model chain against BertForMaskedLM; the op's forms, errors and batching."""
import os

import numpy as np
import pytest
import torch

from agent_tpu_amd import tokenizer as T
from agent_tpu_amd.models.bert import BertClassifier, config_for, from_hf_state_dict
from agent_tpu_amd.utils.synthetic import make_text_rows

MODEL = "bert-tiny?mlm=1&batch=4&seq=40&seed=3"
TEXTS = make_text_rows(5, words_per_row=7, seed=8) + ["", "lorem ipsum " * 30]
CONTRACT = os.path.join(os.path.dirname(__file__), "..", "..", "ops", "map_sparse_embed.CONTRACT.md")


def test_terms_match_hf_masked_lm():
    """log1p(relu(max over the attention mask of BertForMaskedLM's logits)), selected in the total order."""
    transformers = pytest.importorskip("transformers")
    hcfg = transformers.BertConfig(vocab_size=4096, hidden_size=256, num_hidden_layers=2, num_attention_heads=4,
                                   intermediate_size=1024, max_position_embeddings=512, type_vocab_size=2,
                                   hidden_act="gelu", layer_norm_eps=1e-12, attn_implementation="eager",
                                   tie_word_embeddings=True)
    torch.manual_seed(13)
    hf = transformers.BertForMaskedLM(hcfg).eval()
    with torch.no_grad():
        for p in hf.parameters():  # our pack stores bf16 weights: give HF the same values
            p.copy_(p.bfloat16().float())
        hf.cls.predictions.bias.copy_(torch.linspace(-0.5, 0.5, 4096))
    cfg = config_for("bert-tiny", mlm_head=True)
    ours = BertClassifier(cfg, from_hf_state_dict(cfg, hf.state_dict(), head="mlm"), fp32=True)
    S, k, atol = 64, 48, 2e-4
    ids, lens = T.tokenize_rows([t.encode() for t in make_text_rows(6, words_per_row=12, seed=4) + [""]], S, 4096)
    mask = torch.from_numpy(np.arange(S)[None, :] < lens[:, None])
    with torch.no_grad():
        logits = hf(input_ids=torch.from_numpy(ids).long(), attention_mask=mask.long()).logits
        tok, xs, w, nnz = ours.terms(torch.from_numpy(ids), torch.from_numpy(lens), k)
    x = logits.masked_fill(~mask[:, :, None], float("-inf")).amax(1)
    assert (tok >= 0).all() and (nnz > k).all() and (xs[:, :-1] >= xs[:, 1:]).all()
    torch.testing.assert_close(xs, torch.gather(x, 1, tok.long()), atol=atol, rtol=1e-4)
    torch.testing.assert_close(w, torch.log1p(xs))
    assert ((nnz - (x > 0).sum(1)).abs() <= ((x.abs() <= atol).sum(1))).all()
    for b in range(tok.shape[0]):  # every HF term that clears the list's last x by twice the atol is in the list
        assert set(torch.nonzero(x[b] > xs[b, -1] + 2 * atol).view(-1).tolist()) <= set(tok[b].tolist())


@pytest.fixture()
def op(monkeypatch):
    monkeypatch.setenv("CLASSIFY_DEVICE", "cpu")
    from ops import get_batch_op, get_op
    return get_op("map_sparse_embed"), get_batch_op("map_sparse_embed")


def _close(got, want):
    # the weights up to the last bits: the PyTorch reference path is not batch-invariant
    assert [t["token_ids"] for t in got["terms"]] == [t["token_ids"] for t in want["terms"]]
    np.testing.assert_allclose(sum((t["weights"] for t in got["terms"]), []),
                               sum((t["weights"] for t in want["terms"]), []), atol=1e-6, rtol=0)
    skip = ("elapsed_ms", "rows_per_sec", "terms")
    assert {k: v for k, v in got.items() if k not in skip} == {k: v for k, v in want.items() if k not in skip}


def test_op_output_forms_prefix_and_min_weight(op):
    run = op[0]
    r = run({"texts": TEXTS, "model_path": MODEL, "max_terms": 40})
    assert r["ok"] and r["op"] == "map_sparse_embed" and r["row_count"] == 7 and r["max_terms"] == 40
    assert r["vocab_size"] == config_for("bert-tiny").vocab_size and len(r["terms"]) == len(r["nnz"]) == 7
    for t, n in zip(r["terms"], r["nnz"]):
        ws, ids = t["weights"], t["token_ids"]
        assert len(ids) == min(n, 40) > 0 and t["tokens"] is None and all(x > 0 for x in ws)
        assert all(a > b or (a == b and i < j) for a, b, i, j in zip(ws, ws[1:], ids, ids[1:]))
    _close(run({"text": TEXTS[1], "model_path": MODEL, "max_terms": 40}),
           dict(r, row_count=1, terms=r["terms"][1:2], nnz=r["nnz"][1:2]))
    assert run({"texts": [], "model_path": MODEL})["terms"] == []
    small = run({"texts": TEXTS, "model_path": MODEL, "max_terms": 7})  # a total order: top-k is a prefix of top-K
    _close(small, dict(r, max_terms=7, terms=[{"token_ids": t["token_ids"][:7], "tokens": None,
                                               "weights": t["weights"][:7]} for t in r["terms"]]))
    cut = r["terms"][0]["weights"][20]
    mw = run({"texts": TEXTS, "model_path": MODEL, "max_terms": 40, "min_weight": cut})
    assert mw["nnz"] == r["nnz"] and all(x >= cut for t in mw["terms"] for x in t["weights"])
    assert mw["terms"][0]["token_ids"] == r["terms"][0]["token_ids"][:21]


BAD = [({}, "missing"), ({"text": "a", "texts": ["b"]}, "both"), ({"text": 5}, "text"), ({"texts": "a"}, "texts"),
       ({"text": "a", "max_terms": 0}, "max_terms"), ({"text": "a", "max_terms": 1025}, "max_terms"),
       ({"text": "a", "min_weight": -1}, "min_weight"), ({"text": "a", "min_weight": float("inf")}, "min_weight"),
       ({"text": "a", "model_path": "bert-tiny?batch=4&seq=40"}, "mlm")]


@pytest.mark.parametrize("payload,key", BAD)
def test_op_errors(op, payload, key):
    from ops.map_sparse_embed import ERRORS
    with pytest.raises(ValueError) as e:
        op[0](dict({"model_path": MODEL}, **payload))
    assert str(e.value) == ERRORS[key]
    with open(CONTRACT, encoding="utf-8") as f:
        assert "`" + ERRORS[key] + "`" in f.read() and {k for _, k in BAD} == set(ERRORS)


def test_batched_jobs_equal_single_jobs(op):
    jobs = [{"texts": TEXTS[:3], "model_path": MODEL, "max_terms": 16}, {"text": 5, "model_path": MODEL},
            {"text": TEXTS[4], "model_path": MODEL, "max_terms": 16, "min_weight": 0.01},
            {"texts": TEXTS[3:], "model_path": MODEL, "max_terms": 9}]
    res = op[1](jobs)
    assert [r[0] for r in res] == ["ok", "err", "ok", "ok"] and str(res[1][1]) == "payload.text must be a string"
    for i in (0, 2, 3):
        _close(res[i][1], op[0](jobs[i]))
