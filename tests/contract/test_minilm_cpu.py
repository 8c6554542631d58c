"""``minilm-l6`` (hidden 384, 12 heads of 32) on the CPU oracle against transformers; head_dim 32 attention in fp64."""
import math

import pytest
import torch

from agent_tpu_amd import ops
from agent_tpu_amd.models.bert import BertClassifier, config_for, from_hf_state_dict


@pytest.mark.parametrize("cls_only_last", [True, False])
def test_minilm_logits_match_hf(cls_only_last):
    transformers = pytest.importorskip("transformers")
    hcfg = transformers.BertConfig(vocab_size=4096, hidden_size=384, num_hidden_layers=2, num_attention_heads=12,
                                   intermediate_size=1536, max_position_embeddings=512, type_vocab_size=2,
                                   num_labels=3, hidden_act="gelu", layer_norm_eps=1e-12, attn_implementation="eager")
    torch.manual_seed(3)
    hf = transformers.BertForSequenceClassification(hcfg).eval()
    with torch.no_grad():
        for p in hf.parameters():  # our pack stores bf16 weights: give HF the same values
            p.copy_(p.bfloat16().float())
    cfg = config_for("minilm-l6", layers=2, vocab_size=4096, num_labels=3)
    ours = BertClassifier(cfg, from_hf_state_dict(cfg, hf.state_dict()), fp32=True, cls_only_last=cls_only_last)
    B, S, lens = 4, 64, torch.tensor([64, 40, 7, 2])
    ids = torch.randint(1000, 4096, (B, S), generator=torch.Generator().manual_seed(1))
    mask = (torch.arange(S).view(1, S) < lens.view(B, 1)).long()
    ids = ids * mask
    ids[:, 0] = 101
    with torch.no_grad():
        ref = hf(input_ids=ids, attention_mask=mask).logits
        logits, _, _ = ours.forward(ids.to(torch.int32), lens.to(torch.int32), 3)
    torch.testing.assert_close(logits.float(), ref, atol=2e-4, rtol=1e-4)


@pytest.mark.parametrize("Sq,Skv", [(16, 16), (1, 40), (130, 130)])
def test_attention_head_dim_32_by_definition(Sq, Skv):
    B, H, D = 3, 12, 32
    g = torch.Generator().manual_seed(Sq + Skv)
    q, k, v = (torch.randn((B * s, H * D), generator=g) for s in (Sq, Skv, Skv))
    lens = torch.tensor([Skv, 1, Skv // 2], dtype=torch.int32)
    out = ops.attention(q, k, v, lens, B, Sq, Skv, H, head_dim=D)
    qd, kd, vd = (t.double().view(B, -1, H, D) for t in (q, k, v))
    s = torch.einsum("bqhd,bkhd->bhqk", qd, kd) / math.sqrt(D)
    s = s.masked_fill(torch.arange(Skv).view(1, 1, 1, Skv) >= lens.view(B, 1, 1, 1), float("-inf"))
    ref = torch.einsum("bhqk,bkhd->bqhd", torch.softmax(s, -1), vd).reshape(B * Sq, H * D)
    torch.testing.assert_close(out.double(), ref, atol=1e-5, rtol=1e-5)  # fp32 op against fp64
