"""``minilm-l6`` at 2 layers (hidden 384, 12 heads of 32) on the GPU against its fp32 CPU oracle, 32 x 128 with mixed
lengths, and ``map_embed`` with the preset. Logit bounds: test_bert_gpu.py's. Embeddings: twice the error of the same
model on the CPU in bf16 against that oracle (test_embed_gpu.py has no absolute bound; docs/PERF_NOTES.md says why)."""
import pytest
import torch

from agent_tpu_amd import ops
from agent_tpu_amd.models.bert import BertClassifier, config_for, init_random

pytestmark = pytest.mark.gpu
B, S = 32, 128


@pytest.fixture(scope="module")
def case():
    cfg = config_for("minilm-l6", layers=2, num_labels=3)
    pack = init_random(cfg, seed=3, bias_std=0.02)
    ids = torch.randint(1000, cfg.vocab_size, (B, S), generator=torch.Generator().manual_seed(1), dtype=torch.int32)
    lens = torch.tensor([max(S - 5 * i, 2) for i in range(B)], dtype=torch.int32)
    lens[-1], lens[-2] = 1, S
    return cfg, pack, ids, lens, BertClassifier(cfg, pack, fp32=True), BertClassifier(cfg, pack)


@pytest.mark.parametrize("what", ["logits", "mean", "cls"])
def test_minilm_vs_fp32_oracle(gpu, case, what):
    cfg, pack, ids, lens, oracle, twin = case
    dev = BertClassifier(cfg, pack.to(gpu))
    assert not dev.can_fold(B, S)  # 384 is no multiple of 256: the unfolded encoder, attention_d32 + the w128 norms
    if what == "logits":
        rl, ri, rs = oracle.forward(ids, lens, k=3)
        gl, gi, _ = dev.forward(ids.to(gpu), lens.to(gpu), k=3)
        err, bound = (gl.cpu() - rl).abs().max().item(), 0.05 * rl.abs().max().item()
        ok = rs[:, 0] - rs[:, 1] > 0.02  # top-1 must agree where the oracle's margin is clear
        assert torch.equal(gi.cpu()[ok, 0], ri[ok, 0])
    else:
        ref = oracle.embed(ids, lens, what, True)
        bound = 2.0 * (twin.embed(ids, lens, what, True) - ref).abs().max().item()
        e = dev.embed(ids.to(gpu), lens.to(gpu), what, True)
        err = (e.cpu() - ref).abs().max().item()
    print(f"minilm {what}: err vs fp32 oracle {err:.3e}, bound {bound:.3e}")
    assert err < bound


def test_map_embed_op_minilm(gpu, monkeypatch):
    from ops.map_embed import map_embed

    monkeypatch.delenv("CLASSIFY_DEVICE", raising=False)
    prev = ops.set_batch_invariant(True)  # the op serves in this process-wide mode: put it back
    try:
        texts = [f"short text number {i} about row widths" for i in range(8)]
        r = map_embed({"texts": texts, "model_path": "minilm-l6?seed=1"})
    finally:
        ops.set_batch_invariant(prev)
    e = torch.tensor(r["embeddings"], dtype=torch.float64)
    assert r["ok"] and r["dim"] == 384 and e.shape == (8, 384)
    assert ((e.norm(dim=1) - 1.0).abs() <= 2e-5).all()  # fp32: 384 squares summed, <= 384 * 2^-24 / 2 on the root
