"""cls_attend (csrc/kernels/cls_attend.hip) against its PyTorch twin, and the re-associated
[CLS] last layer of the folded BERT encoder against ATPU_CLS_REASSOC=0 and the fp32 oracle.

Tolerance of the kernel tests: the kernel's own bf16 output rounding (2^-8 relative) plus the
fp32 twin's measured error against the fp64 twin on the same inputs (the twin rounds the
softmax weights to bf16 as the kernel does, fp64 does not).
"""
import pytest
import torch

from agent_tpu_amd import ops
from agent_tpu_amd.models.bert import BertClassifier, BertConfig, config_for, init_random

pytestmark = pytest.mark.gpu

S = 128
LENS = [1, 2, 15, 16, 17, 127, 128]
CONFIGS = [(256, 4), (768, 12)]
_cache = {}


def _case(H, heads, B):
    """Inputs (CPU), the fp32 twin's output and its max error against fp64: computed once."""
    key = (H, heads, B)
    if key not in _cache:
        gen = torch.Generator().manual_seed(H + B)
        lens = torch.tensor([LENS[(3 * i + B) % len(LENS)] for i in range(B)], dtype=torch.int32)
        g = (torch.randn(B * S, H, generator=gen) * (0.5 + torch.randn(B * S, 1, generator=gen).abs())
             + 0.3 * torch.randn(B * S, 1, generator=gen)).bfloat16()
        x = g.float()
        rs = torch.rsqrt(x.var(1, unbiased=False) + 1e-12)
        fin = torch.stack([rs, rs * x.mean(1)], -1).contiguous()
        u = (torch.randn(B, heads * H, generator=gen) * 0.15).bfloat16()
        twin = ops.cls_attend_ref(g, fin, u, lens, heads)
        exact = ops.cls_attend_ref(g, fin, u, lens, heads, dtype=torch.float64, round_p=False)
        _cache[key] = (g, fin, u, lens, twin, (twin.double() - exact).abs().max().item())
    return _cache[key]


@pytest.mark.parametrize("B", [1, 3, 17])
@pytest.mark.parametrize("H,heads", CONFIGS)
def test_cls_attend_matches_twin(gpu, H, heads, B):
    g, fin, u, lens, twin, twin_err = _case(H, heads, B)
    dg = g.to(gpu).view(B, S, H).clone()
    for b in range(B):  # rows >= len are never read: poison them
        dg[b, int(lens[b]):] = float("nan")
    z = ops.cls_attend(dg.view(B * S, H), fin.to(gpu), u.to(gpu), lens.to(gpu), heads)
    torch.cuda.synchronize()
    assert z.shape == (B, heads * H) and z.dtype == torch.bfloat16
    diff = (z.float().cpu() - twin).abs()
    tol = 2.0 ** -8 * twin.abs() + twin_err
    print(f"H={H} B={B}: max diff {diff.max().item():.3e} twin err vs fp64 {twin_err:.3e}")
    assert torch.isfinite(z.float()).all() and (diff <= tol).all(), (diff - tol).max().item()
    z2 = ops.cls_attend(dg.view(B * S, H), fin.to(gpu), u.to(gpu), lens.to(gpu), heads)
    assert torch.equal(z, z2)  # bit-equal run to run


@pytest.mark.parametrize("H,heads", CONFIGS)
def test_cls_attend_sequence_bits_do_not_depend_on_batch(gpu, H, heads):
    g, fin, u, lens, _, _ = _case(H, heads, 17)
    z17 = ops.cls_attend(g.to(gpu), fin.to(gpu), u.to(gpu), lens.to(gpu), heads)
    for b in (0, 5, 16):
        z1 = ops.cls_attend(g[b * S:(b + 1) * S].to(gpu), fin[b * S:(b + 1) * S].to(gpu).contiguous(),
                            u[b:b + 1].to(gpu), lens[b:b + 1].to(gpu), heads)
        assert torch.equal(z1[0], z17[b]), b


def test_cls_attend_rejects_unsupported_shapes(gpu):
    g = torch.zeros((S, 320), dtype=torch.bfloat16, device=gpu)
    fin = torch.ones((S, 2), device=gpu)
    with pytest.raises(ValueError):
        ops.cls_attend(g, fin, torch.zeros((1, 5 * 320), dtype=torch.bfloat16, device=gpu),
                       torch.ones(1, dtype=torch.int32, device=gpu), 5)


def _model_case(cfg, seed):
    pack = init_random(cfg, seed=seed, bias_std=0.02)
    gen = torch.Generator().manual_seed(seed + 1)
    for name in pack.names():
        if name.endswith("_g"):
            pack[name].copy_(1 + 0.1 * torch.randn(pack[name].shape, generator=gen))
        elif name.endswith("ln_b") or name.endswith("ln1_b") or name.endswith("ln2_b"):
            pack[name].copy_(0.05 * torch.randn(pack[name].shape, generator=gen))
    B = 16
    ids = torch.randint(1000, cfg.vocab_size, (B, S), generator=gen, dtype=torch.int32)
    ids[:, 0] = 101
    lens = torch.tensor([2, 3, 15, 16, 17, 31, 40, 64, 65, 90, 100, 111, 120, 127, 128, 128], dtype=torch.int32)
    ids[torch.arange(S).view(1, S) >= lens.view(B, 1)] = 0
    return pack, ids, lens


@pytest.mark.parametrize("name", ["bert-tiny", "h768-2layer"])
def test_reassociated_last_layer_logits(gpu, name, monkeypatch):
    """B = 16, S = 128 (the smallest batch the folded encoder takes): the new path's logit error
    against the fp32 CPU oracle is at most 1.5x that of ATPU_CLS_REASSOC=0 on the same rows, and
    top-1 agrees with the oracle wherever its margin exceeds 0.02."""
    cfg = (config_for("bert-tiny", num_labels=3) if name == "bert-tiny"
           else BertConfig(vocab_size=4096, hidden=768, layers=2, heads=12, intermediate=3072, num_labels=3))
    pack, ids, lens = _model_case(cfg, seed=31)
    oracle = BertClassifier(cfg, pack, fp32=True)
    rl, _, rs = oracle.forward(ids, lens, k=3)
    dpack = pack.to(gpu)
    out = {}
    for flag in ("0", "1"):
        monkeypatch.setenv("ATPU_CLS_REASSOC", flag)
        m = BertClassifier(cfg, dpack)
        assert m.can_fold(16, S) and m.cls_only_last and m.cls_reassoc == (flag == "1")
        assert ("cls_wu" in m.folded()) == (flag == "1")
        lg, idx, _ = m.forward(ids.to(gpu), lens.to(gpu), k=3)
        out[flag] = (lg.float().cpu(), idx.cpu())
    e_old = (out["0"][0] - rl).abs().max().item()
    e_new = (out["1"][0] - rl).abs().max().item()
    print(f"{name}: logit err vs fp32 oracle: reassoc off {e_old:.3e} on {e_new:.3e} ratio {e_new / e_old:.3f}")
    assert e_new <= 1.5 * e_old, (e_new, e_old)
    sure = (rs[:, 0] - rs[:, 1]) > 0.02
    top = rl.argmax(-1).to(out["1"][1].dtype)
    assert torch.equal(out["1"][1][sure, 0], top[sure])
