"""Encoder activations in K-tile image order ([M/256][W/64][256][64], `ops.to_image_order`).

The layout changes global addressing only (LDS images, MFMA order and the epilogue math are
those of the row-major kernels), so every test asks for bit-identical results: the image-order
output, un-permuted on the host, must `torch.equal` the row-major output of the same call.

Shapes: M = 2048 (8 row tiles) and 2304 (9); N, K in {768, 3072}. The persistent grid is
held to 8 workgroups (`cu_budget`), so each workgroup walks several tiles, an odd number of
them at M = 2304 or N = 768 (24 / 27 / 96 / 108 tiles over 8 workgroups): the DMA stream runs
on from one tile's image into the next one's, and row statistics are flushed a tile late.
"""
import pytest
import torch

from agent_tpu_amd import ops
from agent_tpu_amd._native import native
from agent_tpu_amd.models.bert import BertClassifier, config_for, init_random

pytestmark = pytest.mark.gpu

SHAPES = [(M, K, N) for M in (2048, 2304) for K, N in ((768, 3072), (3072, 768), (768, 768))]


@pytest.fixture
def few_cus():
    nat = native()
    nat.cu_budget(8)
    try:
        yield
    finally:
        nat.cu_budget(0)


def _rand(shape, gen, scale=1.0, shift=0.0, dtype=torch.bfloat16, dev="cuda"):
    return (torch.randn(shape, generator=gen) * scale + shift).to(dtype).to(dev)


def _ln_vecs(K, gen, dev):
    # non-trivial gamma / beta
    return ((1 + 0.2 * torch.randn(K, generator=gen)).to(dev), (0.1 * torch.randn(K, generator=gen)).to(dev))


LA, LC, LR = ops.LAYOUT_A, ops.LAYOUT_C, ops.LAYOUT_R


@pytest.mark.parametrize("lay", [LC, LA | LC])
@pytest.mark.parametrize("M,K,N", SHAPES)
def test_input_norm_gelu_image_order(gpu, few_cus, M, K, N, lay):
    """InNorm + GELU (FFN1): C, or A and C, in image order."""
    assert ops.image_order_ok()
    gen = torch.Generator().manual_seed(M + K + N)
    x = _rand((M, K), gen, 2.0, 0.5, dev=gpu)
    w = _rand((N, K), gen, 0.05, dev=gpu)
    b = (0.1 * torch.randn(N, generator=gen)).to(gpu)
    gam, bet = _ln_vecs(K, gen, gpu)
    wf, colsum, bf = ops.fold_ln_into_linear(w, b, gam, bet)
    fin = ops.ln_finalize(ops.ln_partials_ref(x.float()), K, 1e-12)
    ref = ops.linear_ln(x, wf, bf, act="gelu", in_fin=fin, colsum=colsum)
    img = torch.full((M, N), float("nan"), dtype=torch.bfloat16, device=gpu)
    ops.linear_ln(ops.to_image_order(x) if lay & LA else x, wf, bf, act="gelu", in_fin=fin, colsum=colsum, out=img,
                  layout=lay)
    assert torch.equal(ops.from_image_order(img), ref)


@pytest.mark.parametrize("lay", [LA, LA | LR, LA | LC | LR])
@pytest.mark.parametrize("M,K,N", SHAPES)
def test_residual_norm_stats_image_order(gpu, few_cus, M, K, N, lay):
    """ResNorm + StatsOut with residual (FFN2, out-proj): A, A and R, or all three in image order."""
    gen = torch.Generator().manual_seed(M + K + N + 1)
    a = _rand((M, K), gen, 1.0, dev=gpu)
    w = _rand((N, K), gen, 0.03, dev=gpu)
    b = (0.1 * torch.randn(N, generator=gen)).to(gpu)
    r = _rand((M, N), gen, 1.5, -0.2, dev=gpu)
    gam, bet = _ln_vecs(N, gen, gpu)
    fin = ops.ln_finalize(ops.ln_partials_ref(r.float()), N, 1e-12)
    part = torch.full((N // 256, M, 2), float("nan"), device=gpu)
    ref = ops.linear_ln(a, w, b + bet, residual=r, res_fin=fin, res_gamma=gam, part_out=part)
    part_i = torch.full_like(part, float("nan"))
    a_img, r_img = ops.to_image_order(a), ops.to_image_order(r)
    y = ops.linear_ln(a_img, w, b + bet, residual=r_img if lay & LR else r, res_fin=fin, res_gamma=gam,
                      part_out=part_i, layout=lay)
    assert torch.equal(ops.from_image_order(y) if lay & LC else y, ref) and torch.equal(part_i, part)
    if lay & LR:
        return
    # without ResNorm (layer 0's out-proj form: the residual is the row-major embedding output)
    ref = ops.linear_ln(a, w, b, residual=r, part_out=part)
    for lay0 in (LA, LA | LC):
        part_i.fill_(float("nan"))
        y = ops.linear_ln(a_img, w, b, residual=r, part_out=part_i, layout=lay0)
        assert torch.equal(ops.from_image_order(y) if lay0 & LC else y, ref) and torch.equal(part_i, part)


@pytest.mark.parametrize("M,K,N", SHAPES)
def test_plain_bias_image_order(gpu, few_cus, M, K, N):
    """Plain bias: A, C, and both in image order."""
    gen = torch.Generator().manual_seed(M + K + N + 2)
    a = _rand((M, K), gen, 1.0, dev=gpu)
    w = _rand((N, K), gen, 0.03, dev=gpu)
    b = (0.1 * torch.randn(N, generator=gen)).to(gpu)
    ref = ops.linear(a, w, b)
    a_img = ops.to_image_order(a)
    assert torch.equal(ops.linear_ln(a_img, w, b, layout=ops.LAYOUT_A), ref)
    assert torch.equal(ops.from_image_order(ops.linear_ln(a, w, b, layout=ops.LAYOUT_C)), ref)
    assert torch.equal(ops.from_image_order(ops.linear_ln(a_img, w, b, layout=ops.LAYOUT_A | ops.LAYOUT_C)), ref)


@pytest.mark.parametrize("M", [2048, 2304])
def test_ffn_pair_through_image_order(gpu, few_cus, M):
    """FFN1 -> FFN2 with the intermediate in image order: the pair's output and statistics."""
    H, I = 768, 3072
    gen = torch.Generator().manual_seed(M)
    a = _rand((M, H), gen, 2.0, 0.5, dev=gpu)
    w1, w2 = _rand((I, H), gen, 0.05, dev=gpu), _rand((H, I), gen, 0.03, dev=gpu)
    b1, b2 = (0.1 * torch.randn(I, generator=gen)).to(gpu), (0.1 * torch.randn(H, generator=gen)).to(gpu)
    gam, bet = _ln_vecs(H, gen, gpu)
    w1f, c1, b1f = ops.fold_ln_into_linear(w1, b1, gam, bet)
    fin = ops.ln_finalize(ops.ln_partials_ref(a.float()), H, 1e-12)
    outs = []
    for img in (False, True):
        part = torch.full((H // 256, M, 2), float("nan"), device=gpu)
        ff = ops.linear_ln(a, w1f, b1f, act="gelu", in_fin=fin, colsum=c1, layout=ops.LAYOUT_C if img else 0)
        g = ops.linear_ln(ff, w2, b2 + bet, residual=a, res_fin=fin, res_gamma=gam, part_out=part,
                          layout=ops.LAYOUT_A if img else 0)
        outs.append((g, part))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])


@pytest.mark.parametrize("B", [16, 18])
def test_qkv_attention_out_proj_image_order(gpu, few_cus, B):
    """Fused QKV + attention -> out-proj: the context in image order (and the raw hidden rows, as the
    fused kernel's A operand and the out-proj's residual), then the layer output."""
    H, heads, S = 768, 12, 128
    M = B * S
    gen = torch.Generator().manual_seed(B)
    x = _rand((M, H), gen, 2.0, 0.5, dev=gpu)
    lens = torch.randint(1, S + 1, (B,), generator=gen, dtype=torch.int32)
    lens[0], lens[1], lens[B - 1] = 1, S, 77
    lens = lens.to(gpu)
    gam, bet = _ln_vecs(H, gen, gpu)
    w = _rand((3 * H, H), gen, 0.05, dev=gpu)  # taken as head-ordered already
    b = (0.1 * torch.randn(3 * H, generator=gen)).to(gpu)
    wf, colsum, bf = ops.fold_ln_into_linear(w, b, gam, bet)
    fin = ops.ln_finalize(ops.ln_partials_ref(x.float()), H, 1e-12)
    ow = _rand((H, H), gen, 0.03, dev=gpu)
    ob = (0.1 * torch.randn(H, generator=gen)).to(gpu)
    x_img = ops.to_image_order(x)
    # layer 0 form (plain bias, row-major A) and the InNorm form
    ref0 = ops.qkv_attention(x, w, b, lens, heads)
    assert torch.equal(ops.from_image_order(ops.qkv_attention(x, w, b, lens, heads, layout=LC)), ref0)
    ref = ops.qkv_attention(x, wf, bf, lens, heads, in_fin=fin, colsum_h=colsum)
    assert torch.isfinite(ref.float()).all()
    ctx_c = ops.qkv_attention(x, wf, bf, lens, heads, in_fin=fin, colsum_h=colsum, layout=LC)
    ctx_ac = ops.qkv_attention(x_img, wf, bf, lens, heads, in_fin=fin, colsum_h=colsum, layout=LA | LC)
    assert torch.equal(ops.from_image_order(ctx_c), ref) and torch.equal(ctx_ac, ctx_c)
    # the layer output: out-proj + LN(residual) + statistics
    part = torch.full((H // 256, M, 2), float("nan"), device=gpu)
    part_i = torch.full_like(part, float("nan"))
    a_ref = ops.linear_ln(ref, ow, ob + bet, residual=x, res_fin=fin, res_gamma=gam, part_out=part)
    a1 = ops.linear_ln(ctx_c, ow, ob + bet, residual=x, res_fin=fin, res_gamma=gam, part_out=part_i, layout=LA)
    assert torch.equal(a1, a_ref) and torch.equal(part_i, part)
    part_i.fill_(float("nan"))
    a2 = ops.linear_ln(ctx_ac, ow, ob + bet, residual=x_img, res_fin=fin, res_gamma=gam, part_out=part_i,
                       layout=LA | LC | LR)
    assert torch.equal(ops.from_image_order(a2), a_ref) and torch.equal(part_i, part)


@pytest.mark.parametrize("cls_only", [True, False])
def test_encode_folded_switch_bit_identical(gpu, cls_only):
    """H = 768 encoder with two full layers at B = 16 (a third on the [CLS] rows, or none), the switch at
    every level vs off: logits equal bit for bit."""
    cfg = config_for("bert-base", layers=3 if cls_only else 2, num_labels=5)
    pack = init_random(cfg, seed=5, bias_std=0.02)
    g = torch.Generator().manual_seed(3)
    for name in pack.names():
        if name.endswith("_g"):
            pack[name].copy_(1 + 0.1 * torch.randn(pack[name].shape, generator=g))
        elif name.endswith("ln_b") or name.endswith("ln1_b") or name.endswith("ln2_b"):
            pack[name].copy_(0.05 * torch.randn(pack[name].shape, generator=g))
    B, S = 16, 128
    ids = torch.randint(1000, cfg.vocab_size, (B, S), generator=g, dtype=torch.int32)
    ids[:, 0] = 101
    lens = torch.randint(1, S + 1, (B,), generator=g, dtype=torch.int32)
    lens[0], lens[1] = 1, S
    ids[torch.arange(S).view(1, S) >= lens.view(B, 1)] = 0
    m = BertClassifier(cfg, pack.to(gpu), cls_only_last=cls_only)
    assert m.can_fold(B, S) and ops.image_order_ok()
    logits = []
    for level in (0, 1, 2, 3):
        m.act_layout = level
        logits.append(m.forward(ids.to(gpu), lens.to(gpu), k=3)[0])
    assert torch.isfinite(logits[0]).all()
    for level in (1, 2, 3):
        assert torch.equal(logits[0], logits[level]), level
