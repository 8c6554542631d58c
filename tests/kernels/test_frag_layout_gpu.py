"""Encoder activations in fragment order (`ops.to_fragment_order`, ATPU_ACT_LAYOUT=4).

Fragment order re-orders the 16-byte units inside image order's 32 KiB images so that a lane's
packed accumulator fragment is the store unit: the producing epilogue drops its LDS transposes,
the consuming kernel's LDS A image is a verbatim copy. Values, MFMA operand order and the
epilogue's FMAs are those of the row-major kernels, so every test asks for bit-identical results
against the row-major call, after un-permuting on the host.

Shapes and the 8-workgroup grid are those of test_act_layout_gpu.py: each workgroup walks several
tiles (an odd number at M = 2304 or N = 768), so the residual prefetch issued in a tile's last
K-tile, the bias staging and the late statistics flush all cross tile boundaries.
"""
import pytest
import torch

from agent_tpu_amd import ops
from agent_tpu_amd._native import native
from agent_tpu_amd.models.bert import BertClassifier, config_for, init_random

pytestmark = pytest.mark.gpu

SHAPES = [(M, K, N) for M in (2048, 2304) for K, N in ((768, 3072), (3072, 768), (768, 768))]
LA, LC = ops.LAYOUT_A, ops.LAYOUT_C
FA, FC, FR = ops.LAYOUT_A_FRAG, ops.LAYOUT_C_FRAG, ops.LAYOUT_R_FRAG


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
    return ((1 + 0.2 * torch.randn(K, generator=gen)).to(dev), (0.1 * torch.randn(K, generator=gen)).to(dev))


def _nan(shape, dev, dtype=torch.bfloat16):
    return torch.full(shape, float("nan"), dtype=dtype, device=dev)


@pytest.mark.parametrize("lay", [FC, FA | FC])
@pytest.mark.parametrize("M,K,N", SHAPES)
def test_input_norm_gelu_fragment_order(gpu, few_cus, M, K, N, lay):
    """InNorm + GELU (FFN1): C, or A and C, in fragment order."""
    assert ops.image_order_ok()
    gen = torch.Generator().manual_seed(M + K + N)
    x = _rand((M, K), gen, 2.0, 0.5, dev=gpu)
    w = _rand((N, K), gen, 0.05, dev=gpu)
    b = (0.1 * torch.randn(N, generator=gen)).to(gpu)
    gam, bet = _ln_vecs(K, gen, gpu)
    wf, colsum, bf = ops.fold_ln_into_linear(w, b, gam, bet)
    fin = ops.ln_finalize(ops.ln_partials_ref(x.float()), K, 1e-12)
    ref = ops.linear_ln(x, wf, bf, act="gelu", in_fin=fin, colsum=colsum)
    out = _nan((M, N), gpu)
    ops.linear_ln(ops.to_fragment_order(x) if lay & LA else x, wf, bf, act="gelu", in_fin=fin, colsum=colsum,
                  out=out, layout=lay)
    assert torch.equal(ops.from_fragment_order(out), ref)


@pytest.mark.parametrize("lay", [LA | FR, LA | FC | FR, FA | FR, FA | FC | FR])
@pytest.mark.parametrize("M,K,N", SHAPES)
def test_residual_norm_stats_fragment_order(gpu, few_cus, M, K, N, lay):
    """ResNorm + StatsOut (out-proj, FFN2): A in image or fragment order, R in fragment order, C in
    fragment order or row-major; the output and its row statistics."""
    gen = torch.Generator().manual_seed(M + K + N + 1)
    a = _rand((M, K), gen, 1.0, dev=gpu)
    w = _rand((N, K), gen, 0.03, dev=gpu)
    b = (0.1 * torch.randn(N, generator=gen)).to(gpu)
    r = _rand((M, N), gen, 1.5, -0.2, dev=gpu)
    gam, bet = _ln_vecs(N, gen, gpu)
    fin = ops.ln_finalize(ops.ln_partials_ref(r.float()), N, 1e-12)
    part = _nan((N // 256, M, 2), gpu, torch.float32)
    ref = ops.linear_ln(a, w, b + bet, residual=r, res_fin=fin, res_gamma=gam, part_out=part)
    part_f, out = torch.full_like(part, float("nan")), _nan((M, N), gpu)
    a_in = ops.to_fragment_order(a) if lay & (FA & ~LA) else ops.to_image_order(a)
    ops.linear_ln(a_in, w, b + bet, residual=ops.to_fragment_order(r), res_fin=fin, res_gamma=gam, part_out=part_f,
                  out=out, layout=lay)
    assert torch.equal(ops.from_fragment_order(out) if lay & LC else out, ref)
    assert torch.equal(part_f, part)


@pytest.mark.parametrize("M,K,N", SHAPES)
def test_layer0_residual_and_plain_bias_fragment_order(gpu, few_cus, M, K, N):
    """Layer 0's out-proj form (a plain row-major residual, A in image order, C in fragment order), and
    plain bias with A and C in fragment order."""
    gen = torch.Generator().manual_seed(M + K + N + 2)
    a = _rand((M, K), gen, 1.0, dev=gpu)
    w = _rand((N, K), gen, 0.03, dev=gpu)
    b = (0.1 * torch.randn(N, generator=gen)).to(gpu)
    r = _rand((M, N), gen, 1.5, -0.2, dev=gpu)
    part = _nan((N // 256, M, 2), gpu, torch.float32)
    ref = ops.linear_ln(a, w, b, residual=r, part_out=part)
    part_f, out = torch.full_like(part, float("nan")), _nan((M, N), gpu)
    ops.linear_ln(ops.to_image_order(a), w, b, residual=r, part_out=part_f, out=out, layout=LA | FC)
    assert torch.equal(ops.from_fragment_order(out), ref) and torch.equal(part_f, part)
    out = _nan((M, N), gpu)
    ops.linear_ln(ops.to_fragment_order(a), w, b, out=out, layout=FA | FC)
    assert torch.equal(ops.from_fragment_order(out), ops.linear(a, w, b))


@pytest.mark.parametrize("M", [2048, 2304])
def test_ffn_pair_through_fragment_order(gpu, few_cus, M):
    """FFN1 -> FFN2 with input, intermediate, residual and output in fragment order."""
    H, I = 768, 3072
    gen = torch.Generator().manual_seed(M)
    a = _rand((M, H), gen, 2.0, 0.5, dev=gpu)
    w1, w2 = _rand((I, H), gen, 0.05, dev=gpu), _rand((H, I), gen, 0.03, dev=gpu)
    b1, b2 = (0.1 * torch.randn(I, generator=gen)).to(gpu), (0.1 * torch.randn(H, generator=gen)).to(gpu)
    gam, bet = _ln_vecs(H, gen, gpu)
    w1f, c1, b1f = ops.fold_ln_into_linear(w1, b1, gam, bet)
    fin = ops.ln_finalize(ops.ln_partials_ref(a.float()), H, 1e-12)
    part = _nan((H // 256, M, 2), gpu, torch.float32)
    ff = ops.linear_ln(a, w1f, b1f, act="gelu", in_fin=fin, colsum=c1)
    g = ops.linear_ln(ff, w2, b2 + bet, residual=a, res_fin=fin, res_gamma=gam, part_out=part)
    a_f, part_f = ops.to_fragment_order(a), torch.full_like(part, float("nan"))
    ff_f, g_f = _nan((M, I), gpu), _nan((M, H), gpu)
    ops.linear_ln(a_f, w1f, b1f, act="gelu", in_fin=fin, colsum=c1, out=ff_f, layout=FA | FC)
    ops.linear_ln(ff_f, w2, b2 + bet, residual=a_f, res_fin=fin, res_gamma=gam, part_out=part_f, out=g_f,
                  layout=FA | FC | FR)
    assert torch.equal(ops.from_fragment_order(ff_f), ff)
    assert torch.equal(ops.from_fragment_order(g_f), g) and torch.equal(part_f, part)


@pytest.mark.parametrize("B", [16, 18])
def test_qkv_attention_fragment_order_a(gpu, few_cus, B):
    """Fused QKV + attention with the raw hidden rows (A) in fragment order, ragged lens."""
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
    ref = ops.qkv_attention(x, wf, bf, lens, heads, in_fin=fin, colsum_h=colsum)
    assert torch.isfinite(ref.float()).all()
    ctx = _nan((M, H), gpu)
    ops.qkv_attention(ops.to_fragment_order(x), wf, bf, lens, heads, in_fin=fin, colsum_h=colsum, out=ctx,
                      layout=FA | LC)
    assert torch.equal(ops.from_image_order(ctx), ref)


@pytest.mark.parametrize("cls_only", [True, False])
def test_encode_folded_level4_bit_identical(gpu, cls_only):
    """3-layer H = 768 encoder at B = 16 (the last layer on the [CLS] rows, or in full): level 4 logits equal
    level 0 bit for bit."""
    cfg = config_for("bert-base", layers=3, num_labels=5)
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
    logits = {}
    for level in (0, 4):
        m.act_layout = level
        logits[level] = m.forward(ids.to(gpu), lens.to(gpu), k=3)[0]
    assert torch.isfinite(logits[0]).all()
    assert torch.equal(logits[0], logits[4])
