"""Re-associated [CLS] attention of the last BERT layer (ops/cls_attend.py), on the CPU.

The K / V projection of all keys is moved onto the one [CLS] query and into the
out-projection. These tests pin (a) the algebra in fp32 against the plain last layer and
(b) the numerics of the bf16 pipeline against today's path, both measured against fp64.
"""
import math

import pytest
import torch
import torch.nn.functional as F

from agent_tpu_amd import ops

S = 128


def _problem(H, heads, lens, seed, w_std, b_std):
    """Raw rows g (bf16 values), non-trivial LN gamma / beta and last-layer attention weights."""
    gen = torch.Generator().manual_seed(seed)
    B = len(lens)
    rnd = lambda *shape: torch.randn(*shape, generator=gen)  # noqa: E731
    g = (rnd(B * S, H) * (0.5 + rnd(B * S, 1).abs()) + 0.2 * rnd(B * S, 1)).bfloat16()
    gam, bet = 1 + 0.2 * rnd(H), 0.1 * rnd(H)
    qkv_w, o_w = (rnd(3 * H, H) * w_std).bfloat16(), (rnd(H, H) * w_std).bfloat16()
    qkv_b, o_b = rnd(3 * H) * b_std, rnd(H) * b_std
    return g, gam, bet, qkv_w, qkv_b, o_w, o_b, torch.tensor(lens, dtype=torch.int32)


def _plain(g, gam, bet, qkv_w, qkv_b, o_w, o_b, lens, heads, dtype, store=lambda t: t):
    """Today's path: LN, K/V projection of every token, Q of [CLS], attention, out-proj + residual.
    ``store`` rounds every tensor the GPU path writes to memory."""
    B, H = lens.numel(), g.shape[1]
    d = H // heads
    x = F.layer_norm(g.to(dtype), (H,), gam.to(dtype), bet.to(dtype), 1e-12)
    w, b = qkv_w.to(dtype), qkv_b.to(dtype)
    kv = store(x @ w[H:].t() + b[H:])                          # linear_ln output
    x0 = store(x.view(B, S, H)[:, 0])                          # h_cls
    q = store(x0 @ w[:H].t() + b[:H]).view(B, heads, 1, d)
    k = kv[:, :H].view(B, S, heads, d).transpose(1, 2)
    v = kv[:, H:].view(B, S, heads, d).transpose(1, 2)
    sc = (q @ k.transpose(2, 3)) / math.sqrt(d)
    dead = torch.arange(S).view(1, 1, 1, S) >= lens.view(B, 1, 1, 1)
    p = torch.softmax(sc.masked_fill(dead, float("-inf")), -1)
    ctx = store((p @ v).transpose(1, 2).reshape(B, H))
    return store(ctx @ o_w.to(dtype).t() + o_b.to(dtype) + x0)


def _fin(g, dtype=torch.float32):
    x = g.to(dtype)
    mu, var = x.mean(1), x.var(1, unbiased=False)
    rs = torch.rsqrt(var + 1e-12)
    return torch.stack([rs, rs * mu], -1).float().contiguous()


def _reassoc(g, gam, bet, qkv_w, qkv_b, o_w, o_b, lens, heads, wdtype, round_p, store=lambda t: t):
    B, H = lens.numel(), g.shape[1]
    cw = ops.cls_reassoc_weights(qkv_w, qkv_b, o_w, o_b, gam, bet, heads, dtype=wdtype)
    x0 = store(F.layer_norm(g.float().view(B, S, H)[:, 0], (H,), gam, bet, 1e-12))
    u = store(x0 @ cw["cls_wu"].float().t() + cw["cls_bu"])
    z = store(ops.cls_attend_ref(g, _fin(g), u, lens, heads, round_p=round_p))
    return store(z @ cw["cls_wz"].float().t() + cw["cls_bz"] + x0)


def test_reassociated_form_equals_plain_last_layer_fp32():
    H, heads = 256, 4
    prob = _problem(H, heads, [1, 2, 128, 77, 16], seed=3, w_std=0.05, b_std=0.05)
    ref = _plain(*prob, heads, torch.float32)
    got = _reassoc(*prob, heads, torch.float32, round_p=False)
    assert (got - ref).abs().max().item() <= 1e-5 * ref.abs().max().item()


def test_cls_attend_cpu_op_clamps_len_and_ignores_dead_rows():
    """ops.cls_attend on CPU tensors is the twin: len 0 acts as len 1, rows >= len may hold anything."""
    H, heads = 256, 4
    g, *_ = _problem(H, heads, [0, 5], seed=4, w_std=0.05, b_std=0.0)
    gen = torch.Generator().manual_seed(5)
    u = (torch.randn(2, heads * H, generator=gen) * 0.1).bfloat16()
    lens = torch.tensor([0, 5], dtype=torch.int32)
    z = ops.cls_attend(g, _fin(g), u, lens, heads)
    g2 = g.clone().view(2, S, H)
    g2[0, 1:] = float("nan")
    g2[1, 5:] = float("inf")
    z2 = ops.cls_attend(g2.view(-1, H), _fin(g), u, lens, heads)
    assert z.dtype == torch.bfloat16 and torch.isfinite(z.float()).all() and torch.equal(z, z2)
    z1 = ops.cls_attend(g, _fin(g), u, torch.tensor([1, 5], dtype=torch.int32), heads)
    assert torch.equal(z, z1)
    # one live key: Z_h is that key's normalised row for every head
    x0 = F.layer_norm(g.float()[:1], (H,), None, None, 1e-12)
    torch.testing.assert_close(z.float()[0].view(heads, H), x0.expand(heads, H), rtol=2 ** -7, atol=2 ** -7)


@pytest.mark.parametrize("w_std,b_std,seed", [(0.02, 0.0, 11), (0.02, 0.05, 12), (0.1, 0.0, 13), (0.1, 0.05, 14)])
def test_bf16_pipeline_error_is_within_1p5x_of_todays_path(w_std, b_std, seed):
    """bf16 rounding at every tensor either GPU path stores (H = 768, 12 heads, ragged lens):
    the re-associated out-projection output may be at most 1.5x as far from fp64 as today's."""
    H, heads = 768, 12
    prob = _problem(H, heads, [128, 1, 2, 61, 127, 16, 99, 33], seed, w_std, b_std)
    ref = _plain(*prob, heads, torch.float64)
    bf = lambda t: t.bfloat16().float()  # noqa: E731
    old = _plain(*prob, heads, torch.float32, store=bf)
    new = _reassoc(*prob, heads, torch.bfloat16, round_p=True, store=bf)
    e_old = (old.double() - ref).abs().max().item()
    e_new = (new.double() - ref).abs().max().item()
    print(f"w_std={w_std} b_std={b_std}: err old {e_old:.3e} new {e_new:.3e} ratio {e_new / e_old:.3f}")
    assert e_new <= 1.5 * e_old, (e_new, e_old)
