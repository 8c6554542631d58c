"""Head-dim-32 attention (csrc/kernels/attention_d32.hip): the packed one-chunk route and the general chunked route
against the fp32 reference from the same bf16 inputs, cases whose result is exact in bf16, and batch invariance."""
import pytest
import torch

from agent_tpu_amd import ops
from agent_tpu_amd.ops.attention import attention_ref

pytestmark = pytest.mark.gpu
D, BIG = 32, 3.0e4  # BIG: poison, large and finite, so a masked weight of exactly 0 still hides it


_rel_err = lambda a, b: ((a.float().cpu() - b).abs().max() / (b.abs().max() + 1e-6)).item()  # noqa: E731
_rand = lambda shape, seed: torch.randn(shape, generator=torch.Generator().manual_seed(seed)).bfloat16()  # noqa: E731


@pytest.mark.parametrize("H", [1, 3, 12])
@pytest.mark.parametrize("S", [16, 48, 128])
def test_packed_route(gpu, S, H):
    B, hd = 3, H * D
    qkv = _rand((B * S, 3 * hd), seed=S + H)
    lens = torch.tensor([S, 1, 17 if S > 17 else S - 1], dtype=torch.int32)
    out = ops.attention_packed(qkv.to(gpu), lens.to(gpu), B, S, H, head_dim=D)
    f = qkv.float()
    ref = attention_ref(f[:, :hd], f[:, hd:2 * hd], f[:, 2 * hd:], lens, B, S, S, H, D ** -0.5, head_dim=D)
    assert out.shape == (B * S, hd) and _rel_err(out, ref) < 2e-2


@pytest.mark.parametrize("Sq,Skv", [(1, 128), (1, 130), (130, 130), (40, 300)])
def test_general_route_strided(gpu, Sq, Skv):
    B, H, hd = 3, 3, 3 * D
    qw, kvw = _rand((B * Sq, hd + 64), seed=Sq), _rand((B * Skv, 2 * hd + 96), seed=Skv)
    cut = lambda a, b: (a[:, 32:32 + hd], b[:, 8:8 + hd], b[:, 16 + hd:16 + 2 * hd])  # noqa: E731
    lens = torch.tensor([127, 128, 129], dtype=torch.int32).clamp(max=Skv)  # across the 128-key chunk edge
    out = ops.attention(*cut(qw.to(gpu), kvw.to(gpu)), lens.to(gpu), B, Sq, Skv, H, head_dim=D)
    ref = attention_ref(*cut(qw.float(), kvw.float()), lens, B, Sq, Skv, H, D ** -0.5, head_dim=D)
    assert _rel_err(out, ref) < 2e-2


@pytest.mark.parametrize("H", [3, 12])
@pytest.mark.parametrize("values", ["head", "onehot"])
def test_exact_uniform_weights(gpu, H, values):
    """q = 0: every live weight is exactly 1 and 1/len exact. V = h tells heads and pairs apart, V[j, d] = (j % 32 == d)
    keys, chunks and d-tiles. Keys >= len and the columns past 3*H*32 hold BIG."""
    lens, B, S, hd = torch.tensor([1, 2, 64, 128], dtype=torch.int32), 4, 128, H * D
    live = (torch.arange(S).view(1, S, 1, 1) < lens.view(B, 1, 1, 1)).expand(B, S, H, D)
    if values == "head":
        v = torch.arange(H, dtype=torch.float32).view(1, 1, H, 1).expand(B, S, H, D)
    else:
        v = (torch.arange(S).view(1, S, 1, 1) % D == torch.arange(D).view(1, 1, 1, D)).float().expand(B, S, H, D)
    want = ((v * live).sum(1, keepdim=True) / lens.view(B, 1, 1, 1)).expand(B, S, H, D).reshape(B, S, hd)
    wide = torch.full((B * S, 3 * hd + 64), BIG)
    wide[:, :hd] = 0.0
    wide[:, hd:2 * hd] = torch.where(live, torch.tensor(1.0), torch.tensor(BIG)).reshape(B * S, hd)
    wide[:, 2 * hd:3 * hd] = torch.where(live, v, torch.tensor(BIG)).reshape(B * S, hd)
    w, dl = wide.to(torch.bfloat16).to(gpu), lens.to(gpu)
    q, k, v = w[:, :hd], w[:, hd:2 * hd], w[:, 2 * hd:3 * hd]
    packed = ops.attention(q, k, v, dl, B, S, S, H, head_dim=D)
    first = ops.attention(q.view(B, S, hd)[:, :5].reshape(B * 5, hd), k, v, dl, B, 5, S, H, head_dim=D)  # general route
    want = want.to(torch.bfloat16)
    assert torch.equal(packed.cpu().view(B, S, hd), want) and torch.equal(first.cpu().view(B, 5, hd), want[:, :5])


@pytest.mark.parametrize("Sq,Skv", [(128, 128), (40, 300)])  # the packed and the general route
def test_batch_invariance(gpu, Sq, Skv):
    B, H, hd, packed = 3, 12, 12 * D, Sq == Skv
    qkv = _rand((B * Skv, 3 * hd), seed=5).to(gpu)
    q = qkv[:, :hd] if packed else _rand((B * Sq, hd), seed=6).to(gpu)
    lens = torch.tensor([Skv, Skv - 9, 3], dtype=torch.int32, device=gpu)
    full = ops.attention(q, qkv[:, hd:2 * hd], qkv[:, 2 * hd:], lens, B, Sq, Skv, H, head_dim=D)
    one = qkv[Skv:2 * Skv].contiguous()
    q1 = one[:, :hd] if packed else q[Sq:2 * Sq]
    alone = ops.attention(q1, one[:, hd:2 * hd], one[:, 2 * hd:], lens[1:2].contiguous(), 1, Sq, Skv, H, head_dim=D)
    assert torch.equal(full[Sq:2 * Sq], alone)
