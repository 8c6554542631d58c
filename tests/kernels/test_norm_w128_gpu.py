"""LayerNorm (with / without residual) and embedding LayerNorm at odd multiples of 128 columns (the 128-column
kernels of norm_embed.hip) against fp32 ``layer_norm``, at the bound test_kernels_gpu.py holds the other widths to."""
import pytest
import torch
import torch.nn.functional as F

from agent_tpu_amd import ops

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("op", ["ln", "ln_res", "embed"])
@pytest.mark.parametrize("N,B,S", [(384, 8, 125), (384, 17, 59), (640, 7, 11)])  # 1000, 1003, 77 rows (partial block)
def test_w128(gpu, N, B, S, op):
    torch.manual_seed(N + S)
    bf = lambda *shape: torch.randn(shape).to(torch.bfloat16)  # noqa: E731
    g, b = torch.randn(N), torch.randn(N)
    if op == "embed":
        word, pos, typ = bf(1000, N), bf(128, N), bf(2, N)
        ids, tt = torch.randint(0, 1000, (B, S), dtype=torch.int32), torch.randint(0, 2, (B, S), dtype=torch.int32)
        y = ops.embed_layernorm(*(t.to(gpu) for t in (ids, word, pos, typ, g, b)), 1e-12, type_ids=tt.to(gpu))
        x = word.float()[ids.long()] + pos.float()[:S].unsqueeze(0) + typ.float()[tt.long()]
    else:
        xb, r = bf(B * S, N) * 2, bf(B * S, N)
        y = ops.layernorm(xb.to(gpu), g.to(gpu), b.to(gpu), 1e-12, residual=r.to(gpu) if op == "ln_res" else None)
        x = xb.float() + (r.float() if op == "ln_res" else 0.0)
    ref = F.layer_norm(x, (N,), g, b, 1e-12).reshape(B * S, N)
    assert ((y.float().cpu() - ref).abs().max() / (ref.abs().max() + 1e-6)).item() < 1e-2
